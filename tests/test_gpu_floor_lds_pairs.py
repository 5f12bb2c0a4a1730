"""The delta-copy layout of the floor forward kernels (FloorLds: four shifted copies per buffer, two buffers, four frame-maximum
slot groups) at the smallest shapes at which the copy stride, the per-copy write offsets and the tail of the twelve-frame unroll can
go wrong.  The split kernel (forward_form 6) and the one-target kernel (forward_form 1) share that layout: they must leave the same
raw history rows, paths and log-likelihoods, byte for byte, and both must decode what the CPU oracle decodes.  tonet-recipe matrices
with d_max 12 and 14 at S = 361 and 321 (the shipped grids) and S = 257 and 383 (the first and the last split target sit at the edges of
the half waves); B = 3; T = 1, 2, 13, 14, 25, 50: T - 1 below, equal to and just above one unrolled round of twelve, a tail of either
parity, both delta buffers and all four slot groups.  fp32 emissions for both kernels, fp16 for the one-target kernel: the emissions
lie on the fp16 grid, so the fp16 run must leave the very same bytes."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

SIZES = (361, 321, 257, 383)
DMAX = (12, 14)
LENGTHS = (1, 2, 13, 14, 25, 50)
B, TMAX = 3, 50


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _waves_for(S):          # kernels.hpp banded_waves_for
    return next((w for w in (2, 4, 6, 8, 12) if w >= (S + 63) // 64), 0)


_CASES = {}


def _case(S, dmax, dev):
    """(A, pi, decoder, emissions [B, TMAX, S] as float32 on the fp16 grid), built once per (S, d_max) and left unchanged."""
    if (S, dmax) not in _CASES:
        A, pi = synth.log_params(synth.tonet_transition(S - 1, dmax), synth.floored_prior(S))
        dec = ViterbiDecoder(A, pi, dev)
        assert dec.info["floor_ok"] and dec.info["group_window"] == 32 and dec.info["n_dense_rows"] == 0, dec.info
        # forward_form 6 runs the split kernel on the six-wave grids only (elsewhere the launcher takes the one-target kernel, and
        # the comparison below would hold one kernel against itself)
        assert _waves_for(S) == 6 and S < 64 * 6, S
        E = synth.emissions_peaks(B, TMAX, S, seed=100 * S + dmax).to(torch.float16).to(torch.float32).numpy().copy()
        E.setflags(write=False)
        _CASES[S, dmax] = (A, pi, dec, E)
    return _CASES[S, dmax]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _run(dec, E, lens, form):
    """-> (paths, log-likelihoods, raw history rows [B, T, SD] as int32) of forward kernel `form`.  The history is read after a
    forward pass into a zeroed workspace: rows past a song's length and pad columns nobody writes compare equal."""
    n, T, S = E.shape
    dec.set_option("forward_form", form)
    st, ll = dec.decode(E, lengths=lens, algo="group", out_dtype=torch.int32)
    st, ll = st.cpu().numpy(), ll.cpu().numpy()
    st_d = torch.empty((n, T), dtype=torch.int32, device=E.device)
    ll_d = torch.empty((n,), dtype=torch.float32, device=E.device)
    dec.decode_into(E, st_d, ll_d, lengths=lens, algo="group", phase="forward")      # allocates the workspace
    torch.cuda.synchronize()
    dec._ws.zero_()
    dec.decode_into(E, st_d, ll_d, lengths=lens, algo="group", phase="forward")
    torch.cuda.synchronize()
    dec.set_option("reset", 0)
    SD = (S + 5) // 4 * 4
    pad = (-dec._ws.data_ptr()) % 256
    hist = dec._ws[pad:pad + n * T * SD * 4].view(torch.int32).view(n, T, SD).cpu().numpy().copy()
    return st, ll, hist


def _check(A, pi, dec, E32, lens, dev, tag):
    """E32: float32 emissions on the fp16 grid (numpy).  Split fp32, one-target fp32 and one-target fp16 against the oracle and
    against each other."""
    ref_s, ref_l = vo.decode_c(A, pi, E32, lengths=lens)
    E = torch.from_numpy(np.array(E32, np.float32)).to(dev)          # (a copy: the shared emissions are read-only)
    ln = None if lens is None else torch.from_numpy(np.asarray(lens, np.int64)).to(dev)
    runs = {"split f32": _run(dec, E, ln, 6), "one-target f32": _run(dec, E, ln, 1),
            "one-target f16": _run(dec, E.to(torch.float16), ln, 1)}
    for name, (st, ll, _) in runs.items():
        assert np.array_equal(st, ref_s), (tag, name, "paths differ from the oracle's")
        assert np.array_equal(_bits(ll), _bits(ref_l)), (tag, name, ll, ref_l)
    h6 = runs["split f32"][2]
    for name in ("one-target f32", "one-target f16"):
        h = runs[name][2]
        assert np.array_equal(h6, h), (tag, name, "history rows differ from the split kernel's", np.argwhere(h6 != h)[:8])
    return ref_s, ref_l


@pytest.mark.parametrize("dmax", DMAX)
@pytest.mark.parametrize("S", SIZES)
def test_split_and_one_target_leave_the_same_bytes(dev, S, dmax):
    A, pi, dec, E = _case(S, dmax, dev)
    for T in LENGTHS:
        _check(A, pi, dec, E[:, :T], None, dev, (S, dmax, T))


@pytest.mark.parametrize("S", SIZES)
def test_ragged_lengths(dev, S):
    """Songs of 14, 50 and 1 frames in one batch of T = 50."""
    A, pi, dec, E = _case(S, 14, dev)
    _check(A, pi, dec, E, np.asarray([14, TMAX, 1], np.int64), dev, (S, "ragged"))


@pytest.mark.parametrize("S,dmax", [(361, 14), (257, 12), (383, 14)])
def test_song_with_one_live_state(dev, S, dmax):
    """Song 1's emissions are -inf everywhere except one state (the first split target, where there is one): every other delta of
    that song is -inf from frame 0 on, the frame maximum is that state's, and the song still ends finite on it."""
    A, pi, dec, E0 = _case(S, dmax, dev)
    live = 256 if S > 257 else S // 2
    E = E0.copy()
    E[1] = -np.inf
    E[1, :, live] = E0[1, :, live]
    for T in (14, TMAX):
        ref_s, ref_l = _check(A, pi, dec, E[:, :T], None, dev, (S, dmax, T, "one live state"))
        assert np.all(ref_s[1] == live) and np.isfinite(ref_l[1]), (ref_s[1], ref_l[1])
