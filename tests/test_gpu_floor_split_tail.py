"""The split-window floor forward kernel (forward_form 6) whose full waves issue their four copy stores and the quad maximum's DPP
steps as one statement, and whose trimmed window has its fences reshaped, must not change a bit: raw history rows [B, T, SD]
after zeroing the workspace (pad column S carries the frame maximum M, pad column S + 1 the idle slots' -inf), paths and
log-likelihood bits, against the one-target kernel (forward_form 1) and against the CPU oracle.  Every instantiation the launcher
reaches: WF = 29 (S = 361), WF = 25 (S = 321), the whole window (WF = 32: "floor_live_window" 1, and fp16 emissions), at every
boundary of the twelve-frame prefetch round (interior rounds, the clamped round, every tail length, frame 0 alone).  Each
emission set's premise is checked on the CPU with the oracle before anything runs on the GPU."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests.test_floor_trim_host import _tonet, _widths
from tests.test_gpu_floor_split_trim import _bits, _run
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

B = 3
TS = (1, 2, 12, 13, 14, 25, 26, 37, 61)       # the round boundaries at twelve rows in flight: tails 0, 1, 11, 0 (+ 1 round), 1, ...
TMAX = max(TS)
FULL_LAST_LANES = (63, 127, 191, 255)         # lane 63 of the four full waves
GRIDS = {361: 29, 321: 25}                    # states -> live width the full waves run at


def _lengths(T):
    return [T, max(1, T - 1), max(1, T // 2)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


_decoders = {}


def _decoder(S, dev):
    if S not in _decoders:
        A, pi = _tonet(S)
        assert _widths(A, pi) == (GRIDS[S], GRIDS[S]), (S, _widths(A, pi))
        dec = ViterbiDecoder(A, pi, dev)
        assert dec.info["floor_ok"] and dec.info["group_window"] == 32 and dec.info["n_dense_rows"] == 0, dec.info
        _decoders[S] = (A, pi, dec)
    return _decoders[S]


def _frame_deltas(A, pi, E):
    """delta_t of every song and frame from the oracle (its final delta row on every prefix): [B, T, S]."""
    return np.stack([vo.decode_c(A, pi, E[:, :t + 1], return_delta=True)[2] for t in range(E.shape[1])], axis=1)


def _half_targets(S):
    """Live non-extra targets of the half waves (the extra column is S - 1), spread over the four of them."""
    return {361: [256, 287, 293, 327, 352, 359], 321: [256, 287, 288, 293, 310, 319]}[S]


def _emissions(kind, S, A, pi):
    """[B, TMAX, S] float32 and the premise, asserted here on the CPU."""
    rng = np.random.default_rng(1000 * S + len(kind))
    if kind == "peaks":
        return synth.emissions_peaks(B, TMAX, S, seed=17).cpu().numpy()
    if kind == "inf":
        # whole columns at -inf for the whole song (a full wave's lane 0 and lane 63, half-wave targets, the last state before the
        # extra column), scattered -inf entries, and song 1 dead from frame 5 on (frame 5 is -inf in every column)
        E = -(rng.integers(0, 6, (B, TMAX, S)) / 2).astype(np.float32)
        E[rng.random((B, TMAX, S)) < 0.2] = -np.inf
        cols = [0, 63, 64, 200, 255, 256, 263, 300, S - 2]
        E[:, :, cols] = -np.inf
        E[:, :, 100] = -1.0
        E[1, 5] = -np.inf
        st, ll, _ = vo.decode_c(A, pi, E, return_delta=True)
        assert np.isneginf(ll[1]) and np.isfinite(ll[0]) and np.isfinite(ll[2]), ll
        assert not np.isin(st[[0, 2]], cols).any(), "a live song's path runs through a -inf column"
        d = _frame_deltas(A, pi, E)
        assert np.isneginf(d[1, 5:]).all() and np.isfinite(d[1, :5]).any(axis=1).all()
        assert np.isneginf(d[[0, 2]][:, :, cols]).all()
        return E
    assert kind == "alternate"
    # the frame maximum over the non-extra states sits in a half-wave target on one frame and in lane 63 of a full wave on the next
    # (songs start in different phases): M then comes out of another slot of the group from frame to frame
    E = -(rng.integers(0, 7, (B, TMAX, S)) / 2).astype(np.float32)
    half = _half_targets(S)
    want = np.empty((B, TMAX), np.int64)
    for b in range(B):
        for t in range(TMAX):
            k = t + b
            want[b, t] = half[(k // 2) % len(half)] if k % 2 == 0 else FULL_LAST_LANES[(k // 2) % 4]
            E[b, t, want[b, t]] = 200.0                      # (more than any transition costs: the grids' floor is -87.3)
    d = _frame_deltas(A, pi, E)[:, :, :S - 1]
    assert np.array_equal(d.argmax(axis=2), want), "the frame maximum is not where the emissions put it"
    top = np.sort(d, axis=2)
    assert (top[:, :, -1] > top[:, :, -2]).all(), "the frame maximum is tied"
    assert all(w >= 256 for w in half) and S - 1 not in half
    return E


_cases = {}


def _case(S, kind, dev):
    if (S, kind) not in _cases:
        A, pi, _ = _decoder(S, dev)
        _cases[(S, kind)] = _emissions(kind, S, A, pi)
    return _cases[(S, kind)]


def _compare(dec, A, pi, Enp, dev, whole, f16, tag):
    for T in TS:
        lens_np = np.array(_lengths(T), np.int64)
        Ecut = np.ascontiguousarray(Enp[:, :T])
        if f16:
            E16 = Ecut.astype(np.float16)
            Eref, E = E16.astype(np.float32), torch.from_numpy(E16).to(dev)
        else:
            Eref, E = Ecut, torch.from_numpy(Ecut).to(dev)
        lens = torch.from_numpy(lens_np).to(dev)
        ref_s, ref_l = vo.decode_c(A, pi, Eref, lengths=lens_np)
        st, ll, h = _run(dec, E, lens, 6, whole)
        st1, ll1, h1 = _run(dec, E, lens, 1, 0)
        for b in range(B):
            n = int(lens_np[b])
            assert np.array_equal(st[b, :n], ref_s[b, :n]), (tag, T, b, "path differs from the oracle")
        assert np.array_equal(_bits(ll), _bits(ref_l)), (tag, T, ll, ref_l)
        assert np.array_equal(st, st1) and np.array_equal(_bits(ll), _bits(ll1)), (tag, T, "differs from the one-target kernel")
        assert h.shape[2] >= Enp.shape[2] + 2
        assert np.array_equal(h, h1), (tag, T, "history rows differ from the one-target kernel", np.argwhere(h != h1)[:8])


@pytest.mark.parametrize("kind", ["peaks", "inf", "alternate"])
@pytest.mark.parametrize("whole", [0, 1], ids=["live", "whole"])
@pytest.mark.parametrize("S", list(GRIDS))
def test_split_tail_is_bit_exact(dev, S, whole, kind):
    """WF = 29 / 25 ("live") and WF = 32 ("whole") of the fp32 split kernel."""
    A, pi, dec = _decoder(S, dev)
    _compare(dec, A, pi, _case(S, kind, dev), dev, whole, False, (S, whole, kind))


@pytest.mark.parametrize("kind", ["peaks", "inf", "alternate"])
@pytest.mark.parametrize("S", list(GRIDS))
def test_split_tail_is_bit_exact_fp16(dev, S, kind):
    """The fp16 instantiation (whole window), which only forward_form 6 reaches.  The "inf" and "alternate" sets are multiples of
    1 / 2 below 2048 or -inf, exact in fp16, so their premises hold for the stored emissions as checked."""
    A, pi, dec = _decoder(S, dev)
    E = _case(S, kind, dev)
    if kind != "peaks":
        assert np.array_equal(E.astype(np.float16).astype(np.float32), E)
    _compare(dec, A, pi, E, dev, 0, True, (S, "fp16", kind))
