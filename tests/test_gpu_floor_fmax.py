"""The floor-max forward kernel (one target per lane, forward_form 1) forms the frame maximum M with LDS float atomics into
slot groups that rotate every frame, and stores M into pad column S of the history row, where the back-trace reads it.
These cases aim at what that can get wrong: the first frames and every position of the rotation and of the unrolled
frame loop (lengths 1-13, 25), frame maxima that sit on the extra column (excluded from M), delta rows full of ties and
signed zeros, other wave counts and extra-column counts, and the wide windows (four frames unrolled).  Every case is
decoded bit for bit against the CPU oracle and against a kernel that does not use M (the scan form, forward_form 3, or
the dense kernel where the scan form is not built)."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests.common import GEN
from tests.test_plan_host import _banded_matrix
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

SHORT = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 25]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _check(dec, A, pi, E, lens, tag, other="scan", signed_zero_loglik=True):
    """The floor form against the oracle and against `other`: paths bit for bit, log-likelihoods bit for bit (by value
    where the case allows both signs of zero)."""
    ref_s, ref_l = vo.decode_c(A, pi, E.float().cpu().numpy(), lengths=lens.cpu().numpy())
    out = {}
    for run in ("floor", other):
        dec.set_option("forward_form", {"floor": 1, "scan": 3}.get(run, 0))
        st, ll = dec.decode(E, lengths=lens, algo="dense" if run == "dense" else "group", out_dtype=torch.int32)
        dec.set_option("reset", 0)
        st, ll = st.cpu().numpy(), ll.cpu().numpy()
        assert np.array_equal(st, ref_s), (tag, run)
        if signed_zero_loglik:
            assert np.array_equal(_bits(ll), _bits(ref_l)), (tag, run, ll, ref_l)
        else:
            assert np.array_equal(ll, ref_l), (tag, run, ll, ref_l)
        out[run] = (st, ll)
    assert np.array_equal(out["floor"][0], out[other][0]), tag
    if signed_zero_loglik:
        assert np.array_equal(_bits(out["floor"][1]), _bits(out[other][1])), tag


def _tonet(S=361):
    return synth.log_params(synth.tonet_transition(S - 1, 14), synth.floored_prior(S))


def test_floor_kernel_is_the_one_tested(dev):
    A, pi = _tonet()
    dec = ViterbiDecoder(A, pi, dev)
    assert dec.info["floor_ok"] and dec.info["group_window"] == 32 and dec.info["extras"] == [360]


def test_short_lengths_every_rotation_position(dev):
    """Lengths 1-13 and 25 in one batch: frame 0 alone, each slot group and delta buffer as the last one written, the
    unrolled loop's tail after zero, one and two full rounds of twelve frames."""
    A, pi = _tonet()
    dec = ViterbiDecoder(A, pi, dev)
    for kind in ("peaks", "ties", "dense"):
        E = GEN[kind](len(SHORT), max(SHORT), 361, seed=31, device=dev)
        lens = torch.tensor(SHORT, dtype=torch.int64, device=dev)
        _check(dec, A, pi, E, lens, kind)
        # the longest song of the batch this short as well (T itself is 1, 2, 12, 13, 25; no lengths tensor)
        for T in (1, 2, 12, 13, 25):
            E2 = E[:2, :T].contiguous()
            _check(dec, A, pi, E2, torch.tensor([T, T], dtype=torch.int64, device=dev), (kind, T))


def test_frame_maximum_on_the_extra_column(dev):
    """The unvoiced state (the extra column) holds the frame maximum on most frames; M must be the maximum over the voiced
    states only.  Voiced frames in between let the row-constant term win after an unvoiced stretch."""
    A, pi = _tonet()
    dec = ViterbiDecoder(A, pi, dev)
    x = dec.info["extras"][0]
    B, T = 6, 400
    rng = np.random.default_rng(7)
    E = synth.emissions_peaks(B, T, 361, seed=8).cpu().numpy().copy()
    unv = rng.random((B, T)) < 0.8
    E[:, :, x] = np.where(unv, E.max(axis=2) + rng.integers(1, 40, (B, T)).astype(np.float32) / 4, E[:, :, x])
    E = torch.from_numpy(E.astype(np.float32)).to(dev)
    lens = torch.tensor([T, T - 1, 13, 25, 2, 1], dtype=torch.int64, device=dev)
    _check(dec, A, pi, E, lens, "unvoiced max")


def test_ties_and_signed_zeros(dev):
    """Band entries of +0 and -0, a prior of +-0 and emissions of +-0 on most frames: delta rows of exact ties whose
    maxima are +0 or -0.  Paths bit for bit; the log-likelihood by value (+0 and -0 are the same maximum)."""
    rng = np.random.default_rng(3)
    S = 361
    A = _banded_matrix(S, 10, rng, extras=(S - 1,), floor=-50.0, quant=2)
    zero = A == 0
    A[zero] = np.where(rng.random(int(zero.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    pi = np.where(rng.random(S) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    dec = ViterbiDecoder(A, pi, dev)
    assert dec.info["floor_ok"] and dec.info["group_window"] == 32
    B, T = 5, 60
    Ez = np.where(rng.random((B, T, S)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    Ez[:, ::7] = -(rng.integers(0, 3, (B, len(range(0, T, 7)), S)) / 2).astype(np.float32)
    E = torch.from_numpy(Ez).to(dev)
    lens = torch.tensor([T, 13, 25, 1, 12], dtype=torch.int64, device=dev)
    _check(dec, A, pi, E, lens, "signed zeros", signed_zero_loglik=False)


@pytest.mark.parametrize("S,half,n_extras", [(100, 5, 0), (150, 9, 2), (300, 14, 1), (450, 12, 1), (700, 7, 3)])
def test_other_wave_and_extra_counts(dev, S, half, n_extras):
    """Two to twelve waves, no extra column or several (the general extras path), short and ragged lengths."""
    rng = np.random.default_rng(S)
    extras = sorted(int(v) for v in rng.choice(S, n_extras, replace=False))
    A = _banded_matrix(S, half, rng, extras=extras, floor=-50.0, quant=2)
    pi = -(rng.integers(0, 8, S) / 2).astype(np.float32)
    dec = ViterbiDecoder(A, pi, dev)
    assert dec.info["floor_ok"] and dec.info["n_dense_rows"] == 0, dec.info
    E = torch.from_numpy(-(rng.integers(0, 6, (len(SHORT), 40, S)) / 2).astype(np.float32)).to(dev)
    lens = torch.tensor(SHORT[:-1] + [40], dtype=torch.int64, device=dev)
    _check(dec, A, pi, E, lens, (S, half, extras))


@pytest.mark.parametrize("d_max,W", [(40, 84), (56, 128)])
def test_wide_windows_short_lengths(dev, d_max, W):
    """The wide windows unroll four frames (PF = 4): every rotation position at lengths 1-13 and 25, against the dense
    kernel (no scan form is built for these widths)."""
    A, pi = synth.log_params(synth.tonet_transition(720, d_max), synth.floored_prior(721))
    dec = ViterbiDecoder(A, pi, dev)
    assert dec.info["floor_ok"] and dec.info["group_window"] == W
    E = synth.emissions_peaks(len(SHORT), max(SHORT), 721, seed=d_max, device=dev, dtype=torch.float16)
    lens = torch.tensor(SHORT, dtype=torch.int64, device=dev)
    _check(dec, A, pi, E, lens, W, other="dense")
