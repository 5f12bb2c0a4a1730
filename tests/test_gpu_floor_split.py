"""The split-window floor forward kernel (forward_form 6: eight waves, waves 4-7 evaluate half a window per lane and join
the halves in registers) must decode what the one-target kernel (forward_form 1) and the scan form (forward_form 3)
decode, bit for bit, and leave the same history: every case is checked against the CPU oracle and against both, through
full decodes with the default back-trace and the one-stream-per-lane back-trace (both read the history rows and the frame
maximum in pad column S), and the raw history rows are compared byte for byte as well.  The cases aim at what the split
can get wrong: the first and the last target of the half waves and their wave boundaries, every tail of the unrolled frame
loop, maxima on an extra column / on the last full-wave target / on the first half-wave target, ties across the 15/16
source boundary of a split window, signed zeros and -inf emissions."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests.common import GEN
from tests.test_plan_host import _banded_matrix
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

SHORT = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 25]


def _waves_for(S):          # kernels.hpp banded_waves_for
    return next((w for w in (2, 4, 6, 8, 12) if w >= (S + 63) // 64), 0)


# the last S that takes six waves and leaves the idle slot the floor forms need (S < 64 * waves)
S_LAST = max(S for S in range(257, 64 * 6) if _waves_for(S) == 6)
SIZES = sorted({257, 288, 289, 320, 321, 361, 383, S_LAST})


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _history(dec, E, lens, form):
    """The history rows [B, T, SD] the forward kernel `form` leaves (workspace zeroed first: rows past a song's length and
    the pad columns nobody writes then compare equal)."""
    B, T, S = E.shape
    st = torch.empty((B, T), dtype=torch.int32, device=E.device)
    ll = torch.empty((B,), dtype=torch.float32, device=E.device)
    dec.set_option("forward_form", form)
    dec.decode_into(E, st, ll, lengths=lens, algo="group", phase="forward")      # allocates the workspace
    torch.cuda.synchronize()
    dec._ws.zero_()
    dec.decode_into(E, st, ll, lengths=lens, algo="group", phase="forward")
    torch.cuda.synchronize()
    dec.set_option("reset", 0)
    SD = (S + 5) // 4 * 4
    pad = (-dec._ws.data_ptr()) % 256
    return dec._ws[pad:pad + B * T * SD * 4].view(torch.int32).view(B, T, SD).cpu().numpy().copy()


def _check(dec, A, pi, E, lens, tag, loglik_bits=True, history=True):
    """forward_form 6 against the oracle and against forms 1 and 3, default and per-lane back-trace."""
    assert dec.info["floor_ok"] and dec.info["group_window"] == 32 and dec.info["n_dense_rows"] == 0, (tag, dec.info)
    ref_s, ref_l = vo.decode_c(A, pi, E.float().cpu().numpy(), lengths=None if lens is None else lens.cpu().numpy())
    out = {}
    for form in (6, 1, 3):
        for bt in (0, 4):
            dec.set_option("forward_form", form)
            dec.set_option("backtrace_form", bt)
            st, ll = dec.decode(E, lengths=lens, algo="group", out_dtype=torch.int32)
            dec.set_option("reset", 0)
            st, ll = st.cpu().numpy(), ll.cpu().numpy()
            assert np.array_equal(st, ref_s), (tag, form, bt)
            if loglik_bits:
                assert np.array_equal(_bits(ll), _bits(ref_l)), (tag, form, bt, ll, ref_l)
            else:
                assert np.array_equal(ll, ref_l), (tag, form, bt, ll, ref_l)
            out[form, bt] = (st, ll)
    for key, (st, ll) in out.items():
        assert np.array_equal(st, out[6, 0][0]), (tag, key)
        assert np.array_equal(_bits(ll), _bits(out[6, 0][1])), (tag, key)
    if history:
        h6, h1 = _history(dec, E, lens, 6), _history(dec, E, lens, 1)
        assert np.array_equal(h6, h1), (tag, "history rows differ", np.argwhere(h6 != h1)[:8])


def _matrix(S, rng, n_extras=1, half=None, quant=2):
    extras = [S - 1] if n_extras == 1 else sorted(int(v) for v in rng.choice(S, n_extras, replace=False))
    A = _banded_matrix(S, half or int(rng.integers(9, 15)), rng, extras=extras, floor=-50.0, quant=quant)
    pi = -(rng.integers(0, 8, S) / 2).astype(np.float32)
    return A, pi, extras


def test_sizes_cover_the_six_wave_range():
    assert S_LAST == 383 and _waves_for(256) == 4 and _waves_for(384) == 6 and _waves_for(385) == 8


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_sizes_short_and_ragged_lengths(dev, S, dtype):
    """Every S of interest, lengths 1-13 and 25 ragged in one batch (every tail of the twelve-frame unroll and of the
    slot-group rotation), and the same lengths as the batch's own T."""
    rng = np.random.default_rng(S)
    A, pi, _ = _matrix(S, rng)
    dec = ViterbiDecoder(A, pi, dev)
    E = torch.from_numpy(-(rng.integers(0, 6, (len(SHORT), 40, S)) / 2).astype(np.float32)).to(dev).to(dtype)
    lens = torch.tensor(SHORT[:-1] + [40], dtype=torch.int64, device=dev)
    _check(dec, A, pi, E, lens, (S, "ragged"))
    for T in (1, 2, 12, 13, 25):
        _check(dec, A, pi, E[:2, :T].contiguous(), None, (S, T), history=False)


@pytest.mark.parametrize("kind", ["peaks", "ties", "dense"])
@pytest.mark.parametrize("S", [321, 361])
def test_shipped_grids(dev, S, kind):
    A, pi = synth.log_params(synth.tonet_transition(S - 1, 14 if S == 361 else 12), synth.floored_prior(S))
    dec = ViterbiDecoder(A, pi, dev)
    assert dec.info["extras"] == [S - 1]
    E = GEN[kind](len(SHORT), 300, S, seed=5, device=dev)
    lens = torch.tensor(SHORT[:-2] + [299, 300], dtype=torch.int64, device=dev)
    _check(dec, A, pi, E, lens, (S, kind))


@pytest.mark.parametrize("S", [300, 361, 383])
@pytest.mark.parametrize("n_extras", [0, 1, 2, 3])
def test_extra_column_counts(dev, S, n_extras):
    """0-3 extra columns anywhere (the generic instantiation; one extra column takes the compile-time one)."""
    rng = np.random.default_rng(100 * S + n_extras)
    A, pi, extras = _matrix(S, rng, n_extras=n_extras if n_extras != 1 else 0)
    if n_extras == 1:                       # one extra column that is not the last state
        x = int(rng.integers(0, S - 1))
        A[:, x] = -(rng.integers(0, 40, S) / 2)
        extras = [x]
    dec = ViterbiDecoder(A, pi, dev)
    assert len(dec.info["extras"]) == n_extras, (dec.info["extras"], extras)
    E = torch.from_numpy(-(rng.integers(0, 6, (len(SHORT), 40, S)) / 2).astype(np.float32)).to(dev)
    lens = torch.tensor(SHORT[:-1] + [40], dtype=torch.int64, device=dev)
    _check(dec, A, pi, E, lens, (S, extras))


@pytest.mark.parametrize("where", ["extra", 255, 256, 300, "last"])
def test_frame_maximum_planted(dev, where):
    """The frame maximum sits, on most frames, on the extra column (excluded from M) / on the last full-wave target / on
    the first half-wave target / inside a half wave / on the last voiced state; in between it moves away, so that the
    row-constant term fl(M + c_j) wins for far targets."""
    S = 361
    A, pi = synth.log_params(synth.tonet_transition(S - 1, 14), synth.floored_prior(S))
    dec = ViterbiDecoder(A, pi, dev)
    col = {"extra": dec.info["extras"][0], "last": S - 2}.get(where, where)
    B, T = 6, 200
    rng = np.random.default_rng(11)
    E = synth.emissions_peaks(B, T, S, seed=9).cpu().numpy().copy()
    on = rng.random((B, T)) < 0.8
    E[:, :, col] = np.where(on, E.max(axis=2) + rng.integers(1, 40, (B, T)).astype(np.float32) / 4, E[:, :, col])
    E = torch.from_numpy(E.astype(np.float32)).to(dev)
    lens = torch.tensor([T, T - 1, 13, 25, 2, 1], dtype=torch.int64, device=dev)
    _check(dec, A, pi, E, lens, ("planted", where))


@pytest.mark.parametrize("S", [321, 361, 383])
def test_ties_across_the_split_boundary(dev, S):
    """Every in-window weight 0 and every emission 0 (then a few -1): all the candidates of a target tie, across sources 15
    and 16 of its window too, and the back-trace must still pick the lowest index."""
    rng = np.random.default_rng(S)
    A = np.full((S, S), -50.0, np.float32)
    for j in range(S):
        A[j, max(0, j - 14):min(S, j + 15)] = 0.0
    A[:, S - 1] = 0.0
    pi = np.zeros(S, np.float32)
    dec = ViterbiDecoder(A, pi, dev)
    B, T = 4, 60
    Ez = np.zeros((B, T, S), np.float32)
    Ez[1:, ::5] = -(rng.integers(0, 2, (B - 1, len(range(0, T, 5)), S))).astype(np.float32)
    E = torch.from_numpy(Ez).to(dev)
    lens = torch.tensor([T, 25, 13, 7], dtype=torch.int64, device=dev)
    _check(dec, A, pi, E, lens, ("all ties", S))
    st, _ = dec.decode(E[:1], algo="group", out_dtype=torch.int32)
    assert int(st.max()) == 0, "all candidates tie: the path is state 0 throughout"


@pytest.mark.parametrize("S", [321, 361])
def test_signed_zeros(dev, S):
    rng = np.random.default_rng(3)
    A = _banded_matrix(S, 10, rng, extras=(S - 1,), floor=-50.0, quant=2)
    zero = A == 0
    A[zero] = np.where(rng.random(int(zero.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    pi = np.where(rng.random(S) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    dec = ViterbiDecoder(A, pi, dev)
    B, T = 5, 60
    Ez = np.where(rng.random((B, T, S)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    Ez[:, ::7] = -(rng.integers(0, 3, (B, len(range(0, T, 7)), S)) / 2).astype(np.float32)
    E = torch.from_numpy(Ez).to(dev)
    lens = torch.tensor([T, 13, 25, 1, 12], dtype=torch.int64, device=dev)
    # +0 and -0 are the same maximum: paths bit for bit, log-likelihood by value, history through the decodes
    _check(dec, A, pi, E, lens, ("signed zeros", S), loglik_bits=False, history=False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_minus_inf_emissions(dev, dtype):
    """A third of the emissions are -inf (never a whole frame): -inf sums on both halves of a window."""
    S = 361
    rng = np.random.default_rng(17)
    A, pi, _ = _matrix(S, rng)
    dec = ViterbiDecoder(A, pi, dev)
    B, T = 6, 80
    Ez = -(rng.integers(0, 6, (B, T, S)) / 2).astype(np.float32)
    Ez[rng.random((B, T, S)) < 0.33] = -np.inf
    Ez[:, :, 100] = -1.0
    Ez[:, :, 300] = -1.5
    E = torch.from_numpy(Ez).to(dev).to(dtype)
    lens = torch.tensor([T, 25, 13, 12, 2, 1], dtype=torch.int64, device=dev)
    _check(dec, A, pi, E, lens, "-inf emissions")


@pytest.mark.parametrize("B", [1, 128, 256, 257])
def test_batch_sizes_and_default_selection(dev, B):
    """B = 1, 128, 256: the default (forward_form 0) is byte-identical to the forced forms; B = 257: the default still
    decodes what the two-targets-per-lane kernel (forward_form 2) decodes -- the launcher rule itself (split kernel only up
    to one song per CU) is a line of launch_floor_t."""
    S, T = 361, 64
    A, pi = synth.log_params(synth.tonet_transition(S - 1, 14), synth.floored_prior(S))
    dec = ViterbiDecoder(A, pi, dev)
    E = synth.emissions_peaks(B, T, S, seed=B, device=dev)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    lens[::3] = torch.arange(len(lens[::3]), device=dev) % T + 1
    ref_s, ref_l = vo.decode_c(A, pi, E.cpu().numpy(), lengths=lens.cpu().numpy())
    for form in (0, 6, 1, 2):
        dec.set_option("forward_form", form)
        st, ll = dec.decode(E, lengths=lens, algo="group", out_dtype=torch.int32)
        dec.set_option("reset", 0)
        assert np.array_equal(st.cpu().numpy(), ref_s), (B, form)
        assert np.array_equal(_bits(ll.cpu().numpy()), _bits(ref_l)), (B, form)
    assert np.array_equal(_history(dec, E, lens, 0), _history(dec, E, lens, 1)), B
    assert np.array_equal(_history(dec, E, lens, 6), _history(dec, E, lens, 1)), B


def test_default_at_the_headline_shape_equals_the_one_target_kernel(dev):
    """forward_form 0 at B = 128, S = 361 (what the bench runs, shorter): paths, log-likelihoods and history byte-identical
    to forward_form 1."""
    S, B, T = 361, 128, 1500
    A, pi = synth.log_params(synth.tonet_transition(S - 1, 14), synth.floored_prior(S))
    dec = ViterbiDecoder(A, pi, dev)
    base = synth.emissions_peaks(32, T, S, seed=1234, device=dev)
    E = base.repeat(B // 32, 1, 1).contiguous()
    out = {}
    for form in (0, 1):
        dec.set_option("forward_form", form)
        st, ll = dec.decode(E, algo="group", out_dtype=torch.int32)
        dec.set_option("reset", 0)
        out[form] = (st.cpu().numpy(), ll.cpu().numpy())
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(_bits(out[0][1]), _bits(out[1][1]))
    ref_s, ref_l = vo.decode_c(A, pi, E[:32].cpu().numpy())
    assert np.array_equal(out[0][0][:32], ref_s) and np.array_equal(_bits(out[0][1][:32]), _bits(ref_l))
    assert np.array_equal(_history(dec, E, None, 0), _history(dec, E, None, 1))
