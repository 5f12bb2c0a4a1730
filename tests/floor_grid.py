"""The plan grid of the float32 workgroup variants (tests/test_floor_variant_grid_host.py, tests/test_gpu_floor_variant_grid.py) and
the wave-form geometries of tests/test_gpu_parity.py::test_wave_form_geometries (tests/test_gpu_wave_variant_geometries.py).  Plain
NumPy plus synth, no GPU.

banded_floor_forward_kernel is instantiated per window width W (plan.hpp kBandedWidths) and target-wave count NWT (kernels.hpp
banded_waves_for), once per WgVariant.  GRID names one plan per (W, NWT) pair so that every instantiation of the Packed, Ckpt and
PackedCkpt variants, and the back-trace instantiation behind it, decodes something in the suite:

  * 22 pairs by the band recipe of tests/f64_ref.band_params(S, half): band +/- half over S - 1 bins, the unvoiced state last;
  * 3 pairs -- (84, 4), (96, 4), (128, 6) -- by sparse_band_matrix.  A full band reaches none of them: the plan takes a column
    that is an exception in more than a quarter of the rows for an extra column (plan.cpp step 2), a full band +/- half makes every
    column one in 2 half + 1 rows, and these pairs need 2 half + 1 > S / 4 (band_params and tests/test_plan_host._banded_matrix at
    (200, 40), (255, 46), (383, 56): ok == False).  A band that holds every other diagonal only spans the same window with half
    the exceptions per column;
  * UNREACHED, 5 pairs no plan reaches: (64, 2), (84, 2), (96, 2), (128, 2), (128, 4).  The plan picks a width only where
    2 W <= S (plan.cpp step 4), and banded_waves_for(S) == NWT bounds S by 64 NWT.  These instantiations cannot be launched.

REFUSAL_EDGES: banded, floor-proven plans with S == 64 NWT.  The variants keep the frame maximum in idle slot S of the last target
wave, which does not exist there: the three variant entry points refuse them, decode serves them."""
import numpy as np
import torch

from tests.common import single_survivor, window_positions
from tests.f64_ref import band_params
from viterbi_spl_amd import synth

WIDTHS = (16, 32, 64, 84, 96, 128)          # plan.hpp kBandedWidths
WAVES = (2, 4, 6, 8, 12)                    # kernels.hpp banded_waves_for


def waves_for(S):                           # kernels.hpp banded_waves_for
    return next((w for w in WAVES if w >= (S + 63) // 64), 0)


def floor_form_instantiated(W, nwt):        # kernels.hpp
    return nwt > 0 and W <= 128 and nwt <= 12


def floor_packed_applies(S, W, floor_ok, n_dense):      # kernels.hpp
    nwt = waves_for(S)
    return bool(floor_ok) and n_dense == 0 and nwt > 0 and S < nwt * 64 and W in WIDTHS and floor_form_instantiated(W, nwt)


def floor_ckpt_pair(W, nwt):                # kernels.hpp; floor_pckpt_applies asks the same
    return W >= 64 or nwt >= 8


def sparse_backtrace_applies_group(S, W):
    """backtrace_sparse.hip sparse_backtrace_applies over the workgroup rows of a banded plan without dense rows (capi.hip
    ck_sparse_applies, kFamGroup: row stride (S + 5) / 4 * 4, the frame maximum in column S)."""
    kc = (W + 4 + 1 + 63) // 64             # candidates per lane: window + kMaxExtras + the row constant
    span = {1: 64, 2: 128}.get(kc, 160)
    sd = (S + 5) // 4 * 4
    return kc <= 3 and W + 32 <= span and sd >= span and sd % 4 == 0 and (S + 63) // 64 <= 12


# (W, NWT) -> (S, half) of band_params
BAND_GRID = {
    (16, 2): (100, 6), (16, 4): (200, 6), (16, 6): (383, 6), (16, 8): (450, 6), (16, 12): (722, 6),
    (32, 2): (127, 14), (32, 4): (200, 14), (32, 6): (383, 14), (32, 8): (450, 14), (32, 12): (722, 14),
    (64, 4): (255, 30), (64, 6): (321, 30), (64, 8): (450, 30), (64, 12): (722, 30),
    (84, 6): (361, 40), (84, 8): (450, 40), (84, 12): (722, 40),
    (96, 6): (383, 46), (96, 8): (450, 46), (96, 12): (722, 46),
    (128, 8): (511, 56), (128, 12): (722, 56),
}
# (W, NWT) -> (S, half) of sparse_band_matrix
SPARSE_GRID = {(84, 4): (200, 40), (96, 4): (255, 46), (128, 6): (383, 56)}
UNREACHED = ((64, 2), (84, 2), (96, 2), (128, 2), (128, 4))
REFUSAL_EDGES = ((128, 14), (256, 30), (384, 46), (512, 56), (768, 6))          # (S, half) of band_params

# every grid plan as (W, NWT, S, half, recipe), narrow windows and few waves first
GRID = tuple(sorted([(W, n, S, h, "band") for (W, n), (S, h) in BAND_GRID.items()] +
                    [(W, n, S, h, "sparse") for (W, n), (S, h) in SPARSE_GRID.items()]))


def plan_id(entry):
    W, n, S, half, recipe = entry
    return f"W{W}-N{n}-S{S}" + ("-sparse" if recipe == "sparse" else "")


def sparse_band_matrix(S, half, rng, floor=-50.0, quant=2):
    """tests/test_plan_host._banded_matrix with every other diagonal of the band left at the floor: A[j][i] is drawn where
    |i - j| <= half and i - j is even (half even: the span of a row is still 2 half + 1 wide), no extra column."""
    assert half % 2 == 0
    A = np.full((S, S), floor, np.float32)
    i = np.arange(S)
    for j in range(S):
        on = (np.abs(i - j) <= half) & ((i - j) % 2 == 0)
        A[j, on] = -(rng.integers(0, 40, int(on.sum())) / quant)
    return A


def plan_params(entry):
    """(logA_T, log_pi) float32 of a GRID entry."""
    W, n, S, half, recipe = entry
    if recipe == "band":
        return band_params(S, half)
    rng = np.random.default_rng(1000 * W + S)
    A = sparse_band_matrix(S, half, rng)
    pi = -(rng.integers(0, 8, S) / 2).astype(np.float32)
    return A, pi


# One frame, both sides of the twelve-frame unroll, both sides of one and two segments of 64 frames, a full-length song
T = 200
LENGTHS = np.asarray([200, 1, 2, 3, 13, 14, 63, 64, 65, 129, 199], np.int64)


def pack_order(lens):
    """The order the songs are packed in: fixed and shuffled, not sorted by length either way."""
    order = np.random.default_rng(5).permutation(len(lens))
    d = np.diff(np.asarray(lens)[order])
    assert (d > 0).any() and (d < 0).any()
    return order


def offsets_of(lens):
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return off


def forced_song(A, W, half, lo, unvoiced, n_frames=T):
    """One song with a single finite emission per frame (tests/common.py single_survivor: the path is the survivor's walk, whatever the
    matrix says) whose steps are every offset of the band, then half - (W - 1) and back: a step by +half enters its target through
    the FIRST window entry, the step by half - (W - 1) through the LAST (lo[j] = j - half away from the borders).  unvoiced: that
    state survives frames 150 and 151 (entered from a voiced state, held, and left again); None: the plan has no extra column.
    The start of the walk is drawn until both window edges occur.  -> (E [n_frames, S] float32 on the fp16 grid, walk [n_frames])"""
    S = A.shape[0]
    D = half - (W - 1)
    offsets = [0] + [s * k for k in range(1, half + 1) for s in (1, -1)] + [D, -D]
    assert len(offsets) + 1 < 150 <= n_frames - 2
    for seed in range(64):
        rng = np.random.default_rng(7000 + seed)
        E, walk = single_survivor(rng, np.asarray(A), 1, n_frames, offsets)
        E, walk = E[0], walk[0]
        if unvoiced is not None:
            for t in (150, 151):
                E[t, :] = -np.inf
                E[t, unvoiced] = -(int(rng.integers(0, 8)) / 2)
                walk[t] = unvoiced
        pos = window_positions(walk[None], [n_frames], lo)
        if (pos == 0).any() and (pos == W - 1).any():
            return E, walk
    raise AssertionError("no walk reaches both window edges")


def premise_forced(path, W, lo, unvoiced):
    """On a decoded path alone: a step through the first window entry, one through the last, and the unvoiced state entered and left."""
    path = np.asarray(path, np.int64)
    pos = window_positions(path[None], [len(path)], lo)
    assert (pos == 0).any(), "no step through the first window entry"
    assert (pos == W - 1).any(), "no step through the last window entry"
    if unvoiced is not None:
        at = np.nonzero(path == unvoiced)[0]
        assert len(at) and at[0] > 0 and at[-1] < len(path) - 1, "the unvoiced column is not entered and left"
        assert path[at[0] - 1] != unvoiced and path[at[-1] + 1] != unvoiced


def emissions_hops(B, n_frames, S, seed, peaks=4):
    """Emissions that make the best path leave the window: -200 everywhere but `peaks` states per frame, drawn uniformly over all
    states, with values 0 .. -12 on the half-integer grid (exact in float16).  Staying near the path costs 200 a frame, a hop to
    the next peak the row constant (log(tiny) = -87.3 for the band recipe, -50 for the sparse bands): most steps are decided by the
    candidate fl(M + c_j), M the frame maximum -- the forward kernel's slot S, the column the back-trace reads its bound from, and
    what a resumed segment re-forms from its checkpoint row.  The i.i.d. kinds of synth keep their paths inside the band."""
    rng = np.random.default_rng(seed)
    E = np.full((B, n_frames, S), -200.0, np.float32)
    for b in range(B):
        for t in range(n_frames):
            E[b, t, rng.integers(0, S, peaks)] = -(rng.integers(0, 25, peaks) / 2)
        for t in range(64, n_frames, 64):       # frames t - 1 and t hold one peak each, S // 2 >= W states apart: the step into t is a hop
            p = int(rng.integers(0, S // 2 - 1))
            E[b, t - 1:t + 1] = -200.0
            E[b, t - 1, p], E[b, t, p + S // 2] = -(rng.integers(0, 25, 2) / 2)
    return E


def outside_steps(ref_s, lens, W, lo, extras):
    """(steps of the paths whose source lies outside the target's window and is no extra column, all steps)."""
    out = total = 0
    lo = np.asarray(lo, np.int64)
    for b in range(ref_s.shape[0]):
        p = np.asarray(ref_s[b, :int(lens[b])], np.int64)
        src, tgt = p[:-1], p[1:]
        far = ((src < lo[tgt]) | (src >= lo[tgt] + W)) & ~np.isin(src, np.asarray(extras, np.int64))
        out, total = out + int(far.sum()), total + len(src)
    return out, total


def premise_hops(ref_s, lens, W, lo, extras):
    """On the oracle's paths alone: at least an eighth of all steps come from outside the window (the grid plans have a sixth, where
    the window spans a third of the states and more, to three quarters of them), and in every song that reaches them the steps into
    frames 64, 128 and 192 (the first frames of resumed segments of 64)."""
    out, total = outside_steps(ref_s, lens, W, lo, extras)
    assert 8 * out >= total > 0, (out, total)
    for b in range(ref_s.shape[0]):
        for t in range(64, int(lens[b]), 64):
            assert outside_steps(ref_s[b:b + 1, t - 1:t + 1], [2], W, lo, extras) == (1, 1), ("no hop into frame", t, "of song", b)


# (W, NWT) -> added to the seed of the plan's hops batch.  tests/test_gpu_stream_grid.py wants a wrong entry guess in song 0 when its
# back-trace runs as seven chunks without a warm-up (premise_wrong_guess); with the plain seed this plan has none.
HOPS_RESEED = {(64, 6): 2000}


def premise_wrong_guess(A, pi, E, ref_path, chunks=7):
    """On the oracle alone: a back-trace of this song in `chunks` chunks without a warm-up starts at least one interior chunk from a
    wrong state.  Chunk c assumes the lowest-index arg-max of delta row hi_c = Lf (c + 1) / chunks, Lf = frames - 1, as its entry
    state (backtrace_common.hpp bt_run_chunks), so a verify-and-repair pass that did nothing would leave a wrong path.  -> the number
    of wrong guesses."""
    from oracle import viterbi_oracle as vo
    n = len(ref_path)
    hi = np.asarray([(n - 1) * (c + 1) // chunks for c in range(chunks - 1)], np.int64)
    rep = np.ascontiguousarray(np.broadcast_to(np.asarray(E)[None, :n], (chunks - 1, n) + np.shape(E)[1:]))
    _, _, rows = vo.decode_c(A, pi, rep, lengths=hi + 1, return_delta=True)
    wrong = int(np.sum(np.argmax(rows, axis=1) != np.asarray(ref_path)[hi]))
    assert wrong > 0, "premise: every entry guess of the chunked back-trace is right -- pick another seed (HOPS_RESEED)"
    return wrong


def plan_batches(entry, A, lo, extras):
    """The inputs of one grid plan, float32 on the fp16 grid (one oracle run serves both storage types):
    [("peaks", E [11, T, S], LENGTHS), ("ties", E [12, T, S], LENGTHS + the forced song of T frames), ("hops", E [11, T, S], LENGTHS)]."""
    W, n, S, half, recipe = entry
    seed = 100 * S + W
    peaks = synth.emissions_peaks(len(LENGTHS), T, S, seed=seed).to(torch.float16).to(torch.float32).numpy().copy()
    ties = synth.emissions_ties(len(LENGTHS), T, S, seed=seed + 1).to(torch.float16).to(torch.float32).numpy()
    unvoiced = extras[0] if extras else None
    forced, _ = forced_song(A, W, half, lo, unvoiced)
    ties = np.concatenate([ties, forced[None]], axis=0)
    hops = emissions_hops(len(LENGTHS), T, S, seed + 2 + HOPS_RESEED.get((W, n), 0))
    for E in (ties, hops):
        assert np.array_equal(E.astype(np.float16).astype(np.float32), E)
    return [("peaks", peaks, LENGTHS.copy()), ("ties", ties, np.append(LENGTHS, T)), ("hops", hops, LENGTHS.copy())]


# ---------------------------------------------------------------------------------------------------------------------
# Wave-form geometries: the matrices of tests/test_gpu_parity.py::test_wave_form_geometries
# ---------------------------------------------------------------------------------------------------------------------
WAVE_GEOMETRY_SEEDS = tuple(range(10))
# the seeds whose plan has the wave form (S + extra columns < 384); tests/test_floor_variant_grid_host.py holds this against the plan
WAVE_FORM_SEEDS = (0, 2, 3, 4, 5, 6, 7, 8, 9)     # (seed 1: S = 383 with one extra column)


def wave_geometry(seed):
    """State count, half-width, extra columns, matrix and prior of geometry `seed` (0 .. 9), and the generator they were drawn from,
    left where the draws ended -> (S, half, extras, A, pi, rng)."""
    from tests.test_plan_host import _banded_matrix
    rng = np.random.default_rng(900 + seed)
    S = [321, 383, 361, 322, 382][seed % 5] if seed < 5 else int(rng.integers(321, 384))
    half = [14, 1, 7, 14, 13][seed % 5] if seed < 5 else int(rng.integers(1, 15))
    extras = sorted(set(int(x) for x in rng.integers(0, S, seed % 3)))
    A = _banded_matrix(S, half, rng, extras, (), floor=-50.0, quant=2)
    pi = -(rng.integers(0, 8, S) / 2).astype(np.float32)
    return S, half, extras, A, pi, rng


# ---------------------------------------------------------------------------------------------------------------------
# Structure cases: the matrices of tests/test_gpu_parity.py::test_every_kernel_path_is_exercised,
# ::test_random_banded_structures_on_gpu and ::test_generic_backtrace_with_windows_wider_than_a_wave, shared with the
# off-grid twins of tests/inexact_cases.py
# ---------------------------------------------------------------------------------------------------------------------
def kernel_path_matrices(rng):
    """One matrix per forward / back-trace combination, named "<forward>+<back-trace>", drawn from `rng` in this order."""
    from tests.test_plan_host import _banded_matrix

    def varying_band(S):                       # lower half-width depends on the row: window start not affine in j
        A = np.full((S, S), -60.0, np.float32)
        for j in range(S):
            lo, hi = max(0, j - 1 - j % 5), min(S, j + 4)
            A[j, lo:hi] = -(rng.integers(0, 40, hi - lo) / 2)
        return A

    return {
        "floor+lean_affine": _banded_matrix(150, 5, rng, extras=(149,), floor=-50.0, quant=2),
        "floor+lean_table": varying_band(170),
        "scan+lean": _banded_matrix(150, 5, rng, extras=(40,), floor=-3.0, quant=2),        # window entries below the floor
        "scan+generic": _banded_matrix(150, 5, rng, extras=(149,), dense_rows=(7, 100), floor=-50.0, quant=2),
        "scan(full waves)+lean": _banded_matrix(128, 4, rng, floor=-50.0, quant=2),          # S == 64 * waves
    }


def selected_kernels(info):
    """("floor" | "scan", "lean_affine" | "lean_table" | "generic") the launchers pick for a banded plan with this ViterbiDecoder.info."""
    S = info["S"]
    nwt = next(w for w in (2, 4, 6, 8, 12) if w * 64 >= S)
    fwd = "floor" if info["floor_ok"] and info["n_dense_rows"] == 0 and S < nwt * 64 else "scan"
    bt = ("lean_affine" if info["lo_affine"] else "lean_table") if info["n_dense_rows"] == 0 else "generic"
    return fwd, bt


RANDOM_BANDED_SEEDS = tuple(range(8))


def random_banded_structure(seed):
    """Structure `seed` (0 .. 7): 70 .. 399 states, half-widths 1 .. 14, 0 - 2 extra columns and dense rows anywhere, floor -50 / -3 /
    -inf by seed -> (S, half, extras, dense_rows, A, pi, rng), the generator left where the draws ended."""
    from tests.test_plan_host import _banded_matrix
    rng = np.random.default_rng(100 + seed)
    S = int(rng.integers(70, 400))
    half = int(rng.integers(1, 15))
    extras = sorted(set(int(x) for x in rng.integers(0, S, int(rng.integers(0, 3)))))
    dense_rows = sorted(set(int(x) for x in rng.integers(0, S, int(rng.integers(0, 3)))))
    floor = [-50.0, -3.0, -np.inf][seed % 3]
    A = _banded_matrix(S, half, rng, extras, dense_rows, floor=floor, quant=2)
    pi = -(rng.integers(0, 8, S) / 2).astype(np.float32)
    return S, half, extras, dense_rows, A, pi, rng


WIDE_ROWS = (50, 70, 90, 110, 130, 150)


def few_wide_rows(S, rng, wide_rows, half_wide=40, half=5):
    """Narrow band everywhere, a handful of rows with a wide one: more than kMaxDenseRows of them, so the plan widens the
    evaluated window (W = 96) instead of declaring them dense rows -- while S stays small enough for the generic
    back-trace to keep its tables in LDS."""
    A = np.full((S, S), -50.0, np.float32)
    for j in range(S):
        h = half_wide if j in wide_rows else half
        lo, hi = max(0, j - h), min(S, j + h + 1)
        A[j, lo:hi] = -(rng.integers(0, 40, hi - lo) / 2)
    A[:, S - 1] = -(rng.integers(0, 40, S) / 2)
    return A


def wide_row_emissions(rng, B, T, S, wide=WIDE_ROWS):
    """Emissions on the half-integer grid that force the paths through the wide rows: odd frames strongly favour a wide row j, the
    frame before a state 24 .. 40 above it, so the path enters j through a window source beyond the first 64 (window = j - 40 ..
    j + 40)."""
    E = -(rng.integers(0, 12, (B, T, S)) / 2).astype(np.float32)
    for t in range(1, T, 2):
        j = wide[(t // 2) % len(wide)]
        E[:, t, j] = 6.0
        E[:, t - 1, j + 24 + (t // 2) % 17] = 6.0
    return E
