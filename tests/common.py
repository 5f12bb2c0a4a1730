"""Shared helpers for the tests (input regeneration from the golden manifest)."""
import hashlib

import numpy as np
import torch

from viterbi_spl_amd import synth

GEN = {"peaks": synth.emissions_peaks, "dense": synth.emissions_dense, "ties": synth.emissions_ties,
       "scaled": synth.emissions_scaled}


def case_params(golden, case):
    p = golden["params"]
    return p[f"{case['params']}_logA_T"], p[f"{case['params']}_log_pi"]


def case_emissions(case, device="cpu", as_stored=False):
    """[T,S] emissions of a golden case.  as_stored=True keeps fp16 storage for f16 cases."""
    dt = torch.float16 if case["f16"] else torch.float32
    e = GEN[case["kind"]](1, case["T"], case["S"], seed=case["seed"], dtype=dt, device=device)[0]
    return e if as_stored else e.to(torch.float32)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def logits_case(seed, n_frames, n_bins):
    """Seeded pitch logits for the emission-builder tests: weak noise floor (unvoiced frames), melody-like
    bumps in two frames out of three, and some exactly tied values."""
    rng = np.random.default_rng(seed)
    x = rng.normal(-8.0, 1.5, (n_frames, n_bins)).astype(np.float32)
    for f in range(n_frames):
        if f % 3:
            c = int(rng.integers(8, n_bins - 8))
            x[f, c - 2:c + 3] += np.asarray([1.0, 3.0, 6.0, 3.0, 1.0], np.float32) * np.float32(rng.uniform(0.5, 2.5))
    x[:, ::37] = np.round(x[:, ::37])
    return x


# spans (nats below a frame's top logit) of the range-edge frames: e^-d is a normal float32 up to d ~ 87.3, a subnormal
# from there to ~103.3 (103.0 - 103.6 is left out: there the rounding to the smallest subnormal decides) and 0 beyond
RANGE_SPANS = (80, 86, 88, 90, 95, 100, 102, 106, 120)
RANGE_TOPS = (0, 10, -20, 37)


def range_edge_logits(n_bins, spw, tops=RANGE_TOPS, unvoiced_column=False):
    """Deterministic pitch logits at the float32 range edge of exp: integer values, a constant background 130 below the
    frame's top, and isolated peaks (2*spw + 2 bins apart, so that exactly these bins are peaks) at the top and at
    top - d for every d of RANGE_SPANS, rotated through the slots frame by frame.  The first slot is bin 0 (the left-end
    rule) or bin spw // 2 + 1 (the first bin past those that are never a peak).  -> float32 [n, n_bins].
    unvoiced_column=True: [n, n_bins + 1] with column 0 the unvoiced logit, 5 below the top, and one more frame per top and
    span in which the unvoiced logit is the far one (top - d)."""
    seq = (0,) + RANGE_SPANS
    rows, unv = [], []
    for top in tops:
        for start in (0, spw // 2 + 1):
            for r in range(len(seq)):
                x = np.full(n_bins, top - 130, np.float32)
                for j, b in enumerate(range(start, n_bins, 2 * spw + 2)):
                    x[b] = top - seq[(j + r) % len(seq)]
                rows.append(x)
                unv.append(top - 5)
        if unvoiced_column:
            for d in RANGE_SPANS:
                x = np.full(n_bins, top - 130, np.float32)
                x[spw + 1::2 * spw + 2] = top - 3
                x[spw + 1] = top
                rows.append(x)
                unv.append(top - d)
    x = np.stack(rows)
    if unvoiced_column:
        x = np.concatenate([np.asarray(unv, np.float32)[:, None], x], axis=1)
    return np.ascontiguousarray(x, np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# Value-edge inputs (tests/test_value_edges_host.py, tests/test_gpu_value_edges.py): -inf entries, songs that die, float32
# overflow / absorption, signed zeros and the float16 edge values.  Plain NumPy, seeded, no GPU.  Every builder returns float32
# emissions [B, T, S] plus what its premise check needs; the premise_* functions assert, on the ORACLE's output alone, that a
# construction hit what it aims at -- a builder that misses fails as a test error, never as a silent pass.
# ---------------------------------------------------------------------------------------------------------------------
NINF_BITS = 0xFF800000


def f32_bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _grid(rng, B, T, S):
    return -(rng.integers(0, 12, (B, T, S)) / 2).astype(np.float32)


def kept_columns(S):
    """Two adjacent states in the middle of the voiced range: each reaches the other through any band of half-width >= 1."""
    return (S // 3, S // 3 + 1)


def sparse_inf(rng, B, T, S, keep=None):
    """About a third of the entries -inf, two columns kept finite."""
    E = _grid(rng, B, T, S)
    E[rng.random((B, T, S)) < 1 / 3] = -np.inf
    for c in (keep or kept_columns(S)):
        E[:, :, c] = -(rng.integers(0, 4, (B, T)) / 2)
    return E


def premise_all_finite(ref_l):
    assert np.all(np.isfinite(ref_l)), ref_l


def dead_frame(rng, B, T, S, deaths, keep=None):
    """deaths = {song: t_d}: every state's emission of that song is -inf at frame t_d (the other frames: sparse_inf)."""
    E = sparse_inf(rng, B, T, S, keep)
    for b, t_d in deaths.items():
        E[b, t_d, :] = -np.inf
    return E


def premise_dead(ref_s, ref_l, lens, deaths):
    """Songs that reach their frame t_d: log-likelihood -inf (by bits) and state 0 from t_d on; every other song finite."""
    B = ref_s.shape[0]
    hit = 0
    for b in range(B):
        n = int(lens[b])
        t_d = deaths.get(b)
        if t_d is not None and t_d < n:
            assert f32_bits(ref_l)[b] == NINF_BITS, (b, ref_l[b])
            assert np.all(ref_s[b, t_d:n] == 0), (b, t_d, ref_s[b, t_d:n])
            hit += 1
        else:
            assert np.isfinite(ref_l[b]), (b, ref_l[b])
    assert hit >= 1 and hit < B, "a batch holds dead and live songs"


def starved(rng, A, B, T, deaths):
    """A = a band matrix with floor -inf and no extra column.  At frame t_d - 1 only three adjacent states have finite
    emissions; at frame t_d the emissions are finite only on targets none of those three reaches: the song dies through the
    matrix, no emission row is all -inf.  Premise: premise_dead."""
    S = A.shape[0]
    E = _grid(rng, B, T, S)
    for b, t_d in deaths.items():
        assert t_d >= 1
        c = int(rng.integers(S // 4, S // 2))
        live = np.arange(c, c + 3)
        E[b, t_d - 1, :] = -np.inf
        E[b, t_d - 1, live] = -(rng.integers(0, 4, 3) / 2)
        reached = np.isfinite(A[:, live]).any(axis=1)
        assert reached.any() and not reached.all(), "the matrix must have a -inf floor"
        E[b, t_d, reached] = -np.inf
        assert np.isfinite(E[b, t_d]).any()
    return E


def single_survivor(rng, A, B, T, offsets):
    """Per frame exactly one finite emission; the survivor of song b walks by offsets[(t - 1 + 21 b) % len] where the matrix allows the
    step (A[j][i] finite, j inside the states) and by the negated or a zero step at the borders.  -> (E, walk [B, T])."""
    S = A.shape[0]
    E = np.full((B, T, S), -np.inf, np.float32)
    walk = np.empty((B, T), np.int64)
    for b in range(B):
        i = int(rng.integers(S // 3, S // 2))
        for t in range(T):
            if t:
                d = int(offsets[(t - 1 + 21 * b) % len(offsets)])
                for step in (d, -d, 0):
                    j = i + step
                    if 0 <= j < S and np.isfinite(A[j, i]):
                        break
                else:
                    raise AssertionError("no finite step out of state %d" % i)
                i = j
            walk[b, t] = i
            E[b, t, i] = -(int(rng.integers(0, 8)) / 2)
    return E, walk


def premise_survivor(ref_s, ref_l, lens, walk, offsets):
    premise_all_finite(ref_l)
    seen = set()
    for b in range(ref_s.shape[0]):
        n = int(lens[b])
        assert np.array_equal(ref_s[b, :n], walk[b, :n]), b
        seen |= set(np.diff(walk[b, :n]).tolist())
    assert set(int(d) for d in offsets) <= seen, sorted(set(int(d) for d in offsets) - seen)


def window_positions(ref_s, lens, lo):
    """Position inside the evaluated window (source - lo[target]) of every step of the oracle's paths."""
    out = []
    for b in range(ref_s.shape[0]):
        n = int(lens[b])
        out.append(ref_s[b, :n - 1] - np.asarray(lo)[ref_s[b, 1:n]])
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def dead_prior(rng, S, all_dead=False):
    pi = np.full(S, -np.inf, np.float32)
    if not all_dead:
        c = S // 3
        pi[[c, c + 1, (2 * S) // 3]] = -(rng.integers(0, 8, 3) / 2)
    return pi


def premise_all_dead(ref_s, ref_l, lens):
    assert np.all(f32_bits(ref_l) == NINF_BITS), ref_l
    for b in range(ref_s.shape[0]):
        assert np.all(ref_s[b, :int(lens[b])] == 0), b


def overflow_dead(rng, B, T, S, deaths):
    """float32 only: every emission of frames t_d, t_d + 1 is -3e38 -- delta overflows to -inf, no input is -inf."""
    E = _grid(rng, B, T, S)
    for b, t_d in deaths.items():
        E[b, t_d:t_d + 2, :] = np.float32(-3e38)
    assert np.all(np.isfinite(E))
    return E


def premise_overflow(ref_l, lens, deaths):
    for b in range(len(ref_l)):
        t_d = deaths.get(b)
        if t_d is not None and t_d + 1 < int(lens[b]):
            assert f32_bits(ref_l)[b] == NINF_BITS, (b, ref_l[b])
        elif t_d is None:
            assert np.isfinite(ref_l[b]), (b, ref_l[b])


def absorbing(rng, B, T, S):
    """float32 only: emissions around -1e30, off any grid -- every matrix entry is absorbed by the sum."""
    return (np.float32(-1e30) * (1 + rng.random((B, T, S)))).astype(np.float32)


def premise_absorbing(ref_l, A):
    lo = np.float32(A[np.isfinite(A)].min())
    assert np.all(np.isfinite(ref_l)) and np.all((np.float32(ref_l) + lo).astype(np.float32) == ref_l), ref_l


def signed_zeros(rng, A, B, T):
    """-> (A2, pi, E): the zero entries of A take a random sign, the prior is +-0 throughout, the emissions are +-0 with every
    seventh frame on a coarse grid (tests/test_gpu_floor_split.py::test_signed_zeros, for any S)."""
    S = A.shape[0]
    A2 = np.array(A, np.float32)
    zero = A2 == 0
    A2[zero] = np.where(rng.random(int(zero.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    pi = np.where(rng.random(S) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    E = np.where(rng.random((B, T, S)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    E[:, ::7] = -(rng.integers(0, 3, (B, len(range(0, T, 7)), S)) / 2).astype(np.float32)
    return A2, pi, E


# +0, -0, +-2^-24 (smallest subnormal), +-largest subnormal, +-2^-14 (smallest normal), -65504, -inf
FP16_EDGE_BITS = (0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x8400, 0xFBFF, 0xFC00)


def fp16_edges(rng, B, T, S, deaths=None, keep=None):
    """Built from uint16 bit patterns: half the entries draw from FP16_EDGE_BITS, the rest are ordinary values (-k/8, k < 96);
    two columns kept ordinary; deaths = {song: t_d} plants whole -inf frames.  -> (float32 [B, T, S], float16 [B, T, S]): the
    float32 tensor is the exact widening of the float16 one (the oracle's input)."""
    ordinary = (-(rng.integers(0, 96, (B, T, S)) / 8)).astype(np.float16).view(np.uint16)
    edge = np.asarray(FP16_EDGE_BITS, np.uint16)[rng.integers(0, len(FP16_EDGE_BITS), (B, T, S))]
    u = np.where(rng.random((B, T, S)) < 0.5, edge, ordinary).astype(np.uint16)
    for c in (keep or kept_columns(S)):
        u[:, :, c] = ordinary[:, :, c]
    for b, t_d in (deaths or {}).items():
        u[b, t_d, :] = 0xFC00
    E16 = np.ascontiguousarray(u).view(np.float16)
    for pat in FP16_EDGE_BITS:
        assert (u == pat).any(), hex(pat)
    assert not np.isnan(E16).any()
    return E16.astype(np.float32), E16


def inf_floor_sibling(logA_T):
    """The matrix with its floor (the lowest value, log(tiny) in the shipped ones: log(0 + tiny)) replaced by -inf = log(0)."""
    A = np.array(logA_T, np.float32)
    A[A == A.min()] = -np.inf
    return A


def dense_with_inf(rng, S, dead_row=None, dead_col=None, share=0.3):
    """Unstructured matrix on a quarter grid with random -inf entries, one all -inf row (a target nothing reaches) and one all
    -inf column (a source that leads nowhere)."""
    A = (-rng.integers(0, 32, (S, S)) / 4).astype(np.float32)
    A[rng.random((S, S)) < share] = -np.inf
    A[np.arange(S), np.arange(S)] = -(rng.integers(0, 8, S) / 4)          # staying is always possible
    A[S // 5 if dead_row is None else dead_row, :] = -np.inf
    A[:, (2 * S) // 3 if dead_col is None else dead_col] = -np.inf
    return A


def alternating(half):
    """0, +1, -1, +2, -2, ... +half, -half: every step of a band once, with partial sums inside 0 .. half."""
    return [0] + [s * k for k in range(1, half + 1) for s in (1, -1)]


EDGE_B = 12


def _dead_batches(T):
    """Two batches of EDGE_B songs: {song: t_d} and lengths.  Deaths at 0, 1, T-1, around 16 and around 64 (a wave's lanes, the
    segment length of the checkpointed runs), an even and an odd mid-song frame, on a song's last frame and in a song of one frame;
    live songs of 1, 2, T - 1 and T frames in between."""
    out = []
    for td in ((0, 1, 15, 16, 17, T - 1), (63, 64, 65, 40, 41, T - 2)):
        deaths = {b: t for b, t in enumerate(td)}
        lens = [T] * 6
        deaths[6], deaths[11] = td[3], 0
        lens += [td[3] + 1, 1, 2, T, T - 1, 1]                  # song 6 dies on its last frame, song 11 has one frame, a dead one
        out.append((deaths, np.asarray(lens, np.int64)))
    return out


RAGGED = np.asarray([0, 1, 2, 0, -1, 3, 64, 65, 66, 17, 0, 33], np.int64)       # 0 / -1: T, T - 1


def ragged_lengths(T):
    return np.where(RAGGED <= 0, T + RAGGED, np.minimum(RAGGED, T)).astype(np.int64)


def edge_cases(seed, A, pi, T, half=None, f16=False, only=None):
    """Every input class that applies to (A, pi), as (name, A, pi, E32, E16 or None, lens, premise, by_value): premise(ref_s,
    ref_l) asserts the construction on the oracle's output; by_value = compare log-likelihoods by value (signed zeros).
    half: the band's half-width (enables single_survivor); classes that need a -inf floor run where A has one; f16 drops the
    float32-only classes and stores every tensor on the float16 grid."""
    rng = np.random.default_rng(seed)
    S, B = A.shape[0], EDGE_B
    lens = ragged_lengths(T)
    inf_floor = bool(np.isneginf(A).any())

    def store(E):                                   # float16 storage: the oracle sees the rounded values
        if not f16:
            return E, None
        E16 = E.astype(np.float16)
        return E16.astype(np.float32), E16

    def want(name):
        return only is None or name in only

    if want("sparse_inf"):
        E, E16 = store(sparse_inf(rng, B, T, S))
        yield ("sparse_inf", A, pi, E, E16, lens, lambda s, l: premise_all_finite(l), False)
    if want("dead_frame"):
        for k, (deaths, dl) in enumerate(_dead_batches(T)):
            E, E16 = store(dead_frame(rng, B, T, S, deaths))
            yield (f"dead_frame{k}", A, pi, E, E16, dl, lambda s, l, d=deaths, n=dl: premise_dead(s, l, n, d), False)
    if want("starved") and inf_floor:
        deaths, dl = _dead_batches(T)[1]
        deaths = {b: max(t, 1) for b, t in deaths.items() if b != 11}
        E, E16 = store(starved(rng, A, B, T, deaths))
        yield ("starved", A, pi, E, E16, dl, lambda s, l, d=deaths, n=dl: premise_dead(s, l, n, d), False)
    if want("single_survivor") and inf_floor and half:
        off = alternating(half)
        E, walk = single_survivor(rng, A, B, T, off)
        E, E16 = store(E)
        pi_open = np.where(np.isfinite(pi), pi, np.float32(-4.0)).astype(np.float32)
        yield ("single_survivor", A, pi_open, E, E16, lens, lambda s, l, w=walk, n=lens, o=off: premise_survivor(s, l, n, w, o), False)
    if want("dead_prior"):
        E, E16 = store(_grid(rng, B, T, S))
        yield ("dead_prior", A, dead_prior(rng, S), E, E16, lens, lambda s, l: premise_all_finite(l), False)
        yield ("dead_prior_all", A, dead_prior(rng, S, all_dead=True), E, E16, lens, lambda s, l, n=lens: premise_all_dead(s, l, n), False)
    if want("overflow_dead") and not f16:
        deaths, dl = _dead_batches(T)[0]
        E = overflow_dead(rng, B, T, S, deaths)
        yield ("overflow_dead", A, pi, E, None, dl, lambda s, l, d=deaths, n=dl: premise_overflow(l, n, d), False)
    if want("absorbing") and not f16:
        E = absorbing(rng, B, T, S)
        yield ("absorbing", A, pi, E, None, lens, lambda s, l, M=A: premise_absorbing(l, M), False)
    if want("signed_zeros"):
        A2, pi2, E = signed_zeros(rng, A, B, T)
        E, E16 = store(E)
        yield ("signed_zeros", A2, pi2, E, E16, lens, lambda s, l: premise_all_finite(l), True)
    if want("fp16_edges") and f16:
        E, E16 = fp16_edges(rng, B, T, S)
        yield ("fp16_edges", A, pi, E, E16, lens, lambda s, l: premise_all_finite(l), False)
        deaths, dl = _dead_batches(T)[0]
        E, E16 = fp16_edges(rng, B, T, S, deaths=deaths)
        yield ("fp16_edges_dead", A, pi, E, E16, dl, lambda s, l, d=deaths, n=dl: premise_dead(s, l, n, d), False)


# ---------------------------------------------------------------------------------------------------------------------
# Step-structured matrices (tests/test_step_plan_host.py, tests/test_gpu_step_geometries.py): what analyze_step (csrc/plan.cpp)
# accepts beyond the one Durrieu geometry the forward step kernels are instantiated for.
# ---------------------------------------------------------------------------------------------------------------------
def step_matrix(n, bw, kb, rng, zero_top=False, return_table=False):
    """logA_T [n + 1, n + 1] float32 with step structure: n voiced states and the unvoiced state n.  For voiced target j and voiced
    source i  A[j][i] = C[min(|i - j| // bw, kb)][i]: column i is constant in distance bands of bw bins and holds its far value
    C[kb][i] from distance kb * bw on.  Everything lies on the half-integer grid, so that sums tie exactly and the lowest-index rule
    decides: the far values are drawn per column from -15 .. -24.5 (ten or more different values in every row: no row constant, so
    the banded analysis refuses the matrix), each nearer band adds 0, 0.5 or 1 to the next one (a band may equal its neighbour, never
    lie below it) -- except in source column 0, where it adds 0.5 or 1: consecutive bands differ there, which is how the plan measures
    bw and kb.  The unvoiced source column is one value for every voiced target, the unvoiced target's row is arbitrary.
    zero_top=True shifts every column so that its nearest band is exactly +0.  return_table=True: (A, C [kb + 1, n])."""
    far = -(rng.integers(30, 50, n) / 2)
    inc = rng.integers(0, 3, (kb, n)) / 2
    inc[:, 0] = np.maximum(inc[:, 0], 0.5)
    C = np.empty((kb + 1, n), np.float64)
    C[kb] = far
    for k in range(kb - 1, -1, -1):
        C[k] = C[k + 1] + inc[k]
    if zero_top:
        C = C - C[0][None, :]
        C[C == 0] = 0.0                                                      # (+0, never -0)
    C = C.astype(np.float32)
    idx = np.arange(n)
    band = np.minimum(np.abs(idx[None, :] - idx[:, None]) // bw, kb)         # [target j, source i]
    A = np.empty((n + 1, n + 1), np.float32)
    A[:n, :n] = C[band, idx[None, :]]
    A[:n, n] = np.float32(-(int(rng.integers(8, 40)) / 2))
    A[n, :] = -(rng.integers(0, 40, n + 1) / 2)
    return (A, C) if return_table else A


def durrieu_log_params(n, bps):
    """(logA_T, log_pi) of imm's decoder at n voiced states and bps bins per semitone, with the uniform prior."""
    return synth.log_params(synth.durrieu_transition(n, bps), synth.uniform_prior(n + 1))


def emissions_jumps(B, T, S, seed, bw, peaks=6, spread=12):
    """Emissions [B, T, S] float32 that make the best path jump: every frame has `peaks` states with values 0 .. -spread on the
    half-integer grid (exact in float16) and -60 everywhere else, so the path hops from peak to peak, and with `spread` about the
    span of a column's band values the predecessors of a state compete across all distance bands.  Half of the peaks are drawn uniformly over the voiced
    states, half from the bw // 2 states at either end (end-to-end hops land in the far band whenever (kb + 1) * bw < n); one frame
    in eight also offers the unvoiced state.  The i.i.d. kinds of synth ("dense", "ties") keep their paths in the nearest bands."""
    rng = np.random.default_rng(seed)
    n = S - 1
    E = np.full((B, T, S), -60.0, np.float32)
    ends = np.concatenate([np.arange(max(bw // 2, 1)), n - 1 - np.arange(max(bw // 2, 1))])
    for b in range(B):
        for t in range(T):
            pos = np.where(rng.random(peaks) < 0.5, rng.integers(0, n, peaks), ends[rng.integers(0, len(ends), peaks)])
            E[b, t, pos] = -(rng.integers(0, 2 * spread + 1, peaks) / 2)
            if rng.integers(0, 8) == 0:
                E[b, t, n] = -(int(rng.integers(0, 6)) / 2)
    return E


def path_bands(states, lens, n, bw, kb):
    """The distance band min(|i - j| // bw, kb) of every voiced-to-voiced step of the paths `states` [B, T] -> sorted unique bands."""
    out = set()
    for b in range(states.shape[0]):
        s = np.asarray(states[b, :int(lens[b])], np.int64)
        i, j = s[:-1], s[1:]
        v = (i < n) & (j < n)
        out |= set(np.minimum(np.abs(i - j)[v] // bw, kb).tolist())
    return sorted(out)


# seed index of emissions_jumps per (kind, n, bw, kb) for the [6, T, n + 1] ragged batches of tests/test_gpu_step_geometries.py
# (T = 150, 100 above 800 states): the lowest k of 0 .. 11 for which the oracle's paths use every distance band 0 .. kb -- each
# test asserts that premise -- and a back-trace that clamps the band index to kb - 1 decodes another path (checked once on the
# host with tests/plan_replay.py: replay_step)
JUMP_K = {("durrieu", 367, 5, 9): 4, ("durrieu", 500, 7, 9): 1, ("durrieu", 1023, 64, 9): 3, ("generated", 128, 4, 15): 6,
          ("generated", 199, 12, 15): 7, ("generated", 1023, 63, 15): 1, ("durrieu", 705, 20, 9): 2, ("durrieu", 706, 20, 9): 3,
          ("durrieu", 707, 20, 9): 1, ("durrieu", 708, 20, 9): 1, ("durrieu", 768, 20, 9): 1}


def jump_seed(kind, n, bw, kb):
    return 100 * JUMP_K.get((kind, n, bw, kb), 0) + n
