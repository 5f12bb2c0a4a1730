"""Inputs whose addresses pass element index 2^31 and byte offset 2^32 of every buffer a decode touches, with expected results that
cost seconds (tests/test_far_offsets_host.py, tests/test_gpu_far_offsets_*.py).  Plain NumPy and the oracle; no GPU in here.

The marks.  A buffer of `itemsize`-byte elements has two: element index `mark` (where a 32-bit signed element index wraps) and byte
offset `2 * mark` (where a 32-bit unsigned byte offset wraps); mark = 2^31 in the GPU tier, a few thousand elements in the host
tier, which runs the same constructions through the oracle alone.  For float16 emissions the two coincide.

A  far song bases: [B, T, S] with T * S past the marks and live lengths of a few hundred frames -- song 1 starts past every mark
   of the emissions and of the history; the compute is that of a short batch.  (The marks of `states` are out of reach: 2^31
   int32 states belong to 3 TB of emissions.)
B  many songs: B * T past the marks with T about 1500, the batch 8 distinct songs repeated; padded and packed.
C  one recording longer than the marks: stretches on which a single state k is alive (the path is k, the score a scalar
   recursion the oracle computes on the one-state HMM [[A_kk]]) and islands of ordinary emissions around every mark row, which the
   oracle decodes from the stretch frame in front (a one-hot prior holding the entering score) to the stretch frame behind (which
   forces k again).  piecewise_expected chains them; the host tier proves the chain equal to ONE oracle run over the recording.
"""
import ctypes

import numpy as np
import torch

from oracle import observation_oracle as oo
from oracle import viterbi_oracle as vo
from viterbi_spl_amd import synth

MARK = 1 << 31
KINDS = {"peaks": synth.emissions_peaks, "dense": synth.emissions_dense, "ties": synth.emissions_ties}
PLANS_A = ("tonet361", "msnet321", "jdc722", "durrieu722", "dense361")


# ------------------------------------------------------------------------------------------------------------- marks and strides
def mark_elements(itemsize, mark=MARK):
    """The element indices of a buffer's two marks: element `mark`, and the element at byte offset 2 * mark."""
    return sorted({int(mark), 2 * int(mark) // int(itemsize)})


def mark_rows(row_elems, itemsize, mark=MARK):
    """The rows (frames) of a buffer of `row_elems`-element rows that hold its marks."""
    return sorted({e // int(row_elems) for e in mark_elements(itemsize, mark)})


def rows_past(buffers, mark=MARK):
    """The smallest row count n for which rows 0 .. n - 1 of EVERY buffer (row_elems, itemsize) reach past both of its marks: some
    element of row n - 1 lies at or beyond the higher mark."""
    return max(max(mark_rows(r, i, mark)) for r, i in buffers) + 1


def create_plan(lib, A, pi):
    A = np.ascontiguousarray(A, np.float32)
    pi = np.ascontiguousarray(pi, np.float32)
    plan = ctypes.c_void_p()
    assert lib.vit_plan_create(A.ctypes.data, pi.ctypes.data, A.shape[0], ctypes.byref(plan)) == 0
    return plan


def _slope(size_of, n=1 << 16):
    """Bytes per frame of a size query that grows by whole rows: size_of(T) for one song at T = n and 2n (n a multiple of 64, so the
    256-byte alignment of the history's end adds nothing); 0 where the query refuses."""
    a, b = int(size_of(n)), int(size_of(2 * n))
    if a == 0 or b == 0:
        return 0
    assert (b - a) % n == 0, (a, b)
    return (b - a) // n


def history_rows(lib, plan):
    """The history row of every layout the plan serves, read off the library's own size queries -> {name: (row_elems, itemsize)}:
    "group" / "wave" / "dense" (vit_workspace_bytes_for, full history), "f64" (rows of doubles), "packed", "stream"."""
    from viterbi_spl_amd import _lib
    out = {}
    assert lib.vit_plan_set_option(plan, b"reset", 0) == 0
    for name in ("dense", "group", "wave", "auto"):
        per = _slope(lambda T: lib.vit_workspace_bytes_for(plan, 1, T, _lib.ALGO[name]))
        if per:
            out[name] = (per // 4, 4)
    for name, fn, size in (("f64", lib.vit_workspace_bytes_f64, 8), ("packed", lib.vit_workspace_bytes_packed, 4),
                           ("f64_packed", lib.vit_workspace_bytes_f64_packed, 8), ("stream", lib.vit_workspace_bytes_stream, 4)):
        per = _slope(lambda T: fn(plan, 1, T))
        if per:
            assert per % size == 0
            out[name] = (per // size, size)
    return out


# ------------------------------------------------------------------------------------------------------------- construction A
# ragged, odd ones, a song of one frame -- song 0, at the low offsets: every FAR song (1, and 2 of three) has a few hundred frames,
# so its far emission rows are read and its far history rows are written by the forward pass AND read back by the back-trace
LIVE_A = {3: (1, 301, 257), 2: (1, 257)}


def shape_a(S, e_itemsize, hist, mark=MARK, budget=60 << 30):
    """(B, T) of construction A: T the fewest frames whose emission rows AND history rows (hist = (row_elems, itemsize) or None)
    pass both marks, so that song 1 starts past every mark of both buffers; three songs where emissions + history fit `budget`
    bytes, else two."""
    buffers = [(S, e_itemsize)] + ([hist] if hist else [])
    T = rows_past(buffers, mark)
    per_song = T * sum(r * i for r, i in buffers)
    B = 3 if 3 * per_song <= budget else 2
    return B, T


def live_songs(kind, lens, S, seed, f16=False):
    """The live frames of construction A: synth's generator -> float32 or float16 [B, max(lens), S] on the host."""
    return KINDS[kind](len(lens), max(lens), S, seed=seed, dtype=torch.float16 if f16 else torch.float32).numpy()


def expected_a(A, pi, live, lens):
    """The oracle on the live frames -> (states int32 [B, max(lens)] with -1 behind each length, loglik float32 [B])."""
    st, ll = vo.decode_c(A, pi, np.asarray(live, np.float32), lengths=np.asarray(lens, np.int64))
    st = st.copy()
    for b, n in enumerate(lens):
        st[b, n:] = -1
    return st, ll


# ------------------------------------------------------------------------------------------------------------- construction B
LENS_B = (1500, 1499, 1373, 1, 1437, 1500, 777, 1002)          # the eight lengths the packed batches cycle through


def shape_b(S, e_itemsize, hist, T=1500, mark=MARK):
    """(B, T): the fewest songs of T frames, a multiple of 8, whose emission and history rows pass both marks."""
    buffers = [(S, e_itemsize)] + ([hist] if hist else [])
    B = -(-rows_past(buffers, mark) // T)
    return -(-B // 8) * 8, T


def packed_offsets(B, lens8):
    """int64 [B + 1]: recording b has lens8[b % 8] frames."""
    n = np.asarray([lens8[b % 8] for b in range(B)], np.int64)
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


def count_b_packed(S, e_itemsize, hist, lens8, mark=MARK):
    """The fewest recordings, a multiple of 8, whose packed rows pass both marks of the emissions and the history."""
    buffers = [(S, e_itemsize)] + ([hist] if hist else [])
    need, per8 = rows_past(buffers, mark), int(sum(lens8))
    return -(-need // per8) * 8


def base_songs(S, T, f16, seed):
    """The 8 distinct songs of construction B, [8, T, S] in the emission type on the host: three of peaks, three dense, two of ties."""
    return np.concatenate([live_songs("peaks", [T] * 3, S, seed, f16), live_songs("dense", [T] * 3, S, seed + 1, f16),
                           live_songs("ties", [T] * 2, S, seed + 2, f16)], axis=0)


def packed_batch_b(A, pi, base, lens8, hist, f16, f64=False, mark=MARK):
    """Construction B, packed: the fewest recordings (a multiple of 8, recording b = base[b % 8][:lens8[b % 8]]) whose rows pass both
    marks of the emissions and of `hist`.  -> dict(B, off, period: the 8 recordings' rows concatenated [sum lens8, S] (the batch is
    B / 8 copies of it), ref_s [8, T] / ref_l [8]: the oracle's decode of the 8 (f64: tests/f64_ref.py's, loglik float64), want:
    their states concatenated like `period`, picks: the recordings compared one by one)."""
    from tests import f64_ref
    S, isz = base.shape[2], 2 if f16 else 4
    B = count_b_packed(S, isz, hist, lens8, mark)
    off = packed_offsets(B, lens8)
    assert int(off[-1]) * S > max(mark_elements(isz, mark)) and int(off[-1]) * hist[0] > max(mark_elements(hist[1], mark))
    if f64:
        ref_s, ref_l = f64_ref.decode_f64_batch(A, pi, np.asarray(base[:, :max(lens8)], np.float32), lens8)
        ref_s = ref_s.astype(np.int32)
    else:
        ref_s, ref_l = expected_a(A, pi, base, lens8)
    return {"B": B, "off": off, "ref_s": ref_s, "ref_l": ref_l,
            "period": np.concatenate([base[b, :n] for b, n in enumerate(lens8)], axis=0),
            "want": np.concatenate([ref_s[b, :n] for b, n in enumerate(lens8)]),
            "picks": straddlers(off, [(S, isz), hist], mark)}


def straddlers(offsets, buffers, mark=MARK):
    """The recordings that hold a mark row of one of the buffers, plus the first and the last."""
    off = np.asarray(offsets, np.int64)
    out = {0, len(off) - 2}
    for r, i in buffers:
        for row in mark_rows(r, i, mark):
            b = int(np.searchsorted(off, row, side="right")) - 1
            assert 0 <= b < len(off) - 1, "the batch does not reach the mark"
            out.add(b)
    return sorted(out)


# ------------------------------------------------------------------------------------------------------------- construction C
def survivor_state(A):
    """The state the stretches keep alive: in the middle of the grid, with a finite self-transition."""
    k = A.shape[0] // 2
    assert np.isfinite(A[k, k])
    return k


def stretch_value(A, k, f16):
    """The stretch emission of state k: -A[k][k] rounded to the emission type (the score then stays small)."""
    v = np.float32(-A[k, k])
    return np.float32(np.float16(v)) if f16 else v


def island_spans(N, buffers, island, mark=MARK):
    """The islands [s, e) of an N-frame recording: `island` frames at the start, `island` at the end, `island` around every mark row
    of every buffer (row_elems, itemsize), and `island` around the row a byte offset wrapped at 2 * mark would land in (mark row -
    2 * mark / row bytes) where that row exists.  Spans closer than two stretch frames merge into one."""
    want = [(0, island), (N - island, N)]
    for r, i in buffers:
        for row in mark_rows(r, i, mark):
            assert row < N, "the recording does not reach the mark"
            for centre in (row, row - (2 * mark) // (r * i)):
                if centre >= 0:
                    s = max(0, min(centre - island // 2, N - island))
                    want.append((s, s + island))
    spans = []
    for s, e in sorted(set(want)):
        if spans and s < spans[-1][1] + 2:
            spans[-1] = (spans[-1][0], max(e, spans[-1][1]))
        else:
            spans.append((s, e))
    assert spans[0][0] == 0 and spans[-1][1] == N
    for r, i in buffers:
        assert all(any(s <= row < e for s, e in spans) for row in mark_rows(r, i, mark))
    return spans


def island_emissions(kind, spans, S, seed, f16=False):
    """synth's generator, one "song" per island -> a list of [e - s, S] arrays of the emission type (host)."""
    E = KINDS[kind](len(spans), max(e - s for s, e in spans), S, seed=seed, dtype=torch.float16 if f16 else torch.float32).numpy()
    return [np.ascontiguousarray(E[n, :e - s]) for n, (s, e) in enumerate(spans)]


def fill_recording(E, k, v, spans, islands):
    """Write construction C into E [N, S] (a NumPy array or a torch tensor of the emission type, any device): -inf everywhere, v in
    column k, the islands over their frames."""
    E[:] = -np.inf
    E[:, k] = float(v)
    for (s, e), isl in zip(spans, islands):
        E[s:e] = torch.from_numpy(isl).to(E.device) if isinstance(E, torch.Tensor) else isl


def _stretch_f32(a_kk, v, d, n):
    """The float32 score of the survivor after n more stretch frames from score d: the oracle on the one-state HMM [[A_kk]] (a first
    frame of emission 0 carries d in)."""
    if n == 0:
        return np.float32(d)
    E = np.full((1, n + 1, 1), v, np.float32)
    E[0, 0, 0] = 0.0
    _, ll = vo.decode_c(np.full((1, 1), a_kk, np.float32), np.asarray([d], np.float32), E)
    return np.float32(ll[0])


def _stretch_f64(a_kk, v, d, n):
    """The same for the float64 family: d <- fl64(fl64(d + f64(A_kk)) + f64(v)), n times (tests/f64_ref.py's recursion for S = 1,
    whose arg max is trivial)."""
    a, e, d = np.float64(np.float32(a_kk)), np.float64(np.float32(v)), np.float64(d)
    for _ in range(n):
        nxt = (d + a) + e
        if nxt == d:                                               # a fixed point: every later frame repeats it
            break
        d = nxt
    return d


def piecewise_expected(A, pi, k, v, N, spans, islands, f64=False):
    """The expected decode of construction C, island by island -> (states int32 [N], loglik: float32, or float64 with `f64`).
    Each island is decoded by the oracle (f64: tests/f64_ref.decode_f64) from the stretch frame in front of it -- a one-hot prior
    with the entering score, a frame of emission 0 -- to the stretch frame behind it; the first island starts the recording with the
    real prior, the last one ends it."""
    from tests import f64_ref
    A = np.ascontiguousarray(A, np.float32)
    S = A.shape[0]
    states = np.full(N, k, np.int32)
    stretch = np.full(S, -np.inf, np.float32)
    stretch[k] = v
    d, at = None, None                                            # the survivor's score at stretch frame `at`
    for (s, e), isl in zip(spans, islands):
        rows = [np.asarray(isl, np.float32)]
        if s == 0:
            prior = np.asarray(pi, np.float32)
        else:
            d = (_stretch_f64 if f64 else _stretch_f32)(A[k, k], v, d, s - 1 - at)
            prior = np.full(S, -np.inf, np.float64 if f64 else np.float32)
            prior[k] = d
            rows.insert(0, np.zeros((1, S), np.float32))
        if e < N:
            rows.append(stretch[None])
        E = np.ascontiguousarray(np.concatenate(rows, axis=0))
        if f64:
            st, drow = _decode_f64_from(A, prior, E) if s > 0 else f64_ref.decode_f64(A, prior, E)
        else:
            st, _, drow = vo.decode_c(A, prior, E, return_delta=True)
        lead = 0 if s == 0 else 1
        assert lead == 0 or st[0] == k
        states[s:e] = st[lead:lead + e - s]
        if e == N:
            return states, (np.float64 if f64 else np.float32)(drow[st[-1]])
        assert st[-1] == k and np.isfinite(drow[k]), "the island cannot reach the survivor again"
        d, at = drow[k], e
    raise AssertionError("no island ends the recording")


def _decode_f64_from(A, d0, E):
    """tests/f64_ref.decode_f64 entered with a float64 score row d0 in place of fl32(log_pi + E_0) (E[0] is the frame that carries it)."""
    A64 = np.ascontiguousarray(A, np.float32).astype(np.float64)
    T, S = E.shape
    ar = np.arange(S)
    psi = np.empty((T, S), np.int32)
    d = np.asarray(d0, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(1, T):
            c = d[None, :] + A64
            i = np.argmax(c, axis=1)
            psi[t] = i
            d = c[ar, i] + E[t].astype(np.float64)
    s = int(np.argmax(d))
    states = np.empty(T, np.int64)
    states[T - 1] = s
    for t in range(T - 2, -1, -1):
        s = int(psi[t + 1, s])
        states[t] = s
    return states, d


def recording_c(A, pi, f16, buffers, kind, seed, island=150, mark=MARK, f64=False):
    """Everything of construction C but the emission tensor -> dict(N, k, v, spans, islands, states, loglik).  `buffers`: (row_elems,
    itemsize) of every buffer the recording's rows index (the emission rows first).  N: the fewest frames that pass every mark, the
    rest of the mark's island, eight stretch frames and the last island."""
    A = np.asarray(A, np.float32)
    N = rows_past(buffers, mark) + island // 2 + 8 + island
    k = survivor_state(A)
    v = stretch_value(A, k, f16)
    spans = island_spans(N, buffers, island, mark)
    islands = island_emissions(kind, spans, A.shape[0], seed, f16)
    states, loglik = piecewise_expected(A, pi, k, v, N, spans, islands, f64=f64)
    return {"N": N, "k": k, "v": v, "spans": spans, "islands": islands, "states": states, "loglik": loglik}


# ------------------------------------------------------------------------------------------------------------- row-independent kernels
def probe_rows(n_rows, row_elems_itemsizes, seed, mark=MARK, edge=64, n_random=4096):
    """The rows compared of a row-independent kernel: the first and last `edge`, `edge` around every mark row of every buffer
    (row_elems, itemsize) and n_random seeded ones -> sorted unique int64."""
    rng = np.random.default_rng(seed)
    rows = [np.arange(min(edge, n_rows)), np.arange(max(0, n_rows - edge), n_rows), rng.integers(0, n_rows, n_random)]
    for r, i in row_elems_itemsizes:
        for row in mark_rows(r, i, mark):
            assert row < n_rows, "the buffer does not reach the mark"
            rows.append(np.arange(max(0, row - edge // 2), min(n_rows, row + edge // 2)))
    return np.unique(np.concatenate(rows).astype(np.int64))


# ------------------------------------------------------------------------------------------------------------- the emission builders' bar
# (moved here from tests/test_gpu_builders.py, which imports them: the oracle side of a builder comparison and the bar it is held to)
TINY = np.float32(np.finfo(np.float32).tiny)
FLOOR = np.log(TINY)                                   # log(0 + tiny): a structural zero
ULP = float(np.spacing(-FLOOR))                        # float32 spacing at |log(tiny)|: 7.6e-6
VTH2 = 0.5                                             # mode 2's voicing-threshold probability: unvoiced logit 0


def builder_prior(U):
    p = np.random.default_rng(U).random(U + 1).astype(np.float32) + np.float32(1e-3)
    return p / p.sum()


def builder_oracle(mode, x, spw, prior=None):
    """The oracle restatement of the reference's builder of `mode` -> probabilities float32 [n, U+1], unvoiced last."""
    x = np.ascontiguousarray(x)
    if mode == 0:
        return np.ascontiguousarray(oo.shaun_observation_probs(x, 0.32, spw=spw).T)
    if mode == 1:
        return oo.softmax_observation_probs(x, spw=spw)
    return oo.softmax_scaled_observation_probs(x, np.float32(VTH2), prior if prior is not None else np.ones(x.shape[1] + 1, np.float32),
                                               scaled=prior is not None, spw=spw)


def _first_indices(mask, k=4):
    return [tuple(int(i) for i in ix) for ix in np.argwhere(mask)[:k]]


def assert_builder_matches(got, want_p, mode, what):
    """got: GPU log-emissions; want_p: the oracle's probabilities.  The structural log(tiny) set must be the same and the values within
    the bar.  Reference values a few ulp above log(tiny) (a subnormal p of up to ~190 times the smallest one) round onto log(tiny)
    or not by the last bit of the log - NumPy's or the GPU's - not by the builder: they leave the structural comparison and are held,
    with every value within 1.0 of log(tiny), to 3e-5 (4 ulp) in the log domain.  A flushed subnormal misses that by 4.7e-4 or more
    at spans up to 95 nats and is a structural difference below that."""
    want = np.log(want_p + TINY)
    exact = np.log(want_p.astype(np.float64) + np.float64(TINY))
    edge = (want_p > 0) & (exact < np.float64(FLOOR) + 3 * ULP)
    bad = ((got == FLOOR) != (want == FLOOR)) & ~edge
    assert not bad.any(), f"{what}: peak set / structural zeros differ at {_first_indices(bad)}"
    live = (want != FLOOR) & ~edge
    if mode == 2:
        ok = np.isclose(got, want, rtol=0, atol=2e-5)                # log-likelihoods up to +8: compared in the log domain
    else:
        ok = np.isclose(np.exp(got), np.exp(want), rtol=1e-5, atol=1e-30)
    bad = live & ~ok
    assert not bad.any(), f"{what}: values differ at {_first_indices(bad)}"
    near = (want_p > 0) & (exact < np.float64(FLOOR) + 1.0)
    bad = near & ~np.isclose(got, want, rtol=0, atol=3e-5)
    assert not bad.any(), f"{what}: the subnormal band differs at {_first_indices(bad)}: got {got[bad][:4]}, want {want[bad][:4]}"


# ------------------------------------------------------------------------------------------------------------- GPU-tier plumbing
def need_free(nbytes):
    """Skip the test where the device reports less free memory than the test holds at a time (the one skip these tests know)."""
    import pytest
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + (2 << 30):
        pytest.skip(f"{free} bytes of device memory free, the test holds {nbytes}")


class measured:
    """``with measured(test, shape):`` prints one line ``far_offsets_time {json}`` with the block's wall time (the device
    synchronised at both ends) and the peak of torch's allocator inside it: what profiles/far_offsets_time.json records."""

    def __init__(self, test, shape):
        self.test, self.shape = test, [int(x) for x in shape]

    def __enter__(self):
        import time
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, exc_type, exc, tb):
        import json
        import time
        if exc_type is None:
            torch.cuda.synchronize()
            print("far_offsets_time " + json.dumps({"test": self.test, "shape": self.shape, "seconds": round(time.perf_counter() - self.t0, 3),
                                                    "peak_bytes": int(torch.cuda.max_memory_allocated())}))
        return False


def release():
    """After the caller's ``del``: hand the allocator's cached blocks back before the next test allocates its tens of gigabytes."""
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def nan_batch(shape, dtype, dev):
    """An emission or logit tensor nobody may read outside the live frames: NaN everywhere."""
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)
