"""Step-structured plans at every geometry analyze_step (csrc/plan.cpp) accepts, on the CPU (no GPU needed): the recovered band
width and band count, the refusal at every boundary and after every single-entry edit, the band table in the plan image, a host
replay of the step kernels' arithmetic driven by the plan's own parameters, and the multiply-shift division of the back-trace.
The GPU tier (tests/test_gpu_step_geometries.py) decodes the same geometries."""
import numpy as np
import pytest

from oracle import viterbi_oracle as vo
from tests.common import GEN, durrieu_log_params, emissions_jumps, step_matrix
from tests.plan_replay import STEP_ROWS, HostPlan, replay_step, step_backtrace_weights, step_multiplier

# (n voiced states, bins per semitone): synth.durrieu_transition, nine near bands each
DURRIEU = [(705, 20), (706, 20), (707, 20), (708, 20), (768, 20), (769, 20), (128, 4), (128, 12), (300, 16), (367, 5), (368, 8),
           (500, 7), (641, 64), (1023, 64)]
# (n, bw, kb): tests.common.step_matrix
GENERATED = [(128, 4, 1), (128, 4, 15), (199, 12, 15), (1023, 63, 15), (1023, 64, 14), (400, 5, 3)]


def _uniform(n):
    return np.full(n + 1, np.float32(np.log(np.float32(1.0 / (n + 1)))), np.float32)


_cache = {}


def accepted(kind, n, bw, kb=9):
    """(A, pi, plan) of one accepted geometry, built once per session (the matrices are read, never written)."""
    key = (kind, n, bw, kb)
    if key not in _cache:
        if kind == "durrieu":
            A, pi = durrieu_log_params(n, bw)
        else:
            A, pi = step_matrix(n, bw, kb, np.random.default_rng(1000 * n + 16 * bw + kb)), _uniform(n)
        A.setflags(write=False)
        _cache[key] = (A, pi, HostPlan(A, pi))
    return _cache[key]


ALL = [("durrieu", n, bps, 9) for n, bps in DURRIEU] + [("generated", n, bw, kb) for n, bw, kb in GENERATED]


def _id(case):
    return "%s-n%d-bw%d-kb%d" % case


# ------------------------------------------------------------------ 1. acceptance
@pytest.mark.parametrize("case", ALL, ids=_id)
def test_accepted_geometries_recover_band_width_and_count(case):
    kind, n, bw, kb = case
    A, pi, plan = accepted(*case)
    assert not plan.ok, "premise: the banded analysis refuses the matrix"
    assert plan.step_ok and (plan.step_bw, plan.step_kb) == (bw, kb), (plan.step_ok, plan.step_bw, plan.step_kb)
    assert plan.S == n + 1 and plan.SP == (n + 1 + 63) // 64 * 64
    assert plan.step_cn.tobytes() == A[0, n].tobytes()


# ------------------------------------------------------------------ 2. refusal
@pytest.mark.parametrize("n,bw,kb", [(127, 4, 3), (200, 3, 5), (400, 65, 3), (400, 8, 16), (192, 12, 15), (128, 64, 1), (130, 13, 9)],
                         ids=lambda v: str(v))
def test_refused_by_size_or_shape(n, bw, kb):
    """n < 128, a band width outside 4 .. 64, more than 15 near bands, and (kb + 1) * bw >= n (== n in three of the cases): each
    matrix has the structure, the plan has no table for it."""
    A = step_matrix(n, bw, kb, np.random.default_rng(n + bw + kb))
    plan = HostPlan(A, _uniform(n))
    assert not plan.ok and not plan.step_ok
    assert not plan.stepC.any(), "no table is written for a refused matrix"


def test_refused_durrieu_640_64():
    A, pi = durrieu_log_params(640, 64)                      # (9 + 1) * 64 == n
    plan = HostPlan(A, pi)
    assert not plan.ok and not plan.step_ok
    A, pi = durrieu_log_params(127, 4)
    assert not HostPlan(A, pi).step_ok


def test_the_smallest_accepted_sizes_sit_next_to_the_refused_ones():
    """The boundary from the accepted side: n = 128, bw = 4 and 64, kb = 15, (kb + 1) * bw == n - 1."""
    for n, bw, kb in ((128, 4, 15), (130, 64, 1), (193, 12, 15), (641, 64, 9)):
        plan = HostPlan(step_matrix(n, bw, kb, np.random.default_rng(3)), _uniform(n))
        assert not plan.ok and plan.step_ok and (plan.step_bw, plan.step_kb) == (bw, kb), (n, bw, kb)


def _ulp_up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


EDIT_BASES = [("generated", 400, 5, 3), ("generated", 199, 12, 15), ("durrieu", 300, 16, 9)]


@pytest.mark.parametrize("case", EDIT_BASES, ids=_id)
def test_single_entry_edits_are_refused(case):
    kind, n, bw, kb = case
    A0, pi, plan0 = accepted(*case)
    assert plan0.step_ok
    j = n // 2

    def refused(edit, what):
        B = np.array(A0)
        edit(B)
        assert int(np.sum(B.view(np.uint32) != A0.view(np.uint32))) == 1, what
        assert not HostPlan(B, pi).step_ok, what

    def setv(r, c, v):
        def f(B):
            B[r, c] = v
        return f

    refused(setv(j, j + 1, _ulp_up(A0[j, j + 1])), "near band, one ulp up")
    refused(setv(j, j + bw, np.nextafter(A0[j, j + bw], np.float32(-np.inf))), "second band, one ulp down")
    refused(setv(2, n - 1, _ulp_up(A0[2, n - 1])), "far band, one ulp up")
    refused(setv(n - 1, 0, _ulp_up(A0[n - 1, 0])), "far band of source column 0")
    refused(setv(bw, 0, A0[0, 0]), "source column 0: band 0 one bin too wide")
    refused(setv(7, n, _ulp_up(A0[7, n])), "unvoiced source column")
    refused(setv(0, n, A0[0, n] - np.float32(1)), "unvoiced source column, target 0")
    assert n - 2 >= kb * bw                                   # (n - 1, 1) lies in the far band of source column 1
    refused(setv(2, 1, A0[n - 1, 1] - np.float32(1)), "a near value below its column's far value")
    refused(setv(j, j - 2, np.float32(np.nan)), "NaN in a near band")
    refused(setv(1, n - 2, np.float32(np.nan)), "NaN in the far band")
    # the unvoiced target's row is arbitrary: an edit there changes nothing
    B = np.array(A0)
    B[n, 5] -= np.float32(3)
    p = HostPlan(B, pi)
    assert p.step_ok and (p.step_bw, p.step_kb) == (bw, kb)


def test_a_whole_band_below_the_far_value_is_refused():
    """Consistent bits, but the near band of one column is below the column's far value: the one far maximum would be wrong."""
    n, bw, kb = 400, 5, 3
    A0, pi, _ = accepted("generated", n, bw, kb)
    i = 200
    B = np.array(A0)
    idx = np.arange(n)
    band1 = (np.abs(idx - i) // bw) == 1
    B[:n, i][band1] = A0[0, i] - np.float32(0.5)              # A0[0, i]: the far value of column i
    assert not HostPlan(B, pi).step_ok
    B[:n, i][band1] = A0[0, i]                                # equal to the far value: allowed
    assert HostPlan(B, pi).step_ok


def test_signed_zero_mix_inside_a_band_is_refused():
    """The proof compares bit patterns: +0 and -0 in one band are two values."""
    n, bw, kb = 400, 5, 3
    A0 = step_matrix(n, bw, kb, np.random.default_rng(8), zero_top=True)
    pi = _uniform(n)
    plan = HostPlan(A0, pi)
    assert not plan.ok and plan.step_ok and (plan.step_bw, plan.step_kb) == (bw, kb)
    j = 150
    assert A0[j, j + 1].tobytes() == np.float32(0.0).tobytes()
    B = np.array(A0)
    B[j, j + 1] = np.float32(-0.0)
    assert np.array_equal(A0, B)                               # equal by value
    assert not HostPlan(B, pi).step_ok
    B = np.array(A0)
    B[:n, j + 1][np.abs(np.arange(n) - (j + 1)) < bw] = np.float32(-0.0)   # the whole band -0: one value again
    assert HostPlan(B, pi).step_ok


# ------------------------------------------------------------------ 3. the band table
@pytest.mark.parametrize("case", ALL, ids=_id)
def test_band_table_holds_the_matrix(case):
    kind, n, bw, kb = case
    A, pi, plan = accepted(*case)
    assert plan.step_ok and plan.stepC.shape == (STEP_ROWS, plan.SP)
    idx = np.arange(n)
    band = np.minimum(np.abs(idx[None, :] - idx[:, None]) // bw, kb)           # [target j, source i]
    got = plan.stepC[band, idx[None, :]]
    assert got.tobytes() == np.ascontiguousarray(A[:n, :n]).tobytes()
    ninf = np.float32(-np.inf)
    assert np.all(plan.stepC[kb + 1:] == ninf), "rows past the far band"
    assert np.all(plan.stepC[:, n:] == ninf), "columns past the voiced states"
    # a band no voiced target reaches from source i (distance to the farther end below k * bw)
    reach = np.maximum(idx, n - 1 - idx)[None, :] >= (np.arange(kb + 1) * bw)[:, None]
    assert np.all(plan.stepC[:kb + 1, :n][~reach] == ninf)
    assert np.all(np.isfinite(plan.stepC[:kb + 1, :n][reach]))
    if (n, bw, kb) == (199, 12, 15):
        assert not reach[kb, n // 2] and not reach.all(axis=1)[kb], "premise: the far band is not reached from a middle source"
        assert reach[kb, 0] and reach[kb, n - 1]


# ------------------------------------------------------------------ 4. host replay of the kernels' arithmetic
@pytest.mark.parametrize("case", ALL, ids=_id)
def test_backtrace_weights_equal_the_matrix(case):
    """What the back-trace adds for target j and source i -- the band table through the multiply-shift index and the clamp -- is the
    matrix entry, bit for bit, for every pair: the path-independent half of the replay below (a path visits few of the pairs)."""
    _, n, bw, kb = case
    A, pi, plan = accepted(*case)
    W = np.stack([step_backtrace_weights(plan, j) for j in range(n + 1)])
    assert W.tobytes() == A.tobytes(), np.argwhere(W.view(np.uint32) != A.view(np.uint32))[:4]


def delta_rows(A, pi, E):
    """Every delta row of the dense recursion from the oracle: song b of the batch is the first b + 1 frames, its final delta row
    is row b.  -> (states, loglik, rows [T, S])."""
    T = E.shape[0]
    batch = np.ascontiguousarray(np.broadcast_to(E[None], (T,) + E.shape))
    st, ll, rows = vo.decode_c(A, pi, batch, lengths=np.arange(1, T + 1), return_delta=True)
    return st[T - 1].astype(np.int64), ll[T - 1], rows


REPLAY = [("durrieu", 706, 20, 9), ("durrieu", 128, 4, 9), ("durrieu", 300, 16, 9), ("durrieu", 367, 5, 9), ("durrieu", 641, 64, 9),
          ("generated", 128, 4, 1), ("generated", 128, 4, 15), ("generated", 199, 12, 15), ("generated", 400, 5, 3),
          ("generated", 1023, 63, 15)]


def check_replay(A, pi, plan, E, replay=replay_step):
    st, ll, rows = replay(plan, E)
    ref_s, ref_l, ref_rows = delta_rows(A, pi, E)
    assert rows.tobytes() == ref_rows.tobytes(), np.argwhere(rows.view(np.uint32) != ref_rows.view(np.uint32))[:4]
    assert np.float32(ll).tobytes() == np.float32(ref_l).tobytes()
    assert np.array_equal(st, ref_s), np.nonzero(st != ref_s)[0][:8]


@pytest.mark.parametrize("kind", ["dense", "ties", "jumps"])
@pytest.mark.parametrize("case", REPLAY, ids=_id)
def test_step_replay_is_bit_exact(case, kind):
    """Forward: band-window maxima plus one far maximum; back-trace: the multiply-shift band index clamped to kb.  States,
    log-likelihood and every delta row equal the dense oracle's.  "jumps": emissions whose best path hops across the distance bands
    (the i.i.d. kinds stay in the nearest ones), so a wrong band index or a wrong far maximum changes the result."""
    _, n, bw, kb = case
    A, pi, plan = accepted(*case)
    assert not plan.ok and plan.step_ok and (plan.step_bw, plan.step_kb) == (bw, kb)
    T = 24 if n > 800 else 40
    E = emissions_jumps(1, T, n + 1, 7 + n, bw)[0] if kind == "jumps" else GEN[kind](1, T, n + 1, seed=7 + n)[0].numpy()
    check_replay(A, pi, plan, E)


def test_step_replay_with_zero_bands_and_signed_zero_emissions():
    n, bw, kb = 199, 12, 15
    rng = np.random.default_rng(21)
    A = step_matrix(n, bw, kb, rng, zero_top=True)
    pi = np.where(rng.random(n + 1) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    plan = HostPlan(A, pi)
    assert not plan.ok and plan.step_ok and (plan.step_bw, plan.step_kb) == (bw, kb)
    E = np.where(rng.random((40, n + 1)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    E[::7] = -(rng.integers(0, 3, (6, n + 1)) / 2).astype(np.float32)
    st, ll, rows = replay_step(plan, E)
    ref_s, ref_l, ref_rows = delta_rows(A, pi, E)
    assert np.array_equal(st, ref_s) and np.array_equal(rows, ref_rows) and ll == ref_l     # by value: the sign of a zero sum is free


# ------------------------------------------------------------------ 5. the multiply-shift division
def test_multiply_shift_equals_the_division():
    """band = min((d * ceil(65536 / bw)) >> 16, kb) for every band width and every distance a 1024-state plan can hold.  The shift
    is the exact quotient for d < 1024 (d * (mult * bw - 65536) < 1024 * 64 = 65536), so no clamp is needed to hide an overestimate;
    bt_args_from_plan (capi.hip) drops the band table for a bw that fails this, so a wider accepted range must keep it true."""
    d = np.arange(1024, dtype=np.int64)
    for bw in range(4, 65):
        mult = step_multiplier(bw)
        assert mult == -(-65536 // bw) and mult * 1023 < 2 ** 32
        q = (d * mult) >> 16
        assert np.array_equal(q, d // bw), bw
        for kb in (1, 9, 15):
            assert np.array_equal(np.minimum(q, kb), np.minimum(d // bw, kb)), (bw, kb)
    # the floor multiplier is NOT exact: the ceiling is needed
    assert any(((d * (65536 // bw)) >> 16 != d // bw).any() for bw in range(4, 65))
