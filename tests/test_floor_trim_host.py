"""The split floor kernel's full waves evaluate only the live window entries of their targets (rows 0 .. 255): the plan's proof
of how many that is, and a host replay of the floor form with the dropped entries really left out, on the CPU.

A trailing window position is droppable when it is an extra column (the extra-column path forms that candidate anyway) or holds,
in bits, the row constant c_j: fl(delta_i + c_j) <= fl(M + c_j), which the floor form carries.  The replay below must therefore
reproduce every delta row, every frame maximum M, the path and the log-likelihood of the untrimmed recursion -- also where the
dropped candidate IS the row's maximum (the spike emissions), which the premises check on the CPU."""
import ctypes

import numpy as np
import pytest

from oracle import viterbi_oracle as vo
from tests import plan_replay
from tests.plan_replay import HostPlan, replay_banded
from tests.test_plan_host import _banded_matrix
from viterbi_spl_amd import synth

FULL_ROWS = 256          # targets of the split kernel's full-window waves (kSplitFullRows, plan.hpp)
NINF = np.float32(-np.inf)


def _widths(A, pi, n_rows=FULL_ROWS):
    """(proven live width of rows [0, n_rows), the width the split kernel's full waves then evaluate) from the host plan library."""
    lib = plan_replay._lib()
    lib.vph_live_width.restype = ctypes.c_int
    lib.vph_live_width.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.vph_split_full_width.restype = ctypes.c_int
    lib.vph_split_full_width.argtypes = [ctypes.c_void_p, ctypes.c_int]
    A = np.ascontiguousarray(A, np.float32)
    pi = np.ascontiguousarray(pi, np.float32)
    h = lib.vph_create(A.ctypes.data, pi.ctypes.data, A.shape[0])
    out = lib.vph_live_width(h, n_rows), lib.vph_split_full_width(h, 0)
    assert lib.vph_split_full_width(h, 1) == info_W(lib, h)     # fp16 emissions: always the whole window
    lib.vph_destroy(h)
    return out


def info_W(lib, h):
    info = np.zeros(16, np.int32)
    c0 = np.zeros(1, np.float32)
    lib.vph_info(h, info.ctypes.data, c0.ctypes.data)
    return int(info[3])


def _tonet(S):
    return synth.log_params(synth.tonet_transition(S - 1, 14 if S == 361 else 12), synth.floored_prior(S))


def _s300mid():
    rng = np.random.default_rng(300)
    A = _banded_matrix(300, 10, rng, extras=[148], floor=-50.0, quant=2)
    return A, -(rng.integers(0, 8, 300) / 2).astype(np.float32)


def _live_width_by_hand(A, plan, n_rows=FULL_ROWS):
    """The definition, from the plan image: 1 + the last position over rows [0, n_rows) that is no extra column and differs in bits from c_j."""
    last = 0
    for j in range(min(n_rows, plan.S)):
        for w in range(plan.W - 1, -1, -1):
            i = int(plan.lo[j]) + w
            if i not in plan.extras and plan.tabA[w, j].view(np.uint32) != plan.rowc[j].view(np.uint32):
                last = max(last, w)
                break
    return last + 1


def test_live_width_of_the_shipped_grids(golden):
    p = golden["params"]
    A, pi = _tonet(361)
    assert _widths(A, pi) == (29, 29)
    assert _widths(p["tonet361_logA_T"], p["tonet361_log_pi"]) == (29, 29)
    assert _widths(p["msnet321_logA_T"], p["msnet321_log_pi"]) == (25, 25)
    A, pi = _tonet(321)                                        # tonet_transition(320, 12)
    assert _widths(A, pi) == (25, 25)
    for A, pi in (_tonet(361), (p["msnet321_logA_T"], p["msnet321_log_pi"])):
        assert _widths(A, pi)[0] == _live_width_by_hand(A, HostPlan(A, pi))
    # every row: the clamped rows at the end of the grid reach position 30 (their lo is S - W), which is why the half waves keep W
    assert _widths(*_tonet(361), n_rows=361)[0] == 31


def test_no_trim_where_the_first_rows_are_clamped():
    """S = 257: row 255 is clamped to lo = S - W and its band reaches source 256 = position 31."""
    rng = np.random.default_rng(257)
    A = _banded_matrix(257, 12, rng, extras=[100], floor=-50.0, quant=2)
    pi = np.zeros(257, np.float32)
    plan = HostPlan(A, pi)
    assert plan.floor_ok and plan.W == 32 and plan.extras == [100] and plan.lo[255] == 257 - 32
    assert _widths(A, pi) == (32, 32)


def test_no_trim_with_a_live_entry_at_position_30():
    """tonet's matrix but for one non-constant entry at window position 30 of a row below 256: live width 31 by the definition
    (1 + the last live position); no trimmed instantiation covers it, so the full waves evaluate the whole window (32)."""
    A, pi = _tonet(361)
    A = A.copy()
    plan0 = HostPlan(A, pi)
    j = 100
    A[j, plan0.lo[j] + 30] = np.float32(-1.0)
    plan = HostPlan(A, pi)
    assert plan.ok and plan.floor_ok and plan.W == 32 and plan.lo[j] == plan0.lo[j]
    assert _widths(A, pi) == (31, 32)
    # ... and an in-span entry that happens to equal the constant stays evaluated: only the trailing run is trimmed
    A, pi = _tonet(361)
    A = A.copy()
    A[j, plan0.lo[j] + 20] = plan0.rowc[j]
    assert _widths(A, pi) == (29, 29)


def test_trailing_extra_column_is_trimmed():
    """S = 300, half-width 10 (21 live positions), the extra column mid-grid: for rows 127 .. 137 the extra column is a non-constant
    entry at positions 21 .. 31 of the window -- the only thing behind position 20 -- and the trim goes past it."""
    A, pi = _s300mid()
    plan = HostPlan(A, pi)
    assert plan.floor_ok and plan.W == 32 and plan.extras == [148]
    j = 130
    w = 148 - int(plan.lo[j])
    assert 21 <= w < 32 and plan.tabA[w, j] != plan.rowc[j]
    assert _widths(A, pi) == (21, 25)
    assert _live_width_by_hand(A, plan) == 21


def test_no_trim_without_the_floor_form():
    rng = np.random.default_rng(5)
    A = _banded_matrix(300, 4, rng, floor=-2.0, quant=1)       # window entries below the row constant: no floor form
    plan = HostPlan(A, np.zeros(300, np.float32))
    assert plan.ok and not plan.floor_ok
    assert _widths(A, np.zeros(300, np.float32)) == (plan.W, plan.W)


# ------------------------------------------------------------------------------------------------------------------------------
# host replay of the trimmed floor form
# ------------------------------------------------------------------------------------------------------------------------------
def replay_floor_trim(plan, logE, WF, n_full=FULL_ROWS):
    """The floor form with targets < n_full evaluating window positions [0, WF) only.  Returns (delta rows [T, S], M [T] = max of
    delta_t over the non-extra sources, stats) with stats = frames x targets < n_full where the dropped candidates hold the row's
    maximum: `wins` strictly above everything evaluated but fl(M + c_j), `ties` equal to the best evaluated window entry."""
    S, W = plan.S, plan.W
    logE = np.ascontiguousarray(logE, np.float32)
    T = logE.shape[0]
    lo = plan.lo[:S].astype(np.int64)
    win_idx = lo[:, None] + np.arange(W)[None, :]
    tab = plan.tabA[:, :S].T
    keep = np.arange(W)[None, :] < np.where(np.arange(S) < n_full, WF, W)[:, None]
    is_x = np.isin(win_idx, plan.extras)
    masked = np.zeros(S, bool)
    masked[plan.extras] = True
    hist = np.empty((T, S), np.float32)
    Ms = np.empty(T, np.float32)
    wins = ties = 0
    delta = (plan.log_pi[:S] + logE[0]).astype(np.float32)
    for t in range(T):
        if t > 0:
            cand = (delta[win_idx] + tab).astype(np.float32)
            inw = np.max(np.where(keep, cand, NINF), axis=1)
            ext = np.full(S, NINF, np.float32)
            for k, x in enumerate(plan.extras):
                ext = np.maximum(ext, (delta[x] + plan.extraA[k, :S]).astype(np.float32))
            floor = (Ms[t - 1] + plan.rowc[:S]).astype(np.float32)
            m = np.maximum(np.maximum(inw, ext), floor)
            dropped = np.max(np.where(~keep & ~is_x, cand, NINF), axis=1)
            top = (dropped == m) & np.isfinite(m)
            wins += int(np.sum(top & (dropped > np.maximum(inw, ext))))
            ties += int(np.sum(top & (dropped == inw)))
            delta = (m + logE[t]).astype(np.float32)
        hist[t] = delta
        Ms[t] = np.max(np.where(masked, NINF, delta))
    return hist, Ms, {"wins": wins, "ties": ties}


def _path(A, hist):
    """Dense back-trace over the delta rows, lowest index on ties (what the oracle's argmax does)."""
    T = hist.shape[0]
    s = int(np.argmax(hist[-1]))
    path = np.empty(T, np.int64)
    path[-1] = s
    for t in range(T - 2, -1, -1):
        s = int(np.argmax((hist[t] + A[s]).astype(np.float32)))
        path[t] = s
    return path


def spike_emissions(B, T, S, seed, quant=False, second=None):
    """Adversarial for the trim: on ~85 % of the frames one column (anywhere on the grid, so also 15 .. 17 bins above targets that
    drop those sources) gets an emission 200 .. 230 above the frame's largest; delta of that column is then the frame maximum M, and for
    the targets whose dropped window positions hold it the dropped candidate is the row's true maximum.  `quant`: every value a multiple
    of 1/2 (exact ties with a coarse matrix).  `second` = (distance, drop): a second column `distance` bins below the spike gets the
    spike's emission minus `drop` -- an evaluated in-window source of the spike's far targets that can tie fl(M + c_j)."""
    rng = np.random.default_rng(seed)
    if quant:
        E = -(rng.integers(0, 6, (B, T, S)) / 2).astype(np.float32)
    else:
        E = synth.emissions_peaks(B, T, S, seed=seed).cpu().numpy().copy()
    on = rng.random((B, T)) < 0.85
    col = rng.integers(20, S - 1, (B, T))
    top = E.max(axis=2) + 200 + rng.integers(0, 61, (B, T)).astype(np.float32) / 2
    for b in range(B):
        for t in np.nonzero(on[b])[0]:
            E[b, t, col[b, t]] = top[b, t]
            if second is not None:
                E[b, t, col[b, t] - second[0]] = top[b, t] - np.float32(second[1])
    return E.astype(np.float32)


def _replay_case(A, pi, E, WF):
    plan = HostPlan(A, pi)
    assert plan.floor_ok and plan.n_dense == 0 and plan.W == 32 and plan.S > FULL_ROWS
    hist, Ms, stats = replay_floor_trim(plan, E, WF)
    T = E.shape[0]
    masked = np.zeros(plan.S, bool)
    masked[plan.extras] = True
    for t in range(1, T + 1):                                  # every delta row of the untrimmed floor form: its final delta per prefix
        st, ll, delta = replay_banded(plan, E[:t], floor=True)
        assert delta.tobytes() == hist[t - 1].tobytes(), (t - 1, np.argwhere(delta != hist[t - 1])[:8])
        assert np.float32(np.max(np.where(masked, NINF, delta))).tobytes() == Ms[t - 1].tobytes(), t - 1
    ref_s, ref_l = vo.decode_numpy(A, pi, E)
    assert np.array_equal(st, ref_s) and np.array_equal(_path(A, hist), ref_s)
    assert np.float32(np.max(hist[-1])).tobytes() == np.float32(ref_l).tobytes() == np.float32(ll).tobytes()
    return stats


def _case(name, golden):
    if name == "tonet361":
        return _tonet(361) + (29,)
    if name == "tonet321":
        return _tonet(321) + (25,)
    if name == "msnet321":
        p = golden["params"]
        return p["msnet321_logA_T"], p["msnet321_log_pi"], 25
    A, pi = _s300mid()
    return A, pi, 21                                           # the proven width itself (the kernel would take 25)


@pytest.mark.parametrize("name", ["tonet361", "tonet321", "msnet321", "S300mid"])
def test_trimmed_replay_peaks(golden, name):
    A, pi, WF = _case(name, golden)
    assert _widths(A, pi)[0] == WF
    _replay_case(A, pi, synth.emissions_peaks(1, 40, A.shape[0], seed=3)[0].numpy(), WF)


@pytest.mark.parametrize("name", ["tonet361", "tonet321", "msnet321", "S300mid"])
def test_trimmed_replay_spikes(golden, name):
    """The dropped candidates are the row's true maximum on many (frame, target) pairs and fl(M + c_j) must reproduce them."""
    A, pi, WF = _case(name, golden)
    stats = _replay_case(A, pi, spike_emissions(1, 40, A.shape[0], seed=5, quant=name == "S300mid")[0], WF)
    assert stats["wins"] >= 20, stats                           # premise: the case tests something


def test_trimmed_replay_spike_ties():
    """Coarse matrix and emissions, and a second planted column 20 bins below the spike, 35 lower: for the spike's far targets (16 .. 21
    bins below it here: half-width 10, window 32) that column is an evaluated in-window source at distance <= 4, and
    fl(delta + a) with a in {0, -1/2, .. -19.5} meets fl(M - 50) exactly where a = -15 -- ties between a dropped candidate and an
    evaluated one."""
    A, pi = _s300mid()
    E = spike_emissions(1, 40, 300, seed=7, quant=True, second=(20, 35.0))[0]
    stats = _replay_case(A, pi, E, 21)
    assert stats["wins"] >= 20 and stats["ties"] >= 1, stats
