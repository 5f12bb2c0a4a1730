"""CPU tier of the packed float64 decode under a workspace budget (vit_decode_f64_packed_checkpointed): the exports, the size function
and the unit count on host-only plans, and the segment-length search of plan_workspace_f64_packed_bounded."""
import ctypes
import os

import numpy as np
import pytest

from tests.plan_replay import HostPlan
from viterbi_spl_amd import ViterbiDecoder
from viterbi_spl_amd._lib import ViterbiHipError

NAMES = ("vit_workspace_bytes_f64_packed_checkpointed", "vit_decode_f64_packed_checkpointed", "vit_f64_packed_bounded_units")
CUS = 256          # compute units a plan assumes before its upload
LENGTH_SETS = ((257, 1, 5, 100, 2), (30000, 7500, 64, 65), (64,), (4096,) * 7, tuple(range(1, 40)))
SEGMENTS = (64, 65, 1024, 1 << 24)


@pytest.fixture(scope="module")
def lib():
    from viterbi_spl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _plan(lib, A, pi):
    A, pi = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(pi, np.float32)
    plan = ctypes.c_void_p()
    assert lib.vit_plan_create(A.ctypes.data, pi.ctypes.data, A.shape[0], ctypes.byref(plan)) == 0
    return plan


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)


def _units_per_cu(W, S):
    """the header's rule restated: 1 on twelve target waves, else the workgroups whose waves one compute unit's registers hold (four
    SIMDs of 4, 3, 2 waves at W = 16, 32, wider), at most 4"""
    nwt = next(n for n in (2, 4, 6, 8, 12) if 64 * n >= S)
    if nwt >= 12:
        return 1
    return max(1, min(4, 4 * (4 if W <= 16 else 3 if W <= 32 else 2) // nwt))


def _r(x):
    return (int(x) + 255) // 256 * 256


def test_header_loader_and_exports_agree(lib):
    from tests.test_abi import declared_functions
    from viterbi_spl_amd import _lib
    for n in NAMES:
        assert n in declared_functions() and n in _lib.EXPORTS and hasattr(lib, n), n
    assert lib.vit_abi_version() == 4
    assert lib.vit_workspace_bytes_f64_packed_checkpointed.restype is ctypes.c_size_t
    assert lib.vit_decode_f64_packed_checkpointed.restype is ctypes.c_int32
    assert lib.vit_f64_packed_bounded_units.restype is ctypes.c_int64
    assert [len(getattr(lib, n).argtypes) for n in NAMES] == [4, 11, 2]


def test_size_function_on_the_host(lib, golden):
    """Host-only plans of the 321-, 361- and 722-state bands.  With K = min(segment_frames, longest recording), n_b = ceil(T_b / K),
    U = sum n_b, n = min(B, u x 256) units per launch and rows of SD = (S + 3) / 2 * 2 doubles, the header's layout is
      r((U - B) SD 8) + r(n (K + 1) SD 8) + r(4 B) + r(128 n) + r(8 n) + r(4 n) + r(8 n)
      + 2 r(8 (B + 1)) + r(4 (slots + 1)) + r(4 B) + 2 r(4 U),  slots = min(B, 8 x 256) <= B,
    which this test also evaluates exactly.  Over the rows the decode cannot do without, (U - B + n K) SD 8, that is ONE row per unit
    (in front of the segment), 148 bytes of per-unit arrays per unit, at most 28 bytes per recording and 8 per (recording, segment),
    20 bytes, and thirteen round-ups of at most 255 bytes -- inside the slack of two rows and 160 bytes per unit, 64 bytes per
    recording and unit and 24 round-ups.  It falls below the whole history once every recording has 4 K frames and B <= n; a K
    above the longest recording gives the size at that length."""
    p = golden["params"]
    size = lib.vit_workspace_bytes_f64_packed_checkpointed
    for name, S in (("msnet321", 321), ("tonet361", 361), ("jdc722", 722)):
        A, pi = p[f"{name}_logA_T"], p[f"{name}_log_pi"]
        plan = _plan(lib, A, pi)
        u = _units_per_cu(HostPlan(A, pi).W, S)
        row = (S + 3) // 2 * 2 * 8
        for lens in LENGTH_SETS:
            off = _offsets(lens)
            B, N, tmax = len(lens), int(off[-1]), max(lens)
            n = lib.vit_f64_packed_bounded_units(plan, B)
            assert n == min(B, u * CUS), (name, B, n, u)
            for K in SEGMENTS:
                Kc = min(K, tmax)
                units = sum(-(-t // Kc) for t in lens)
                need = size(plan, B, off.ctypes.data, K)
                floor = (units - B + n * Kc) * row
                assert need >= floor, (name, lens, K, need)
                assert need <= floor + n * row + 148 * n + 28 * B + 8 * units + 20 + 13 * 255, (name, lens, K, need)
                assert need <= floor + 2 * n * row + 64 * (B + units) + 24 * 256 + 160 * n, (name, lens, K, need)
                exact = (_r((units - B) * row) + _r(n * (Kc + 1) * row) + _r(4 * B) + _r(128 * n) + _r(8 * n) + _r(4 * n) + _r(8 * n)
                         + 2 * _r(8 * (B + 1)) + _r(4 * (min(B, 8 * CUS) + 1)) + _r(4 * B) + 2 * _r(4 * units))
                assert need == exact, (name, lens, K, need, exact)
                if min(lens) >= 4 * K and B <= n:
                    assert need < lib.vit_workspace_bytes_f64_packed(plan, B, N), (name, lens, K)
            assert size(plan, B, off.ctypes.data, 1 << 24) == size(plan, B, off.ctypes.data, max(tmax, 64)), (name, lens)
        lib.vit_plan_destroy(plan)
    assert any(min(lens) >= 4 * K for lens in LENGTH_SETS for K in SEGMENTS), "premise: the comparison with the whole history ran"


def test_units_grow_with_the_batch_up_to_the_cap(lib, golden):
    """min(B, u x 256) before the upload: B below, at and above the cap; more units than recordings are never provided for."""
    p = golden["params"]
    for name, S in (("msnet321", 321), ("tonet361", 361), ("jdc722", 722)):
        A, pi = p[f"{name}_logA_T"], p[f"{name}_log_pi"]
        plan = _plan(lib, A, pi)
        cap = _units_per_cu(HostPlan(A, pi).W, S) * CUS
        for B in (0, 1, cap - 1, cap, cap + 1, 1 << 20):
            assert lib.vit_f64_packed_bounded_units(plan, B) == min(B, cap), (name, B)
        assert lib.vit_f64_packed_bounded_units(plan, -1) == 0 and lib.vit_f64_packed_bounded_units(None, 4) == 0
        lib.vit_plan_destroy(plan)
    assert _units_per_cu(128, 722) == 1 and _units_per_cu(16, 100) == 4 and _units_per_cu(32, 361) == 2 and _units_per_cu(64, 450) == 1


def test_zero_sizes_and_refused_plans(lib, golden):
    """0 for a NULL plan, NULL offsets, B < 0, a K outside [64, 2^24] and offsets that do not start at 0 or do not increase; size 0 and
    no units for the three kinds of plan the float64 family refuses, whose decode call answers VIT_ENOTUPLOADED first."""
    p = golden["params"]
    size, units = lib.vit_workspace_bytes_f64_packed_checkpointed, lib.vit_f64_packed_bounded_units
    off = _offsets((100, 70))
    assert size(None, 2, off.ctypes.data, 64) == 0
    plan = _plan(lib, p["tonet361_logA_T"], p["tonet361_log_pi"])
    assert size(plan, 2, off.ctypes.data, 64) > 0
    assert size(plan, 2, None, 64) == 0 and size(plan, -1, off.ctypes.data, 64) == 0
    assert size(plan, 2, off.ctypes.data, 63) == 0 and size(plan, 2, off.ctypes.data, (1 << 24) + 1) == 0 and size(plan, 2, off.ctypes.data, 0) == 0
    assert size(plan, 2, off.ctypes.data, 1 << 24) > 0
    for bad in ((1, 100, 170), (0, 100, 100), (0, 100, 90), (0, 0, 170)):
        o = np.asarray(bad, np.int64)
        assert size(plan, 2, o.ctypes.data, 64) == 0, bad
    lib.vit_plan_destroy(plan)
    A = np.array(p["tonet361_logA_T"])
    A[100, :] = -(np.arange(361) % 17).astype(np.float32) - 1                     # one dense row
    refused = (("unstructured", p["dense361_logA_T"], p["dense361_log_pi"]), ("Durrieu", p["durrieu722_logA_T"], p["durrieu722_log_pi"]),
               ("dense row", A, p["tonet361_log_pi"]))
    for what, A_, pi_ in refused:
        plan = _plan(lib, A_, pi_)
        if what == "dense row":
            hp = HostPlan(A_, pi_)
            assert hp.ok and hp.n_dense == 1, "premise: the plan holds a dense row"
        assert size(plan, 2, off.ctypes.data, 64) == 0, what
        assert units(plan, 2) == 0 and units(plan, 1 << 20) == 0, what
        dummy = ctypes.c_void_p(256 * 1024)
        assert lib.vit_decode_f64_packed_checkpointed(plan, dummy, 0, 2, off.ctypes.data, dummy, 1 << 20, dummy, None, 64, None) == -6, what
        lib.vit_plan_destroy(plan)


class _Stub:
    """the library seen by plan_workspace_f64_packed_bounded: the two size functions it asks, as pure functions of the frames"""

    def __init__(self, per_frame, per_segment_frame, fixed):
        self.per_frame, self.per_segment_frame, self.fixed, self.asked = per_frame, per_segment_frame, fixed, []

    def vit_workspace_bytes_f64_packed(self, plan, B, N):
        return self.fixed + self.per_frame * N

    def vit_workspace_bytes_f64_packed_checkpointed(self, plan, B, offsets, K):
        self.asked.append(K)
        return self.fixed + self.per_segment_frame * K


def test_budget_plan_through_a_stubbed_size_function(monkeypatch):
    """plan_workspace_f64_packed_bounded over ViterbiDecoder._plan_segments with the library's size functions stubbed (no plan, no
    device): "full" where the whole history fits or no budget is set, else the largest K of 8192 .. 64 that fits, asked from the
    largest down; ViterbiHipError below size(64); an empty batch needs nothing."""
    from viterbi_spl_amd import _lib
    stub = _Stub(per_frame=3000, per_segment_frame=700, fixed=5000)
    monkeypatch.setattr(_lib, "load", lambda: stub)
    dec = object.__new__(ViterbiDecoder)
    dec._plan, dec.S = None, 361
    off = _offsets((30000, 7500, 64, 65))
    full = 5000 + 3000 * 37629

    def size_of(K):
        return 5000 + 700 * K
    plan = dec.plan_workspace_f64_packed_bounded
    assert plan(off) == {"mode": "full", "workspace_bytes": full}
    assert plan(off, full) == {"mode": "full", "workspace_bytes": full} and plan(off, 10 ** 13) == {"mode": "full", "workspace_bytes": full}
    assert stub.asked == []
    K = 64
    while K <= 8192:
        for budget in (size_of(K), size_of(K) + 1, size_of(2 * K) - 1):
            assert plan(off, budget) == {"mode": "checkpointed", "segment_frames": K, "workspace_bytes": size_of(K)}, (K, budget)
        K *= 2
    assert plan(off, full - 1)["segment_frames"] == 8192                          # never above 8192, whatever would fit
    stub.asked.clear()
    plan(off, size_of(1024))
    assert stub.asked == [8192, 4096, 2048, 1024]
    with pytest.raises(ViterbiHipError):
        plan(off, size_of(64) - 1)
    assert plan(np.zeros(1, np.int64), 10) == {"mode": "full", "workspace_bytes": 0}
    stub.per_segment_frame, stub.fixed = 0, 0                                     # a plan the checkpointed decode does not serve
    with pytest.raises(ViterbiHipError):
        plan(off, 1000)
    with pytest.raises(ValueError):
        plan(np.asarray([0, 5, 5], np.int64), None)                               # an empty recording
