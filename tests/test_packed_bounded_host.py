"""Host tier of the bounded packed decode (vit_decode_packed_bounded): what ``vit_workspace_bytes_packed_bounded`` and
``vit_packed_bounded_units`` answer from the plan and the offsets alone.  No GPU.  A plan that was never uploaded assumes 256
compute units, so the sizes here are those of a 256-unit device; the device that runs is checked in tests/test_gpu_packed_bounded.py."""
import ctypes
import os

import numpy as np
import pytest

N_CUS = 256          # a plan that was never uploaded (csrc/capi.hip vit_plan::n_cus)
FLOOR_PLANS = ["jdc722", "jdc721", "imm722w"]
STEP_PLANS = ["durrieu722", "durrieu721"]
U_PER_CU = {**{n: 1 for n in FLOOR_PLANS}, **{n: 2 for n in STEP_PLANS}}      # units per compute unit and launch (include/viterbi_hip.h)
EXTRA_ROWS = {**{n: 2 for n in FLOOR_PLANS}, **{n: 1 for n in STEP_PLANS}}    # rows a unit holds besides its K


@pytest.fixture(scope="module")
def lib():
    from viterbi_spl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _plan(lib, A, pi):
    A = np.ascontiguousarray(A, np.float32)
    pi = np.ascontiguousarray(pi, np.float32)
    plan = ctypes.c_void_p()
    assert lib.vit_plan_create(A.ctypes.data, pi.ctypes.data, A.shape[0], ctypes.byref(plan)) == 0
    return plan


def _named(lib, golden, name):
    return _plan(lib, golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"])


def _off(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)


def _need(lib, plan, lens, K):
    off = _off(lens)
    return int(lib.vit_workspace_bytes_packed_bounded(plan, len(lens), off.ctypes.data, K))


def _scan_only_jdc722(golden):
    """jdc722 with one in-window entry below its row's constant (tests/test_gpu_ckpt_group.py): banded, the floor form not proven."""
    A = np.array(golden["params"]["jdc722_logA_T"], np.float32, copy=True)
    vals, counts = np.unique(A[300], return_counts=True)
    A[300, 303] = np.float32(vals[np.argmax(counts)]) - np.float32(5)
    return A, golden["params"]["jdc722_log_pi"]


def _set_401():
    """The 401-recording / 7.68 M-frame set of DESIGN.md 4.6 (scripts/packed_group_time.py): lengths uniform in [7500, 30000]."""
    rng = np.random.default_rng(7)
    lens, left = [], 256 * 30000
    while left > 0:
        n = min(int(rng.integers(7500, 30001)), left)
        lens.append(n)
        left -= n
    assert len(lens) == 401
    return np.asarray(lens, np.int64)


@pytest.mark.parametrize("name", FLOOR_PLANS + STEP_PLANS)
def test_workspace_formula(lib, golden, name):
    """units x (K + 2 | K + 1) segment rows + sum (n_b - 1) checkpoint rows + one scratch row per pass-1 slot, hist_stride(S) =
    (S + 5) / 4 * 4 floats each, plus the tables of the packed checkpointed decode (per song two 8-byte and two 4-byte entries, per
    unit two 4-byte entries, per unit of a launch 20 + 128 bytes, a 4-byte slot bound per slot, the 256-byte roundings); units is
    what vit_packed_bounded_units answers, min(B, u x 256).  At K = 1024 the 401-recording set stays below a tenth of the full history."""
    plan = _named(lib, golden, name)
    S = golden["params"][f"{name}_logA_T"].shape[0]
    sd = (S + 5) // 4 * 4
    rng = np.random.default_rng(5)
    for lens, K in ((_set_401(), 1024), (rng.integers(1, 3000, 700), 64), ([1, 2, 63, 64, 65, 700], 64), ([50, 60], 4096), ([1], 64)):
        lens = np.asarray(lens, np.int64)
        B = len(lens)
        Kc = min(K, int(lens.max()))
        nseg = (lens + Kc - 1) // Kc
        units = int(lib.vit_packed_bounded_units(plan, B))
        assert units == min(B, U_PER_CU[name] * N_CUS) > 0
        n_slots = min(B, 8 * N_CUS)
        rows = units * (Kc + EXTRA_ROWS[name]) + int((nseg - 1).sum()) + n_slots
        need = _need(lib, plan, lens, K)
        print(name, B, K, "bounded", need, "full", int(lib.vit_workspace_bytes_packed(plan, B, int(lens.sum()))))
        assert need >= rows * sd * 4
        assert need <= rows * sd * 4 + 24 * B + 8 * int(nseg.sum()) + 148 * units + 4 * n_slots + 16 * 256
    lens = _set_401()
    full = int(lib.vit_workspace_bytes_packed(plan, 401, int(lens.sum())))
    assert full > 22e9 and 0 < 10 * _need(lib, plan, lens, 1024) <= full
    assert int(lib.vit_packed_bounded_units(plan, 1 << 20)) == U_PER_CU[name] * N_CUS and int(lib.vit_packed_bounded_units(plan, 0)) == 0
    lib.vit_plan_destroy(plan)


@pytest.mark.parametrize("name", ["tonet361", "msnet321"])
def test_wave_form_plans_forward(lib, golden, name):
    """Plans with the wave form get the size of vit_workspace_bytes_packed_checkpointed, and its eight units per compute unit."""
    plan = _named(lib, golden, name)
    rng = np.random.default_rng(9)
    for lens in (rng.integers(7500, 30001, 3250), rng.integers(1, 3000, 100), [1, 2, 63, 64, 65, 700], [50, 60]):
        off = _off(lens)
        for K in (64, 100, 1024, 1 << 24):
            want = int(lib.vit_workspace_bytes_packed_checkpointed(plan, len(lens), off.ctypes.data, K))
            assert want > 0 and _need(lib, plan, lens, K) == want, (name, len(lens), K)
        assert int(lib.vit_packed_bounded_units(plan, len(lens))) == min(len(lens), 8 * N_CUS)
    lib.vit_plan_destroy(plan)


def test_refusals(lib, golden):
    """Size 0 and 0 units for an unstructured matrix and a scan-only banded plan; size 0 for a segment length out of range, bad
    offsets and null arguments; a decode before the upload is refused, not executed."""
    lens = [100, 700, 65]
    for plan in (_named(lib, golden, "dense97"), _plan(lib, *_scan_only_jdc722(golden))):
        assert _need(lib, plan, lens, 64) == 0
        assert int(lib.vit_packed_bounded_units(plan, 3)) == 0
        lib.vit_plan_destroy(plan)
    assert int(lib.vit_packed_bounded_units(None, 3)) == 0
    for name in ("jdc722", "durrieu722", "tonet361"):
        plan = _named(lib, golden, name)
        assert _need(lib, plan, lens, 64) > 0
        assert _need(lib, plan, lens, 63) == 0 and _need(lib, plan, lens, (1 << 24) + 1) == 0 and _need(lib, plan, lens, 1 << 24) > 0
        for bad in ([1, 20, 50], [0, 20, 20], [0, 30, 20]):
            off = np.asarray(bad, np.int64)
            assert int(lib.vit_workspace_bytes_packed_bounded(plan, 2, off.ctypes.data, 64)) == 0, (name, bad)
        assert int(lib.vit_workspace_bytes_packed_bounded(plan, 2, None, 64)) == 0
        off = np.asarray([0, 20, 50], np.int64)
        assert int(lib.vit_workspace_bytes_packed_bounded(None, 2, off.ctypes.data, 64)) == 0
        assert int(lib.vit_workspace_bytes_packed_bounded(plan, -1, off.ctypes.data, 64)) == 0
        assert int(lib.vit_packed_bounded_units(plan, -1)) == 0
        dummy = ctypes.c_void_p(256 * 1024)
        assert lib.vit_decode_packed_bounded(plan, dummy, 0, 2, off.ctypes.data, dummy, 1 << 30, dummy, None, 64, None) == -6
        lib.vit_plan_destroy(plan)


def test_old_entry_points_keep_refusing(lib, golden):
    """The packed checkpointed entry points keep their answer for plans without the wave form: size 0."""
    off = _off([100, 700, 65])
    for name in FLOOR_PLANS + STEP_PLANS:
        plan = _named(lib, golden, name)
        assert int(lib.vit_workspace_bytes_packed_checkpointed(plan, 3, off.ctypes.data, 64)) == 0, name
        lib.vit_plan_destroy(plan)


def test_exports_are_declared():
    """tests/test_abi.py compares the header with the loader's list; both carry the three new entry points, the ABI version stays 4."""
    from tests import test_abi
    from viterbi_spl_amd import _lib
    names = test_abi.declared_functions()
    for n in ("vit_workspace_bytes_packed_bounded", "vit_decode_packed_bounded", "vit_packed_bounded_units"):
        assert n in names and n in _lib.EXPORTS
    assert set(names) == set(_lib.EXPORTS) and _lib.ABI_VERSION == 4
