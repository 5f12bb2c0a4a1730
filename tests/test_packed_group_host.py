"""Host tier of the packed ragged decode for plans without the wave form (722-state grids): which plans
``vit_workspace_bytes_packed`` sizes, what it refuses, and that the wave-form plans' byte counts did not move.
No GPU: the library answers from the plan alone (256 compute units assumed until a plan is uploaded)."""
import ctypes
import os

import numpy as np
import pytest

from tests.plan_replay import HostPlan

GROUP_PLANS = ["jdc722", "jdc721", "imm722w", "durrieu722", "durrieu721"]


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


def _workgroup_stride(S):
    return (S + 2 + 3) // 4 * 4          # state i in column i, the frame maximum in column S, one scratch column, rows 16-byte aligned


@pytest.mark.parametrize("name", GROUP_PLANS)
def test_packed_workspace_exists_and_is_smaller_than_padding(lib, golden, name):
    """A size for every 722-state plan, at least the packed history with the workgroup row stride, and smaller than the padded
    decode's workspace for 64 recordings of 7500 .. 30000 frames (the memory that padding to the longest one costs)."""
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    plan = _plan(lib, A, pi)
    S = A.shape[0]
    SD = _workgroup_stride(S)
    B, T_max = 64, 30000
    lens = np.random.default_rng(5).integers(7500, T_max + 1, B)
    lens[0] = T_max
    N = int(lens.sum())
    packed = int(lib.vit_workspace_bytes_packed(plan, B, N))
    padded = int(lib.vit_workspace_bytes(plan, B, T_max))
    print(name, "packed", packed, "padded", padded, "ratio", packed / padded, "frames", N / (B * T_max))
    assert packed > 0
    assert packed >= N * SD * 4
    assert packed < padded
    for B1, N1 in ((1, 1), (15, 1500)):
        small = int(lib.vit_workspace_bytes_packed(plan, B1, N1))
        assert small >= N1 * SD * 4 and small > 0
    lib.vit_plan_destroy(plan)


def test_packed_workspace_still_refused(lib, golden):
    """Unstructured matrices and banded plans that only have the scan form get no packed decode: size 0."""
    p = golden["params"]
    plan = _plan(lib, p["dense97_logA_T"], p["dense97_log_pi"])
    assert int(lib.vit_workspace_bytes_packed(plan, 4, 400)) == 0
    lib.vit_plan_destroy(plan)
    # jdc722 with one in-window entry below its row's constant: still banded with the same window, but the floor form is not proven
    A = np.array(p["jdc722_logA_T"], np.float32, copy=True)
    base = HostPlan(A, p["jdc722_log_pi"])
    assert base.ok and base.floor_ok and base.W == 84 and not base.wave_ok
    vals, counts = np.unique(A[300], return_counts=True)
    const = np.float32(vals[np.argmax(counts)])                   # the row's constant: its most common value
    assert A[300, 303] != const, "the edited entry must lie inside the band"
    A[300, 303] = const - np.float32(5)
    hp = HostPlan(A, p["jdc722_log_pi"])
    assert hp.ok is True and hp.floor_ok is False and hp.W == 84 and hp.wave_ok is False
    plan = _plan(lib, A, p["jdc722_log_pi"])
    assert int(lib.vit_workspace_bytes_packed(plan, 4, 400)) == 0
    assert int(lib.vit_workspace_bytes(plan, 4, 100)) > 0          # the padded decode still serves it
    lib.vit_plan_destroy(plan)


# vit_workspace_bytes_packed of the wave-form plans as the parent commit (deb9c73) answers on the host, 256 compute units assumed
PARENT_BYTES = {
    "tonet361": {(1, 1): 2100992, (15, 1500): 4404480, (3072, 2300000): 3535287040},
    "msnet321": {(1, 1): 2100992, (15, 1500): 4404480, (3072, 2300000): 3535287040},
}


@pytest.mark.parametrize("name", sorted(PARENT_BYTES))
def test_wave_plans_keep_their_byte_count(lib, golden, name):
    plan = _plan(lib, golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"])
    for (B, N), want in PARENT_BYTES[name].items():
        assert int(lib.vit_workspace_bytes_packed(plan, B, N)) == want, (name, B, N)
    lib.vit_plan_destroy(plan)
