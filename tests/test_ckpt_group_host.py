"""Host tier of the bounded-workspace decode for plans without the wave form (722-state grids): which plans
``vit_workspace_bytes_checkpointed`` sizes, how large the workspace is, what it refuses, and that the wave-form plans' byte
counts did not move.  No GPU: the library answers from the plan alone."""
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
def test_checkpointed_workspace_exists_and_is_bounded(lib, golden, name):
    """A size for every 722-state plan.  At [256, 30000, S] with segments of 1024 frames a song keeps 30 rows of pass 1 (29
    checkpoints + the scratch row) and the 1024 + 1 rows of the segment being walked, at most two more (the row in front of the
    segment, the row behind it), each of the workgroup stride; 1 MB covers the per-song arrays.  That is 1057 of 30000 rows: at
    most a sixteenth of the normal decode's workspace."""
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    plan = _plan(lib, A, pi)
    SD = _workgroup_stride(A.shape[0])
    B, T, K = 256, 30000, 1024
    need = int(lib.vit_workspace_bytes_checkpointed(plan, B, T, K))
    full = int(lib.vit_workspace_bytes(plan, B, T))
    print(name, "checkpointed", need, "full", full, "ratio", need / full)
    assert need > 0
    assert need >= B * (30 + 1025) * SD * 4
    assert need <= B * (30 + 1025 + 2) * SD * 4 + (1 << 20)
    assert 16 * need <= full
    for B1, T1, K1 in ((1, 1, 64), (3, 100, 4096)):
        assert int(lib.vit_workspace_bytes_checkpointed(plan, B1, T1, K1)) > 0
    lib.vit_plan_destroy(plan)


def test_checkpointed_workspace_still_refused(lib, golden):
    """Unstructured matrices, banded plans that only have the scan form, and segments shorter than 64 frames: size 0."""
    p = golden["params"]
    plan = _plan(lib, p["dense97_logA_T"], p["dense97_log_pi"])
    assert int(lib.vit_workspace_bytes_checkpointed(plan, 4, 400, 64)) == 0
    lib.vit_plan_destroy(plan)
    # jdc722 with one in-window entry below its row's constant: still banded with the same window, but the floor form is not proven
    A = np.array(p["jdc722_logA_T"], np.float32, copy=True)
    vals, counts = np.unique(A[300], return_counts=True)
    const = np.float32(vals[np.argmax(counts)])                   # the row's constant: its most common value
    assert A[300, 303] != const, "the edited entry must lie inside the band"
    A[300, 303] = const - np.float32(5)
    hp = HostPlan(A, p["jdc722_log_pi"])
    assert hp.ok is True and hp.floor_ok is False and hp.W == 84 and hp.wave_ok is False
    plan = _plan(lib, A, p["jdc722_log_pi"])
    assert int(lib.vit_workspace_bytes_checkpointed(plan, 4, 400, 64)) == 0
    assert int(lib.vit_workspace_bytes(plan, 4, 400)) > 0          # the normal decode still serves it
    lib.vit_plan_destroy(plan)
    for name in GROUP_PLANS + ["tonet361", "dense97"]:
        plan = _plan(lib, p[f"{name}_logA_T"], p[f"{name}_log_pi"])
        assert int(lib.vit_workspace_bytes_checkpointed(plan, 4, 400, 8)) == 0, name
        assert int(lib.vit_workspace_bytes_checkpointed(plan, 4, 400, (1 << 24) + 1)) == 0, name
        lib.vit_plan_destroy(plan)


# vit_workspace_bytes_checkpointed of the wave-form plans as a build of the parent commit (b7946c8) answers on the host
PARENT_BYTES = {
    "tonet361": {(256, 30000, 1024): 414945280, (9, 1000, 64): 1124096, (2048, 30000, 8192): 25786351616},
    "msnet321": {(256, 30000, 1024): 414945280, (9, 1000, 64): 1124096, (2048, 30000, 8192): 25786351616},
}


@pytest.mark.parametrize("name", sorted(PARENT_BYTES))
def test_wave_plans_keep_their_byte_count(lib, golden, name):
    plan = _plan(lib, golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"])
    for (B, T, K), want in PARENT_BYTES[name].items():
        assert int(lib.vit_workspace_bytes_checkpointed(plan, B, T, K)) == want, (name, B, T, K)
    lib.vit_plan_destroy(plan)
