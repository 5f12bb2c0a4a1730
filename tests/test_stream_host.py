"""Host tier of the streaming decode (vit_stream_*): the symbols, what ``vit_workspace_bytes_stream`` answers from the plan alone and
the order in which ``vit_stream_open`` refuses.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

STREAM_SYMBOLS = ("vit_workspace_bytes_stream", "vit_stream_open", "vit_stream_append", "vit_stream_lengths", "vit_stream_backtrace",
                  "vit_stream_reset", "vit_stream_close")


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


def _golden_plan(lib, golden, name):
    return _plan(lib, golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"])


def _scan_only_banded():
    """tonet's band on 256 states: the floor kernel keeps the frame maximum in an idle target slot, and S = 64 * k leaves none, so this
    banded plan has the scan form only."""
    from viterbi_spl_amd import synth
    return synth.log_params(synth.tonet_transition(255, 14), synth.floored_prior(256))


def test_symbols_declared_and_exported(lib):
    from tests import test_abi
    from viterbi_spl_amd import _lib
    names = test_abi.declared_functions()
    for n in STREAM_SYMBOLS:
        assert n in names and n in _lib.EXPORTS and hasattr(lib, n), n
    assert set(names) == set(_lib.EXPORTS)
    assert lib.vit_abi_version() == _lib.ABI_VERSION == 4


@pytest.mark.parametrize("name", ["tonet361", "msnet321", "jdc722", "imm722w", "durrieu722"])
def test_workspace_bytes_served(lib, golden, name):
    plan = _golden_plan(lib, golden, name)
    S = int(golden["params"][f"{name}_logA_T"].shape[0])
    SD = (S + 5) // 4 * 4                      # the workgroup kernels' history row: 16-byte aligned, at least two pad columns
    for B, T in ((1, 1), (1, 30000), (3, 203), (16, 30000)):
        need = int(lib.vit_workspace_bytes_stream(plan, B, T))
        assert need >= B * T * SD * 4 and need % 256 == 0, (name, B, T, need)
        assert need <= B * T * SD * 4 + 256 + B * 2048 + 8 * 256, (name, B, T, need)     # tables and back-trace scratch: per song, not per frame
    assert int(lib.vit_workspace_bytes_stream(plan, 0, 100)) == 0
    assert int(lib.vit_workspace_bytes_stream(plan, -1, 100)) == 0
    assert int(lib.vit_workspace_bytes_stream(plan, 1, 0)) == 0
    lib.vit_plan_destroy(plan)


def test_workspace_bytes_refused(lib, golden):
    """NULL plan, and the kinds of plan without a stream instantiation: an unstructured matrix, a banded plan that only has the scan
    form (256 states: no idle target slot for the frame maximum), a banded plan with dense rows."""
    assert int(lib.vit_workspace_bytes_stream(None, 1, 100)) == 0
    from viterbi_spl_amd import _lib
    plans = {"dense361": _golden_plan(lib, golden, "dense361")}
    A, pi = _scan_only_banded()
    plans["scan256"] = _plan(lib, A, pi)
    A = np.array(golden["params"]["tonet361_logA_T"], np.float32)
    A[100, :] = -np.linspace(1.0, 9.0, 361, dtype=np.float32)       # one target row with no band structure: a dense row
    plans["dense_row"] = _plan(lib, A, golden["params"]["tonet361_log_pi"])
    info = _lib.PlanInfo()
    assert lib.vit_plan_query(plans["dense361"], ctypes.byref(info)) == 0 and info.banded_ok == 0
    assert lib.vit_plan_query(plans["scan256"], ctypes.byref(info)) == 0 and info.banded_ok == 1
    assert lib.vit_plan_query(plans["dense_row"], ctypes.byref(info)) == 0 and info.banded_ok == 1 and info.reserved[0] >= 1
    dummy = ctypes.c_void_p(256 * 1024)
    out = ctypes.c_void_p()
    for name, plan in plans.items():
        assert int(lib.vit_workspace_bytes_stream(plan, 2, 100)) == 0, name
        # not uploaded is answered before unsupported
        assert lib.vit_stream_open(plan, 2, 100, dummy, 1 << 30, ctypes.byref(out)) == -6, name
        assert not out.value
        lib.vit_plan_destroy(plan)


def test_open_status_order(lib, golden):
    plan = _golden_plan(lib, golden, "tonet361")
    dummy = ctypes.c_void_p(256 * 1024)
    out = ctypes.c_void_p()
    assert lib.vit_stream_open(None, 1, 10, dummy, 1 << 30, ctypes.byref(out)) == -1
    assert lib.vit_stream_open(plan, 1, 10, dummy, 1 << 30, None) == -1
    assert lib.vit_stream_open(plan, 0, 10, dummy, 1 << 30, ctypes.byref(out)) == -1
    assert lib.vit_stream_open(plan, 1, 0, dummy, 1 << 30, ctypes.byref(out)) == -1
    assert lib.vit_stream_open(plan, 1, 10, None, 1 << 30, ctypes.byref(out)) == -1
    assert lib.vit_stream_open(plan, 1, 10, ctypes.c_void_p(256 * 1024 + 64), 1 << 30, ctypes.byref(out)) == -1     # misaligned
    assert lib.vit_stream_open(plan, 1, 10, dummy, 1 << 30, ctypes.byref(out)) == -6                                # not uploaded
    assert lib.vit_stream_open(plan, 1, 10, dummy, 0, ctypes.byref(out)) == -6                                      # ... before the workspace size
    assert not out.value
    # NULL sessions
    assert lib.vit_stream_append(None, dummy, 0, 1, None, None) == -1
    assert lib.vit_stream_lengths(None, dummy) == -1
    assert lib.vit_stream_backtrace(None, dummy, 1, None, None) == -1
    assert lib.vit_stream_reset(None) == -1
    lib.vit_stream_close(None)
    lib.vit_plan_destroy(plan)
