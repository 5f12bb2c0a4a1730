"""CPU tier of the float64-accumulating decode (vit_decode_f64): the NumPy restatement of the reference's float64 function against
the reference's own committed outputs, the float64 floor form replayed from the plan's tables against the restatement, and the
host-only entry points."""
import ctypes
import os

import numpy as np
import pytest

from tests import common, f64_ref
from tests.plan_replay import HostPlan
from viterbi_spl_amd import synth


def test_restatement_equals_the_reference_outputs(golden):
    """The four f64 cases of the golden manifest (T = 500, 4000, 30000, 30000 on the msnet parameters): the restatement returns the
    reference's float64 path on every frame, and differs from the reference's float32 path in exactly the manifest's frames."""
    cases = golden["manifest"]["f64_cases"]
    assert [c["T"] for c in cases] == [500, 4000, 30000, 30000]
    for c in cases:
        k = c["index"]
        assert common.sha(f64_ref.manifest_case_probs(c)) == c["sha256"]
        logA_T, log_pi, logE = f64_ref.manifest_log_inputs(golden, c)
        states, _ = f64_ref.decode_f64(logA_T, log_pi, logE)
        s64 = golden["data"][f"f64_{k}_states64"].astype(np.int64)
        s32 = golden["data"][f"f64_{k}_states32"].astype(np.int64)
        assert np.array_equal(states, s64), (c, int(np.sum(states != s64)))
        assert int(np.sum(states != s32)) == c["differing_frames"], c
    assert [c["differing_frames"] for c in cases] == [0, 0, 1157, 204]


SHIPPED = ("msnet321", "tonet361", "jdc722")


def _matrices(golden):
    for name in SHIPPED:
        A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
        yield name, A, pi
        yield name + "_inf", common.inf_floor_sibling(A), pi


def _same(plan_A, plan_pi, E):
    """restatement == float64 floor replay of the plan's tables: states, log-likelihood and every d row by bit pattern"""
    plan = HostPlan(plan_A, plan_pi)
    assert plan.ok and plan.floor_ok and plan.n_dense == 0
    rs, rd, rrows = f64_ref.decode_f64(plan_A, plan_pi, E, all_rows=True)
    ps, pl, prows = f64_ref.replay_floor_f64(plan, E)
    assert np.array_equal(ps, rs)
    assert f64_ref.bits64(pl) == f64_ref.bits64(rd[rs[-1]])
    assert np.array_equal(f64_ref.bits64(prows), f64_ref.bits64(rrows))
    return rs, rd


@pytest.mark.parametrize("name", [n for s in SHIPPED for n in (s, s + "_inf")])
def test_floor_form_replay_equals_the_restatement(golden, name):
    """The float64 floor form -- window, row constant with M over the non-extra sources, extra columns, the lazy back-trace with its
    bound -- driven by the plan's own tables equals the dense float64 recursion: the shipped 321- / 361- / 722-state matrices and
    their -inf floor siblings; i.i.d., all-tie and the value-edge emissions."""
    A, pi = dict((n, (a, p)) for n, a, p in _matrices(golden))[name]
    S = A.shape[0]
    T = 300 if S < 700 else 120
    for kind in ("dense", "ties"):
        E = common.GEN[kind](1, T, S, seed=5 + S)[0].numpy()
        _same(A, pi, E)
    # every candidate ties: the sums absorb every matrix entry; the path is state 0 throughout
    rs, _ = _same(A, pi, np.full((40, S), -1e30, np.float32))
    assert np.all(rs == 0)
    rs, rd = _same(A, pi, np.full((40, S), -np.inf, np.float32))
    assert np.all(rs == 0) and np.isneginf(rd[0])
    half = {321: 12, 361: 14, 722: 40}[S]
    for cname, A2, pi2, E32, _, lens, _, _ in common.edge_cases(17, A, pi, 70, half=half):
        for b in (0, 6, 9):
            _same(A2, pi2, E32[b, :int(lens[b])])


@pytest.fixture(scope="module")
def lib():
    from viterbi_spl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_header_loader_and_exports_agree(lib):
    from tests.test_abi import declared_functions
    from viterbi_spl_amd import _lib
    for n in ("vit_workspace_bytes_f64", "vit_decode_f64"):
        assert n in declared_functions() and n in _lib.EXPORTS and hasattr(lib, n)
    assert lib.vit_abi_version() == 4
    assert lib.vit_workspace_bytes_f64.restype is ctypes.c_size_t
    assert len(lib.vit_decode_f64.argtypes) == 11


def _plan(lib, A, pi):
    A, pi = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(pi, np.float32)
    plan = ctypes.c_void_p()
    assert lib.vit_plan_create(A.ctypes.data, pi.ctypes.data, A.shape[0], ctypes.byref(plan)) == 0
    return plan


def test_size_function_serves_and_refuses_on_the_host(lib, golden):
    """Host-only calls: 0 for a NULL plan and for an unstructured, a Durrieu and a dense-row plan; the history of doubles otherwise."""
    p = golden["params"]
    assert lib.vit_workspace_bytes_f64(None, 1, 10) == 0
    for name, S in (("msnet321", 321), ("tonet361", 361), ("jdc722", 722), ("imm722w", 722), ("jdc721", 721)):
        plan = _plan(lib, p[f"{name}_logA_T"], p[f"{name}_log_pi"])
        need = lib.vit_workspace_bytes_f64(plan, 3, 100)
        assert need >= 3 * 100 * (S + 1) * 8 and need % 256 == 0, name
        assert need <= 3 * 100 * (S + 3) * 8 + 3 * 256 + 3 * 33 * 4 + 1024, name
        assert lib.vit_workspace_bytes_f64(plan, 0, 100) < 1024
        assert lib.vit_workspace_bytes_f64(plan, 3, 0) == 0 and lib.vit_workspace_bytes_f64(plan, -1, 10) == 0
        lib.vit_plan_destroy(plan)
    # a banded matrix with one dense row (a target that every source reaches with its own weight)
    A = np.array(p["tonet361_logA_T"])
    A[100, :] = -(np.arange(361) % 17).astype(np.float32) - 1
    refused = (("unstructured", p["dense361_logA_T"], p["dense361_log_pi"]), ("Durrieu", p["durrieu722_logA_T"], p["durrieu722_log_pi"]),
               ("dense row", A, p["tonet361_log_pi"]))
    for what, A_, pi_ in refused:
        plan = _plan(lib, A_, pi_)
        if what == "dense row":
            hp = HostPlan(A_, pi_)
            assert hp.ok and hp.n_dense == 1, "premise: the plan holds a dense row"
        assert lib.vit_workspace_bytes_f64(plan, 3, 100) == 0, what
        # refused before anything else is looked at but the arguments: not uploaded comes first, as in vit_decode
        dummy = ctypes.c_void_p(256 * 1024)
        assert lib.vit_decode_f64(plan, dummy, 0, 1, 10, None, dummy, 1 << 20, dummy, None, None) == -6, what
        lib.vit_plan_destroy(plan)
