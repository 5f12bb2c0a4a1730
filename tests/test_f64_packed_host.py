"""CPU tier of the packed ragged float64 decode (vit_decode_f64_packed): the exports, the size function on host-only plans and the
greedy grouping that meets a workspace budget."""
import ctypes
import os

import numpy as np
import pytest

from tests.plan_replay import HostPlan
from viterbi_spl_amd import ViterbiDecoder


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


def test_header_loader_and_exports_agree(lib):
    from tests.test_abi import declared_functions
    from viterbi_spl_amd import _lib
    for n in ("vit_workspace_bytes_f64_packed", "vit_decode_f64_packed"):
        assert n in declared_functions() and n in _lib.EXPORTS and hasattr(lib, n)
    assert lib.vit_abi_version() == 4
    assert lib.vit_workspace_bytes_f64_packed.restype is ctypes.c_size_t
    assert lib.vit_decode_f64_packed.restype is ctypes.c_int32
    assert len(lib.vit_decode_f64_packed.argtypes) == 10 and len(lib.vit_workspace_bytes_f64_packed.argtypes) == 3
    import viterbi_spl_amd
    assert callable(viterbi_spl_amd.viterbi_librosa_f64_recordings_fn)


def test_size_function_on_the_host(lib, golden):
    """Host-only plans of the 321-, 361- and 722-state bands: the history of doubles fits; what is left beside it does not depend on
    the frame count and grows at most linearly in the recordings -- 32 bytes each (a terminal state, a chunk entry, an offset, a slot
    boundary, a slot entry, a wave entry, a chunk base) and at most one 256-byte round-up for each of the seven tables; 0 for a NULL
    plan, negative arguments and the three refused kinds of plan."""
    p = golden["params"]
    size = lib.vit_workspace_bytes_f64_packed
    assert size(None, 1, 10) == 0
    for name, S in (("msnet321", 321), ("tonet361", 361), ("jdc722", 722)):
        plan = _plan(lib, p[f"{name}_logA_T"], p[f"{name}_log_pi"])
        stride = (S + 3) // 2 * 2
        rest0 = size(plan, 0, 0)
        assert rest0 > 0
        for B in (1, 3, 401, 3250, 100000):
            rest = None
            for N in (B, B + 1, 7 * B + 5, 30000 * B, 61000000):
                need = size(plan, B, N)
                assert N * stride * 8 <= need, (name, B, N)
                rest = need - N * stride * 8 if rest is None else rest
                assert need - N * stride * 8 == rest, (name, B, N)
            assert rest0 <= rest <= rest0 + 32 * B + 7 * 256, (name, B, rest, rest0)
        assert size(plan, -1, 10) == 0 and size(plan, 1, -1) == 0
        lib.vit_plan_destroy(plan)
    A = np.array(p["tonet361_logA_T"])
    A[100, :] = -(np.arange(361) % 17).astype(np.float32) - 1                     # one dense row
    refused = (("unstructured", p["dense361_logA_T"], p["dense361_log_pi"]), ("Durrieu", p["durrieu722_logA_T"], p["durrieu722_log_pi"]),
               ("dense row", A, p["tonet361_log_pi"]))
    off = np.asarray([0, 10], np.int64)
    for what, A_, pi_ in refused:
        plan = _plan(lib, A_, pi_)
        if what == "dense row":
            hp = HostPlan(A_, pi_)
            assert hp.ok and hp.n_dense == 1, "premise: the plan holds a dense row"
        assert size(plan, 3, 100) == 0, what
        # refused before anything else is looked at but the arguments: not uploaded comes first, as in vit_decode_packed
        dummy = ctypes.c_void_p(256 * 1024)
        assert lib.vit_decode_f64_packed(plan, dummy, 0, 1, off.ctypes.data, dummy, 1 << 20, dummy, None, None) == -6, what
        lib.vit_plan_destroy(plan)


def _check_groups(offsets, size_of, budget, groups):
    B = len(offsets) - 1
    assert groups[0][0] == 0 and groups[-1][1] == B
    for k, (b0, b1) in enumerate(groups):
        assert b0 < b1 and (k == 0 or groups[k - 1][1] == b0)                          # consecutive, none empty, every recording covered
        assert size_of(b1 - b0, offsets[b1] - offsets[b0]) <= budget                    # each fits
        if b1 < B:
            assert size_of(b1 + 1 - b0, offsets[b1 + 1] - offsets[b0]) > budget         # and could not take the next recording


def test_greedy_groups():
    """ViterbiDecoder._greedy_groups as a pure function of (offsets, size_of, budget)."""
    def size_of(B, N):
        return 1000 + 40 * B + 8 * N
    rng = np.random.default_rng(5)
    for trial in range(20):
        lens = rng.integers(1, 400, size=int(rng.integers(1, 40)))
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        one = max(size_of(1, int(n)) for n in lens)
        for budget in (one, one + 1, 2 * one, 5 * one + 13, size_of(len(lens), int(off[-1])), 10 ** 9):
            groups = ViterbiDecoder._greedy_groups(off, size_of, budget)
            _check_groups([int(x) for x in off], size_of, budget, groups)
            if budget >= size_of(len(lens), int(off[-1])):
                assert groups == [(0, len(lens))]
        with pytest.raises(ValueError):
            ViterbiDecoder._greedy_groups(off, size_of, one - 1)
    assert ViterbiDecoder._greedy_groups([0, 5, 6, 16], size_of, size_of(2, 11)) == [(0, 2), (2, 3)]
    assert ViterbiDecoder._greedy_groups([0], size_of, 1) == []
