"""CPU tier of the bounded-workspace float64 decode (vit_decode_f64_checkpointed): the exports, the size function on host-only plans and
the segment-length search that meets a workspace budget."""
import ctypes
import os

import numpy as np
import pytest

from tests.plan_replay import HostPlan
from viterbi_spl_amd import ViterbiDecoder
from viterbi_spl_amd._lib import ViterbiHipError


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
    for n in ("vit_workspace_bytes_f64_checkpointed", "vit_decode_f64_checkpointed"):
        assert n in declared_functions() and n in _lib.EXPORTS and hasattr(lib, n)
    assert lib.vit_abi_version() == 4
    assert lib.vit_workspace_bytes_f64_checkpointed.restype is ctypes.c_size_t
    assert lib.vit_decode_f64_checkpointed.restype is ctypes.c_int32
    assert len(lib.vit_workspace_bytes_f64_checkpointed.argtypes) == 4 and len(lib.vit_decode_f64_checkpointed.argtypes) == 12


def test_size_function_on_the_host(lib, golden):
    """Host-only plans of the 321-, 361- and 722-state bands: at least the checkpoint rows in front of segments 1 .. nseg - 1 and the
    segment's own rows, at most one checkpoint row and two segment rows more, 1 KB of tables per song and sixteen 256-byte
    round-ups; below the whole history from T = 4 K on; a K above T acts like T."""
    p = golden["params"]
    size = lib.vit_workspace_bytes_f64_checkpointed
    for name, S in (("msnet321", 321), ("tonet361", 361), ("jdc722", 722)):
        plan = _plan(lib, p[f"{name}_logA_T"], p[f"{name}_log_pi"])
        stride = (S + 3) // 2 * 2
        for B in (1, 3, 256):
            for T in (64, 65, 257, 30000):
                for K in (64, 65, 1024, 30000, 1 << 24):
                    Kc = min(K, T)
                    nseg = -(-T // Kc)
                    need = size(plan, B, T, K)
                    assert need >= B * (nseg - 1 + Kc) * stride * 8, (name, B, T, K, need)
                    assert need <= B * (nseg + Kc + 2) * stride * 8 + 1024 * B + 16 * 256, (name, B, T, K, need)
                    if T >= 4 * K:
                        assert need < lib.vit_workspace_bytes_f64(plan, B, T), (name, B, T, K)
                assert size(plan, B, T, 1 << 24) == size(plan, B, T, T)
        lib.vit_plan_destroy(plan)


def test_zero_sizes_and_refused_plans(lib, golden):
    """0 for a NULL plan, B < 0, T < 1 and a K outside [64, 2^24]; 0 for the three kinds of plan the float64 family refuses, whose
    decode call answers VIT_ENOTUPLOADED first, as vit_decode_f64_packed's does."""
    p = golden["params"]
    size = lib.vit_workspace_bytes_f64_checkpointed
    assert size(None, 1, 100, 64) == 0
    plan = _plan(lib, p["tonet361_logA_T"], p["tonet361_log_pi"])
    assert size(plan, 1, 100, 64) > 0 and size(plan, 0, 100, 64) == 0            # (no songs: nothing to keep, as vit_workspace_bytes_f64)
    assert size(plan, -1, 100, 64) == 0 and size(plan, 1, 0, 64) == 0 and size(plan, 1, -5, 64) == 0
    assert size(plan, 1, 100, 63) == 0 and size(plan, 1, 100, (1 << 24) + 1) == 0 and size(plan, 1, 100, 0) == 0
    assert size(plan, 1, 100, 1 << 24) > 0
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
        assert size(plan, 3, 100, 64) == 0, what
        dummy = ctypes.c_void_p(256 * 1024)
        assert lib.vit_decode_f64_checkpointed(plan, dummy, 0, 1, 100, None, dummy, 1 << 20, dummy, None, 64, None) == -6, what
        lib.vit_plan_destroy(plan)


def test_segment_search(lib, golden):
    """ViterbiDecoder._plan_segments as a pure function of (the whole need, a size callback, a budget): "full" when the whole history
    fits or no budget is set, else the largest fitting power of two in 64 .. 8192; ViterbiHipError below size(64).  Then the same
    on a host-only plan: no device is involved."""
    search = ViterbiDecoder._plan_segments

    def size_of(K):
        return 1000 + 40 * K
    full = size_of(30000)
    assert search(full, size_of, None) == {"mode": "full", "workspace_bytes": full}
    assert search(full, size_of, full) == {"mode": "full", "workspace_bytes": full}
    assert search(full, size_of, 10 ** 12) == {"mode": "full", "workspace_bytes": full}
    K = 64
    while K <= 8192:
        for budget in (size_of(K), size_of(K) + 1, size_of(2 * K) - 1):
            assert search(full, size_of, budget) == {"mode": "checkpointed", "segment_frames": K, "workspace_bytes": size_of(K)}, (K, budget)
        K *= 2
    assert search(full, size_of, full - 1)["segment_frames"] == 8192              # never above 8192, whatever would fit
    with pytest.raises(ViterbiHipError):
        search(full, size_of, size_of(64) - 1)
    with pytest.raises(ViterbiHipError):
        search(full, lambda K: 0, full - 1)                                       # a plan the checkpointed decode does not serve
    calls = []
    search(full, lambda K: calls.append(K) or size_of(K), size_of(1024))
    assert calls == [8192, 4096, 2048, 1024]                                      # from the largest down, stopping at the first fit

    p = golden["params"]
    plan = _plan(lib, p["jdc722_logA_T"], p["jdc722_log_pi"])
    B, T = 256, 30000
    whole = lib.vit_workspace_bytes_f64(plan, B, T)

    def ck(K):
        return lib.vit_workspace_bytes_f64_checkpointed(plan, B, T, K)
    got = search(whole, ck, whole // 8)
    assert got["mode"] == "checkpointed" and got["workspace_bytes"] == ck(got["segment_frames"]) <= whole // 8
    assert got["segment_frames"] == 8192 or ck(2 * got["segment_frames"]) > whole // 8
    assert ck(1024) < whole // 20                                                 # about 1.6 GB beside 44.5 GB
    lib.vit_plan_destroy(plan)
