"""Host tier of the commit point of a streaming session (vit_stream_commit*): the NumPy reference of its definition
(tests/commit_ref.py) against the oracle's paths, the symbols, what ``vit_workspace_bytes_stream_commit`` answers from the plan alone
and the refusals that need no device.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from oracle import viterbi_oracle as vo
from tests import commit_ref as cr
from viterbi_spl_amd import synth

COMMIT_SYMBOLS = ("vit_workspace_bytes_stream_commit", "vit_stream_commit_begin", "vit_stream_commit")
T = 203
SCHEDULE = [1] * 9 + [2, 3, 4, 5, 7, 8] + [40, 40, 40, 45]


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


@pytest.mark.parametrize("name", ["tonet361", "jdc722"])
@pytest.mark.parametrize("kind", ["peaks", "dense"])
def test_reference_prefix_is_final(golden, name, kind):
    """What the reference commits after n frames is the prefix of the oracle's path of those n frames AND of all 203: final.  The
    frontiers never decrease, with an unlimited and with a 32-frame lookback; the capped walk commits a prefix of the other."""
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    gen = synth.emissions_peaks if kind == "peaks" else synth.emissions_dense
    E = gen(2, T, A.shape[0], seed=21).numpy()
    whole, _ = vo.decode_c(A, pi, E)
    ns = np.cumsum(SCHEDULE)
    assert ns[-1] == T
    for b in range(2):
        psi = cr.back_pointers(A, pi, E[b])
        ends = {}
        for L in (1 << 20, 32):
            got = np.full(T, -5, np.int32)
            f_prev = 0
            for n, f, f2, st in cr.walk(psi, ns, L):
                assert f == f_prev and f <= f2 <= max(n - 1, 0) and len(st) == f2 - f, (name, kind, b, L, n)
                got[f:f2] = st
                f_prev = f2
                part, _ = vo.decode_c(A, pi, E[b:b + 1, :n])
                assert np.array_equal(got[:f2], part[0, :f2]), (name, kind, b, L, n)
                assert np.array_equal(got[:f2], whole[b, :f2]), (name, kind, b, L, n)
                assert (got[f2:] == -5).all()
            ends[L] = f_prev
        assert ends[32] <= ends[1 << 20] and ends[1 << 20] >= 150, (name, kind, b, ends)
        if kind == "peaks":
            assert ends[1 << 20] >= 190, (name, b, ends)


def test_reference_edges():
    """n < 2 commits nothing; a lookback of 1 only ever looks at frame n - 2; a frontier at n - 1 leaves nothing to walk."""
    psi = np.zeros((5, 3), np.int32)
    psi[1:] = [1, 1, 1]                              # every state comes from state 1
    assert cr.commit(psi, 0, 0, 8)[0] == 0 and cr.commit(psi, 1, 0, 8)[0] == 0
    f, st = cr.commit(psi, 5, 0, 1)
    assert f == 4 and st.tolist() == [1, 1, 1, 1]
    f, st = cr.commit(psi, 5, 2, 8)
    assert f == 4 and st.tolist() == [1, 1]
    f, st = cr.commit(psi, 5, 4, 8)
    assert f == 4 and len(st) == 0
    psi2 = np.tile(np.arange(3, dtype=np.int32), (5, 1))     # every state comes from itself: the survivors never merge
    assert cr.commit(psi2, 5, 0, 8)[0] == 0


def test_symbols_declared_and_exported(lib):
    from tests import test_abi
    from viterbi_spl_amd import _lib
    names = test_abi.declared_functions()
    for n in COMMIT_SYMBOLS:
        assert n in names and n in _lib.EXPORTS and hasattr(lib, n), n
    assert set(names) == set(_lib.EXPORTS)
    assert lib.vit_abi_version() == _lib.ABI_VERSION == 4


@pytest.mark.parametrize("name", ["tonet361", "msnet321", "jdc722", "imm722w"])
def test_commit_bytes_served(lib, golden, name):
    """Per recording, not per frame: four int64 tables and one int32 table of B entries, 8 words of chunk flags and 256 chunk entries
    per recording, each table rounded up to 256 bytes."""
    plan = _plan(lib, golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"])
    for B in (1, 3, 16, 33):
        need = int(lib.vit_workspace_bytes_stream_commit(plan, B))
        per = 4 * 8 + 4 + 8 * 4 + 256 * 4
        assert need >= per * B and need % 256 == 0 and need <= per * B + 7 * 255, (name, B, need)
    assert int(lib.vit_workspace_bytes_stream_commit(plan, 0)) == 0
    assert int(lib.vit_workspace_bytes_stream_commit(plan, -1)) == 0
    lib.vit_plan_destroy(plan)


def test_commit_bytes_refused(lib, golden):
    """NULL plan; a step plan (Durrieu: a session is served, a commit is not); an unstructured matrix."""
    assert int(lib.vit_workspace_bytes_stream_commit(None, 2)) == 0
    for name in ("durrieu722", "dense361"):
        plan = _plan(lib, golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"])
        assert int(lib.vit_workspace_bytes_stream_commit(plan, 2)) == 0, name
        assert (int(lib.vit_workspace_bytes_stream(plan, 2, 100)) > 0) == (name == "durrieu722")
        lib.vit_plan_destroy(plan)


def test_status_without_a_session(lib):
    dummy = ctypes.c_void_p(256 * 1024)
    assert lib.vit_stream_commit_begin(None, dummy, 1 << 20) == -1
    assert lib.vit_stream_commit_begin(None, None, 1 << 20) == -1
    assert lib.vit_stream_commit(None, dummy, 10, dummy, 8, None) == -1
    assert lib.vit_stream_commit(None, None, 10, None, 0, None) == -1
