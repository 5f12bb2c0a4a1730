"""Host tier of the packed checkpointed decode (vit_decode_packed_checkpointed): the launch schedule of pass 2, reached through the
host-only plan library, and what ``vit_workspace_bytes_packed_checkpointed`` answers from the plan and the offsets alone.  No GPU.
The size uses the compute-unit count of the device a plan was uploaded to; a plan that was never uploaded assumes 256, so the
sizes here are those of a 256-unit device and the sizes of the device that runs are checked in tests/test_gpu_packed_ckpt.py."""
import ctypes
import os

import numpy as np
import pytest

from tests import plan_replay

N_CUS = 256          # a plan that was never uploaded (csrc/capi.hip vit_plan::n_cus)
SDW = 384            # history row of the wave form: 64 * ceil(S / 64) floats, S = 321 and S = 361


@pytest.fixture(scope="module")
def host():
    plan_replay._lib()                                   # builds the host library where it is missing
    lib = ctypes.CDLL(plan_replay.LIB)
    lib.vph_packed_ckpt_schedule.restype = ctypes.c_longlong
    lib.vph_packed_ckpt_schedule.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def lib():
    from viterbi_spl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _schedule(host, lens, K, max_units):
    """-> list of launches, each a list of (song, segment), and ckpt_base [B + 1]."""
    lens = np.asarray(lens, np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    B = len(lens)
    units = int(((lens + K - 1) // K).sum())
    song, seg = np.full(units, -7, np.int32), np.full(units, -7, np.int32)
    begin, base = np.full(units + 2, -7, np.int64), np.full(B + 1, -7, np.int64)
    nl = host.vph_packed_ckpt_schedule(off.ctypes.data, B, K, max_units, song.ctypes.data, seg.ctypes.data, units, begin.ctypes.data,
                                       units + 1, base.ctypes.data)
    assert nl >= 0
    assert begin[0] == 0 and begin[nl] == units and (np.diff(begin[:nl + 1]) >= 1).all()
    return [list(zip(song[begin[l]:begin[l + 1]].tolist(), seg[begin[l]:begin[l + 1]].tolist())) for l in range(nl)], base


def _check_schedule(lens, K, max_units, launches, base):
    lens = np.asarray(lens, np.int64)
    nseg = (lens + K - 1) // K
    assert np.array_equal(base, np.concatenate([[0], np.cumsum(nseg - 1)]))       # the checkpoint rows in front of each song's
    seen = {}
    for l, launch in enumerate(launches):
        assert 1 <= len(launch) <= max_units, (l, len(launch))
        songs = [b for b, _ in launch]
        assert len(set(songs)) == len(songs), f"launch {l} holds two units of one song"
        for b, s in launch:
            assert 0 <= b < len(lens) and 0 <= s < nseg[b]
            # descending segment order across launches: the first unit of a song is its last segment, then one lower each time
            assert s == seen.get(b, nseg[b]) - 1, (l, b, s)
            seen[b] = s
    assert sorted(seen) == list(range(len(lens))) and all(v == 0 for v in seen.values())     # every unit exactly once
    # the launch count of the greedy rule: no more than the longest song's segments or the units over the launch size ask for
    assert len(launches) == max(int(nseg.max()), -(-int(nseg.sum()) // max_units)), (len(launches), int(nseg.max()), int(nseg.sum()))


@pytest.mark.parametrize("seed", range(6))
def test_schedule_for_random_offsets(host, seed):
    rng = np.random.default_rng(100 + seed)
    B = int(rng.integers(1, 400))
    K = int(rng.choice([64, 100, 128, 1024]))
    lens = rng.integers(1, 40 * K, B)
    lens[rng.integers(0, B, 3)] = (1, K, K + 1)
    if seed % 2:
        lens[int(rng.integers(0, B))] = 300 * K             # one song far longer than the rest: it bounds the launch count
    for max_units in (1, 7, 64, B, 2048):
        launches, base = _schedule(host, lens, K, max_units)
        _check_schedule(lens, K, max_units, launches, base)


def test_schedule_edges(host):
    for lens, K, mu in (([1], 64, 2048), ([64], 64, 1), ([65], 64, 1), ([1, 2, 63, 64, 65, 127, 128, 129, 193, 700, 1], 64, 4),
                        ([1, 2, 63, 64, 65, 127, 128, 129, 193, 700, 1], 4096, 2048), ([700] * 5, 64, 3)):
        launches, base = _schedule(host, lens, K, mu)
        _check_schedule(lens, K, mu, launches, base)
    # the songs with the most segments left go first, ties to the lowest song
    launches, _ = _schedule(host, [130, 700, 64, 700], 64, 2)
    assert launches[0] == [(1, 10), (3, 10)] and launches[1] == [(1, 9), (3, 9)]
    assert launches[8] == [(0, 2), (1, 2)]                 # three songs with three segments left: the two lowest
    # bad offsets are refused
    off = np.asarray([0, 5, 5], np.int64)
    buf = np.zeros(64, np.int64)
    assert host.vph_packed_ckpt_schedule(off.ctypes.data, 2, 64, 8, buf.ctypes.data, buf.ctypes.data, 8, buf.ctypes.data, 8, buf.ctypes.data) == -1


def _plan(lib, A, pi):
    A = np.ascontiguousarray(A, np.float32)
    pi = np.ascontiguousarray(pi, np.float32)
    plan = ctypes.c_void_p()
    assert lib.vit_plan_create(A.ctypes.data, pi.ctypes.data, A.shape[0], ctypes.byref(plan)) == 0
    return plan


def _need(lib, plan, lens, K):
    off = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)
    return int(lib.vit_workspace_bytes_packed_checkpointed(plan, len(lens), off.ctypes.data, K))


@pytest.mark.parametrize("name", ["tonet361", "msnet321"])
def test_workspace_formula(lib, golden, name):
    """n_units x (K + 1) segment rows + sum (n_b - 1) checkpoint rows + one scratch row per pass-1 wavefront, 384 floats each, plus
    tables: per song two 8-byte and two 4-byte entries, per unit two 4-byte entries, per unit of a launch 20 + 128 bytes of
    per-launch arrays and a 4-byte slot bound, and the 256-byte roundings.  The README's workload (3250 recordings, 61.44 M frames) at K = 1024 stays below 3.4 GB -- the full history
    takes 94 GB."""
    plan = _plan(lib, golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"])
    rng = np.random.default_rng(5)
    for lens, K in ((rng.integers(7500, 30001, 3250), 1024), (rng.integers(1, 3000, 100), 64), ([1, 2, 63, 64, 65, 700], 64), ([50, 60], 4096)):
        lens = np.asarray(lens, np.int64)
        Kc = min(K, int(lens.max()))
        nseg = (lens + Kc - 1) // Kc
        n_units = min(len(lens), 8 * N_CUS)
        rows = n_units * (Kc + 1) + int((nseg - 1).sum()) + n_units
        need = _need(lib, plan, lens, K)
        full = int(lib.vit_workspace_bytes_packed(plan, len(lens), int(lens.sum())))
        print(name, len(lens), K, "checkpointed", need, "full", full)
        assert need >= rows * SDW * 4
        assert need <= rows * SDW * 4 + 24 * len(lens) + 8 * int(nseg.sum()) + 152 * n_units + 16 * 256
    lens = rng.integers(7500, 30001, 3250)
    assert _need(lib, plan, lens, 1024) < 3.4e9 < 20 * 3.4e9 < int(lib.vit_workspace_bytes_packed(plan, 3250, int(lens.sum())))
    lib.vit_plan_destroy(plan)


def test_workspace_refusals(lib, golden):
    """Size 0 for every plan without the wave form (the 722-state floor and step plans, an unstructured matrix), for a segment
    length out of range, for bad offsets and for null arguments."""
    p = golden["params"]
    lens = [100, 700, 65]
    for name in ("jdc722", "imm722w", "durrieu722", "dense97"):
        plan = _plan(lib, p[f"{name}_logA_T"], p[f"{name}_log_pi"])
        assert _need(lib, plan, lens, 64) == 0, name
        lib.vit_plan_destroy(plan)
    plan = _plan(lib, p["tonet361_logA_T"], p["tonet361_log_pi"])
    assert _need(lib, plan, lens, 64) > 0
    assert _need(lib, plan, lens, 63) == 0 and _need(lib, plan, lens, (1 << 24) + 1) == 0 and _need(lib, plan, lens, 1 << 24) > 0
    for bad in ([1, 20, 50], [0, 20, 20], [0, 30, 20]):
        off = np.asarray(bad, np.int64)
        assert int(lib.vit_workspace_bytes_packed_checkpointed(plan, 2, off.ctypes.data, 64)) == 0, bad
    assert int(lib.vit_workspace_bytes_packed_checkpointed(plan, 2, None, 64)) == 0
    off = np.asarray([0, 20, 50], np.int64)
    assert int(lib.vit_workspace_bytes_packed_checkpointed(None, 2, off.ctypes.data, 64)) == 0
    # decode before upload is refused, not executed
    dummy = ctypes.c_void_p(256 * 1024)
    assert lib.vit_decode_packed_checkpointed(plan, dummy, 0, 2, off.ctypes.data, dummy, 1 << 30, dummy, None, 64, None) == -6
    lib.vit_plan_destroy(plan)


def test_exports_are_declared():
    """tests/test_abi.py compares the header with the loader's list; both carry the two new entry points, the ABI version stays 4."""
    from tests import test_abi
    from viterbi_spl_amd import _lib
    names = test_abi.declared_functions()
    for n in ("vit_workspace_bytes_packed_checkpointed", "vit_decode_packed_checkpointed"):
        assert n in names and n in _lib.EXPORTS
    assert set(names) == set(_lib.EXPORTS) and _lib.ABI_VERSION == 4
