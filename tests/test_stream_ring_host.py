"""Host tier of the ring sessions (tests/test_gpu_stream_ring.py): the schedule replay of tests/ring_ref.py against
commit_ref.walk on small synthetic matrices, the new exports against the header, vit_workspace_bytes_stream_ring against the
documented layout, and the refusals that need no device.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import commit_ref as cr
from tests import ring_ref as rr
from tests.common import durrieu_log_params
from tests.f64_ref import band_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vit_workspace_bytes_stream_ring", "vit_stream_open_ring", "vit_stream_commit_ack", "vit_stream_commit_rel", "vit_stream_tail")
EINVAL, EUNSUPPORTED, ENOTUPLOADED = -1, -5, -6


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


def _small_case(seed, S=24, T=260):
    """A banded matrix small enough for the O(T S^2) reference, with emissions that merge within a few frames."""
    A, pi = band_params(S, 3)
    rng = np.random.default_rng(seed)
    E = (rng.integers(-2560, 1, size=(T, S)) / 256.0).astype(np.float32)
    peak = (np.arange(T) * 3 // 7 + rng.integers(0, 2, size=T)) % S
    E[np.arange(T), peak] = 0.0
    E[np.arange(T), (peak + 1) % S] -= 20.0
    return cr.back_pointers(A, pi, E)


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("R,L", [(64, 1 << 20), (64, 16), (96, 7)])
def test_replay_is_the_walk(seed, R, L):
    """ring_ref.replay restates commit_ref.walk (frontiers and states) and counts the ring events by their definitions."""
    psi = _small_case(seed)
    counts = [64, 1, 0, 3, 61, 1, 37, 0, 27, 2, 64]
    ns = np.cumsum(counts)
    steps = rr.replay(psi, counts, R, L)
    walk = cr.walk(psi, ns, L)
    assert len(steps) == len(walk)
    n0 = 0
    for s, (n, f0, f, st), c in zip(steps, walk, counts):
        assert (s["n0"], s["n"], s["f0"], s["f"]) == (n0, n, f0, f) and np.array_equal(s["states"], st)
        assert s["resident"] == (n - f0 <= R)
        assert s["wraps"] == len([t for t in range(n0, n) if t > 0 and t % R == 0])
        assert s["slot0"] == (c > 0 and n0 > 0 and n0 % R == 0)
        in_range = [t for t in range(f0 + 1, f) if t % R == 0]                       # a step R - 1 -> 0 inside [f0, f)
        assert s["range_straddle"] == bool(in_range)
        lo = f - 1 if f > f0 else max(f0, n - 1 - L)
        in_walk = [t for t in range(lo + 1, n - 1) if t % R == 0] if n >= 2 else []  # inside the rows [lo, n - 2]
        assert s["walk_straddle"] == bool(in_walk)
        n0 = n
    sm = rr.summary(steps)
    assert sm["wraps"] == (ns[-1] - 1) // R and sm["resident"] == all(s["resident"] for s in steps)


def test_replay_flags_a_schedule_that_does_not_fit():
    psi = _small_case(1)
    steps = rr.replay(psi, [64, 64, 64], 64, 1 << 20)
    assert steps[0]["resident"] and steps[0]["f"] > 0 and not steps[1]["resident"]      # 128 - f > 64 unless f >= 64
    assert not rr.summary(steps)["resident"]
    assert rr.smallest_ring([psi], [[64, 64, 64]], 1 << 20, candidates=(64, 128)) == 128
    assert rr.smallest_ring([psi], [[200]], 1 << 20, candidates=(64, 128)) is None
    # a lookback of 1 never finds a merge of these emissions' survivors: a stall, never a commit
    st = rr.replay(psi, [40, 40], 128, 1)
    assert not rr.summary(st)["stall_then_commit"] or st[-1]["f"] > 0


def test_exports_agree_with_the_header(lib):
    from viterbi_spl_amd import _lib
    with open(os.path.join(ROOT, "include", "viterbi_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define VIT_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4 and lib.vit_abi_version() == 4
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert len(re.findall(r"^(?:size_t|int) %s\(" % name, header, re.M)) == 1, name
    declared = set(re.findall(r"^(?:size_t|int|void|const char \*|int64_t)\s*\*?(vit_\w+)\(", header, re.M))
    assert set(_lib.EXPORTS) <= declared, sorted(set(_lib.EXPORTS) - declared)
    for text in ("64 <= ring_rows <= 2^30", "VIT_EWORKSPACE", "never an access", "outside the buffers", "with ring_rows in place of T_cap"):
        assert text in header, text


@pytest.mark.parametrize("S,half", [(361, 14), (321, 14), (722, 40)])
def test_size_is_the_documented_layout(lib, S, half):
    """st_layout with R for T_cap: [B][R] rows of SD floats, then the tables of a linear session, each padded to 256 bytes."""
    plan = _plan(lib, *band_params(S, half))
    SD = (S + 5) // 4 * 4
    a256 = lambda x: (x + 255) // 256 * 256
    for B, R in ((1, 64), (2, 65), (3, 2048), (1024, 2048), (1, 1 << 30)):
        want = (a256(B * R * SD * 4) + a256(B * 16 * 4) + a256(B * 8 * 4) + a256(B * 4) + a256(B * 4) + a256(B * 256 * 4) + a256(B * 8)
                + a256(B * 2 * 4))
        got = int(lib.vit_workspace_bytes_stream_ring(plan, B, R))
        assert got == want == int(lib.vit_workspace_bytes_stream(plan, B, R)), (B, R, got, want)
    # one tonet-sized recording of 30 000 frames against its ring of 2048 rows
    if S == 361:
        lin, ring = int(lib.vit_workspace_bytes_stream(plan, 1, 30000)), int(lib.vit_workspace_bytes_stream_ring(plan, 1, 2048))
        assert lin > 43_000_000 and ring < 3_100_000
    for B, R in ((1, 63), (1, (1 << 30) + 1), (0, 64), (1, 0), (1, -64), ((1 << 30) + 1, 64)):
        assert int(lib.vit_workspace_bytes_stream_ring(plan, B, R)) == 0, (B, R)
    assert int(lib.vit_workspace_bytes_stream_ring(None, 1, 64)) == 0
    lib.vit_plan_destroy(plan)


def test_unserved_plans_and_host_refusals(lib):
    """Step plans and unstructured plans: size 0; open_ring's status order up to the upload; NULL sessions."""
    A, pi = durrieu_log_params(721, 20)
    step = _plan(lib, A, pi)
    assert int(lib.vit_workspace_bytes_stream(step, 2, 64)) > 0 and int(lib.vit_workspace_bytes_stream_ring(step, 2, 64)) == 0
    assert int(lib.vit_workspace_bytes_stream_commit(step, 2)) == 0
    rng = np.random.default_rng(0)
    un = _plan(lib, -rng.random((80, 80), dtype=np.float32) * 9, np.full(80, -np.log(80), np.float32))
    assert int(lib.vit_workspace_bytes_stream_ring(un, 2, 64)) == 0
    served = _plan(lib, *band_params(361, 14))
    buf = np.zeros(1 << 12, np.uint8)
    ptr = (buf.ctypes.data + 255) & ~255
    h = ctypes.c_void_p()
    for plan in (step, un, served):
        assert lib.vit_stream_open_ring(plan, 2, 63, ptr, 1 << 40, ctypes.byref(h)) == EINVAL
        assert lib.vit_stream_open_ring(plan, 2, (1 << 30) + 1, ptr, 1 << 40, ctypes.byref(h)) == EINVAL
        assert lib.vit_stream_open_ring(plan, 2, 64, ptr + 8, 1 << 40, ctypes.byref(h)) == EINVAL
        assert lib.vit_stream_open_ring(plan, 2, 64, None, 1 << 40, ctypes.byref(h)) == EINVAL
        assert lib.vit_stream_open_ring(plan, 2, 64, ptr, 1 << 40, None) == EINVAL
        assert lib.vit_stream_open_ring(plan, 2, 64, ptr, 1 << 40, ctypes.byref(h)) == ENOTUPLOADED      # (before EUNSUPPORTED, as vit_stream_open)
        assert lib.vit_stream_open(plan, 2, 64, ptr, 1 << 40, ctypes.byref(h)) == ENOTUPLOADED
    assert lib.vit_stream_open_ring(None, 2, 64, ptr, 1 << 40, ctypes.byref(h)) == EINVAL and not h.value
    z = np.zeros(2, np.int64)
    assert lib.vit_stream_commit_ack(None, z.ctypes.data) == EINVAL
    assert lib.vit_stream_commit_rel(None, ptr, 64, ptr, ptr, 8, None) == EINVAL
    assert lib.vit_stream_tail(None, ptr, 64, ptr, None, None) == EINVAL
    assert not buf.any()
    for plan in (step, un, served):
        lib.vit_plan_destroy(plan)
