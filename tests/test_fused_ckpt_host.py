"""CPU tier of the fused logits decode under a workspace budget (vit_decode_logits_checkpointed): the exports, the size function on
host-only plans -- it answers what vit_workspace_bytes_checkpointed answers wherever the fused workgroup serves the plan and the
builder, and 0 elsewhere -- and the segment-length search of ``ViterbiDecoder.plan_workspace_logits``.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from viterbi_spl_amd import ViterbiDecoder, _lib
from viterbi_spl_amd._lib import ViterbiHipError

# the reference's three builder geometries: (mode, single-side peak width)
BUILDERS = ((0, 5), (1, 15), (2, 5))
SHAPES = ((1, 1, 64), (5, 129, 64), (1024, 30000, 1024), (3, 100, 4096))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _plan(lib, A, pi):
    A, pi = np.ascontiguousarray(A, np.float32), np.ascontiguousarray(pi, np.float32)
    plan = ctypes.c_void_p()
    assert lib.vit_plan_create(A.ctypes.data, pi.ctypes.data, A.shape[0], ctypes.byref(plan)) == 0
    return plan


def _obs(mode, n_bins, spw):
    return _lib.ObsParams(mode, n_bins, spw, -0.75, 1.386 if mode == 0 else 0.0, 2.0 if mode == 0 else 0.0, None)


def _size(lib, plan, obs, B, T, K):
    return int(lib.vit_workspace_bytes_logits_checkpointed(plan, ctypes.byref(obs), B, T, K))


def test_header_loader_and_exports_agree(lib):
    from tests.test_abi import declared_functions
    names = declared_functions()
    for n in ("vit_workspace_bytes_logits_checkpointed", "vit_decode_logits_checkpointed"):
        assert n in names and n in _lib.EXPORTS and hasattr(lib, n)
    assert set(names) == set(_lib.EXPORTS)
    assert lib.vit_abi_version() == 4 and _lib.ABI_VERSION == 4
    assert lib.vit_workspace_bytes_logits_checkpointed.restype is ctypes.c_size_t
    assert lib.vit_decode_logits_checkpointed.restype is ctypes.c_int32
    assert len(lib.vit_workspace_bytes_logits_checkpointed.argtypes) == 5 and len(lib.vit_decode_logits_checkpointed.argtypes) == 12


@pytest.mark.parametrize("name", ["tonet361", "msnet321"])
def test_size_equals_the_checkpointed_decode(lib, golden, name):
    """The workspace is ck_layout's of the wave family: the bytes of vit_workspace_bytes_checkpointed, for every builder geometry."""
    p = golden["params"]
    plan = _plan(lib, p[f"{name}_logA_T"], p[f"{name}_log_pi"])
    S = p[f"{name}_logA_T"].shape[0]
    for mode, spw in BUILDERS:
        for B, T, K in SHAPES:
            want = int(lib.vit_workspace_bytes_checkpointed(plan, B, T, K))
            assert want > 0 and _size(lib, plan, _obs(mode, S - 1, spw), B, T, K) == want, (name, mode, B, T, K)
    # the figure of the README: [1024, 30000, 361] at K = 1024 is (30 + 1025) rows of 1536 bytes per song and some tables
    if S == 361:
        need = _size(lib, plan, _obs(0, 360, 5), 1024, 30000, 1024)
        rows = 1024 * (30 + 1025) * 1536
        assert rows <= need <= rows + 1024 * 1024 and need < 1.7e9
    obs = _obs(0, S - 1, 5)
    assert _size(lib, plan, obs, 3, 100, 1 << 24) == _size(lib, plan, obs, 3, 100, 100) > 0       # a K above T acts like T
    assert _size(lib, plan, obs, 0, 100, 64) == int(lib.vit_workspace_bytes_checkpointed(plan, 0, 100, 64))
    assert _size(lib, plan, obs, -1, 100, 64) == 0 and _size(lib, plan, obs, 1, 0, 64) == 0
    assert int(lib.vit_workspace_bytes_logits_checkpointed(None, ctypes.byref(obs), 1, 100, 64)) == 0
    assert int(lib.vit_workspace_bytes_logits_checkpointed(plan, None, 1, 100, 64)) == 0
    lib.vit_plan_destroy(plan)


def test_size_zero_where_not_served(lib, golden):
    """0 for plans without the fused workgroup (the 722-state grids, an unstructured matrix), for a builder geometry the reference
    does not ship (spw 4), for n_bins + 1 != S, for K outside 64 .. 2^24 and with "wave_uniform" 1; the decode call on a plan that
    was never uploaded answers VIT_ENOTUPLOADED."""
    p = golden["params"]
    for name in ("jdc722", "durrieu722", "dense97"):
        A = p[f"{name}_logA_T"]
        plan = _plan(lib, A, p[f"{name}_log_pi"])
        for mode, spw in BUILDERS:
            assert _size(lib, plan, _obs(mode, A.shape[0] - 1, spw), 3, 100, 64) == 0, (name, mode)
        lib.vit_plan_destroy(plan)
    plan = _plan(lib, p["tonet361_logA_T"], p["tonet361_log_pi"])
    good = _obs(0, 360, 5)
    assert _size(lib, plan, good, 3, 100, 64) > 0
    assert _size(lib, plan, _obs(0, 360, 4), 3, 100, 64) == 0                   # spw 4
    assert _size(lib, plan, _obs(1, 360, 5), 3, 100, 64) == 0                   # the softmax builder's width is 15
    assert _size(lib, plan, _obs(0, 320, 5), 3, 100, 64) == 0                   # n_bins + 1 != S
    assert _size(lib, plan, good, 3, 100, 63) == 0 and _size(lib, plan, good, 3, 100, (1 << 24) + 1) == 0
    assert _size(lib, plan, good, 3, 100, 1 << 24) > 0
    dummy = ctypes.c_void_p(256 * 1024)
    assert lib.vit_decode_logits_checkpointed(plan, dummy, ctypes.byref(good), 1, 100, None, dummy, 1 << 30, dummy, None, 64, None) == -6
    assert lib.vit_decode_logits_checkpointed(None, dummy, ctypes.byref(good), 1, 100, None, dummy, 1 << 30, dummy, None, 64, None) == -1
    assert lib.vit_decode_logits_checkpointed(plan, dummy, None, 1, 100, None, dummy, 1 << 30, dummy, None, 64, None) == -1
    assert lib.vit_plan_set_option(plan, b"wave_uniform", 1) == 0
    assert _size(lib, plan, good, 3, 100, 64) == 0                              # "wave_uniform" 1: no fused instantiation
    assert int(lib.vit_workspace_bytes_checkpointed(plan, 3, 100, 64)) > 0      # (the emission-tensor decode still serves it)
    for opt in (2, 3):
        assert lib.vit_plan_set_option(plan, b"wave_uniform", opt) == 0
        assert _size(lib, plan, good, 3, 100, 64) == int(lib.vit_workspace_bytes_checkpointed(plan, 3, 100, 64))
    lib.vit_plan_destroy(plan)


class _HostDecoder(ViterbiDecoder):
    """plan_workspace_logits and the size functions over a plan that was never uploaded: no device is involved."""

    def __init__(self, lib, A, pi):                      # (no super().__init__: that uploads the plan)
        self._plan = _plan(lib, A, pi)
        self.S = A.shape[0]
        self.device = None


def test_plan_workspace_logits(lib, golden):
    """The whole history where it fits or no budget is set; else the largest K of 8192 .. 64 whose workspace fits; below the least
    need of any K -- size(64) for songs of up to about 4000 frames, a larger K's for longer ones -- a ViterbiHipError that names it."""
    p = golden["params"]
    dec = _HostDecoder(lib, p["tonet361_logA_T"], p["tonet361_log_pi"])
    obs = ViterbiDecoder.obs_params("shaun", 360, 5, -0.75, 1.386, 2.0)
    B, T = 1024, 30000
    full = dec.workspace_bytes_logits(obs, B, T)
    assert full == int(lib.vit_workspace_bytes_logits(dec._plan, ctypes.byref(dec._obs_struct(obs)), B, T)) > 47e9
    for budget in (None, full, full + 1, 10 ** 13):
        assert dec.plan_workspace_logits(obs, B, T, budget) == {"mode": "full", "workspace_bytes": full}

    def ck(K):
        return dec.workspace_bytes_logits_checkpointed(obs, B, T, K)
    KS = (8192, 4096, 2048, 1024, 512, 256, 128, 64)
    least = min(ck(k) for k in KS)

    def largest_fitting(budget):
        return next(k for k in KS if ck(k) <= budget)
    # rows per song are T / K + K + 1: the need falls with K down to about sqrt(T) and rises again below (K = 64 needs more than 128 and 256)
    assert ck(8192) > ck(1024) > ck(256) > ck(128) == least < ck(64)
    for K in KS:
        for budget in (ck(K), ck(K) + 1):
            want = largest_fitting(budget)
            assert want >= K
            assert dec.plan_workspace_logits(obs, B, T, budget) == {"mode": "checkpointed", "segment_frames": want, "workspace_bytes": ck(want)}, (K, budget)
    for K in (8192, 4096, 2048, 1024, 512):                                                      # where the need still falls: K exactly
        assert dec.plan_workspace_logits(obs, B, T, ck(K))["segment_frames"] == K
        assert dec.plan_workspace_logits(obs, B, T, ck(K) - 1)["segment_frames"] == K // 2
    assert dec.plan_workspace_logits(obs, B, T, full - 1)["segment_frames"] == 8192              # never above 8192, whatever would fit
    got = dec.plan_workspace_logits(obs, B, T, full // 8)
    assert got["mode"] == "checkpointed" and got["workspace_bytes"] == ck(got["segment_frames"]) <= full // 8
    assert got["segment_frames"] == 2048 and ck(4096) > full // 8
    assert ck(1024) < 1.7e9
    # nothing fits below the least need of any K, and the error names it
    assert dec.plan_workspace_logits(obs, B, T, least)["workspace_bytes"] == least
    with pytest.raises(ViterbiHipError, match=str(least)):
        dec.plan_workspace_logits(obs, B, T, least - 1)
    # short songs: every K >= T is one segment, the need rises with K from 64 on, and below size(64) nothing fits
    def ck_short(K):
        return dec.workspace_bytes_logits_checkpointed(obs, 8, 2000, K)
    assert min(ck_short(k) for k in KS) == ck_short(64)
    assert dec.plan_workspace_logits(obs, 8, 2000, ck_short(64))["segment_frames"] == 64
    with pytest.raises(ViterbiHipError, match=str(ck_short(64))):
        dec.plan_workspace_logits(obs, 8, 2000, ck_short(64) - 1)
    # a builder the fused workgroup does not serve: a loud error, budget or not
    bad = ViterbiDecoder.obs_params("shaun", 360, 4, -0.75, 1.386, 2.0)
    for budget in (None, full // 8):
        with pytest.raises(ViterbiHipError):
            dec.plan_workspace_logits(bad, B, T, budget)
