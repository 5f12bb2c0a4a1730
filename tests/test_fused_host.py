"""Host tier of the fused logits -> path decode (``vit_decode_logits``, csrc/fused.hip): the two entry points exist, which plans and
builder geometries ``vit_workspace_bytes_logits`` sizes and which it refuses, and the order of the refusals.  No GPU: the library
answers from the plan alone."""
import ctypes
import os
import re

import numpy as np
import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "viterbi_hip.h")
VIT_EINVAL, VIT_ENOTUPLOADED = -1, -6


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


def _obs(mode, n_bins, spw=None):
    from viterbi_spl_amd import _lib
    spw = (5, 15, 5)[mode] if spw is None else spw
    return _lib.ObsParams(mode, n_bins, spw, 0.0, 1.0, 2.0, None)


def _bytes(lib, plan, obs, B=8, T=100):
    return int(lib.vit_workspace_bytes_logits(plan, ctypes.byref(obs), B, T))


def test_declared_and_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("vit_workspace_bytes_logits", "vit_decode_logits"):
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in viterbi_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
    assert "vit_obs_params" in src
    assert lib.vit_abi_version() == 4


@pytest.mark.parametrize("name", ["tonet361", "msnet321"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_served_plans_and_builders(lib, golden, name, mode):
    """Every builder the reference ships, on both wave-form grids: a size that holds a full history in the wave layout (384 floats
    per frame and song) and no emission tensor."""
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    plan = _plan(lib, A, pi)
    S = A.shape[0]
    B, T = 8, 100
    need = _bytes(lib, plan, _obs(mode, S - 1), B, T)
    assert need >= B * T * 384 * 4
    assert need < B * T * 384 * 4 + B * T * S * 4, "the workspace must not hold an emission tensor"
    assert need == int(lib.vit_workspace_bytes_for(plan, B, T, 3)), "the wave form's full-history workspace"
    lib.vit_plan_destroy(plan)


def test_refused_before_anything_else(lib, golden):
    p = golden["params"]
    # a dense 361-state matrix, the 722-state jdc band: no wave form
    for name, S in (("dense361", 361), ("jdc722", 722)):
        plan = _plan(lib, p[f"{name}_logA_T"], p[f"{name}_log_pi"])
        for mode in (0, 1, 2):
            assert _bytes(lib, plan, _obs(mode, S - 1)) == 0, (name, mode)
        lib.vit_plan_destroy(plan)
    plan = _plan(lib, p["tonet361_logA_T"], p["tonet361_log_pi"])
    assert _bytes(lib, plan, _obs(0, 360)) > 0
    assert _bytes(lib, plan, _obs(0, 360, spw=7)) == 0          # a peak width the kernel is not instantiated for
    assert _bytes(lib, plan, _obs(1, 360, spw=5)) == 0          # the softmax builder ships with 15
    assert _bytes(lib, plan, _obs(0, 320)) == 0                 # n_bins + 1 != S
    assert _bytes(lib, plan, _obs(0, 361)) == 0
    assert _bytes(lib, plan, _obs(3, 360, spw=5)) == 0          # no such builder
    # "wave_uniform" 1 switches the last-state form off: the fused kernel has no general extra-column form
    assert lib.vit_plan_set_option(plan, b"wave_uniform", 1) == 0
    assert _bytes(lib, plan, _obs(0, 360)) == 0
    assert lib.vit_plan_set_option(plan, b"wave_uniform", 3) == 0
    assert _bytes(lib, plan, _obs(0, 360)) > 0
    assert lib.vit_plan_set_option(plan, b"reset", 0) == 0
    # "wave_history" 2 is ignored: the same full history
    full = _bytes(lib, plan, _obs(0, 360))
    assert lib.vit_plan_set_option(plan, b"wave_history", 2) == 0
    assert _bytes(lib, plan, _obs(0, 360)) == full
    lib.vit_plan_destroy(plan)


def test_decode_before_upload(lib, golden):
    """vit_decode_logits of a plan that was never uploaded: VIT_ENOTUPLOADED, whatever else is wrong with the call; without a plan
    or builder parameters: VIT_EINVAL."""
    p = golden["params"]
    plan = _plan(lib, p["tonet361_logA_T"], p["tonet361_log_pi"])
    obs = _obs(0, 360)
    rc = lib.vit_decode_logits(plan, None, ctypes.byref(obs), 4, 100, None, None, 0, None, None, None, None)
    assert rc == VIT_ENOTUPLOADED
    assert lib.vit_decode_logits(None, None, ctypes.byref(obs), 4, 100, None, None, 0, None, None, None, None) == VIT_EINVAL
    assert lib.vit_decode_logits(plan, None, None, 4, 100, None, None, 0, None, None, None, None) == VIT_EINVAL
    lib.vit_plan_destroy(plan)
