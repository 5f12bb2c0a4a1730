#!/usr/bin/env python3
"""Record what every workspace-size query of libviterbi_hip.so answers for the plans of tests/golden/params.npz
(tests/golden/workspace_sizes.json, compared byte for byte by tests/test_workspace_sizes_host.py).

A plan that was never uploaded assumes 256 compute units, so every query is answered from the plan and the shapes alone: no GPU.
Reads nothing but params.npz and our own library.  Run it only where a size is MEANT to change; a refactor must reproduce the file."""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "workspace_sizes.json")

SHAPES = [(1, 1), (3, 130), (513, 700)]                          # (B, T) of the padded queries
LENGTHS = [[1], [1, 2, 63, 64, 65, 700], [50, 60]]               # recordings of the packed queries
SEGMENTS = [63, 64, 100, 1 << 24]                                # 63: refused
ALGOS = [0, 1, 2, 3, 4]                                          # auto, dense, banded, wave, group
BUILDERS = [(0, 5), (1, 15), (2, 5), (0, 7)]                     # (mode, peak width): the three geometries served, one refused
SCAN_ONLY = "jdc722_scan_only"


def plan_names(params):
    return sorted(k[:-len("_logA_T")] for k in params.files if k.endswith("_logA_T"))


def scan_only_jdc722(params):
    """jdc722 with one in-window entry below its row's constant (tests/test_packed_bounded_host.py::_scan_only_jdc722)."""
    A = np.array(params["jdc722_logA_T"], np.float32, copy=True)
    vals, counts = np.unique(A[300], return_counts=True)
    A[300, 303] = np.float32(vals[np.argmax(counts)]) - np.float32(5)
    return A, params["jdc722_log_pi"]


def plan_sizes(lib, A, pi):
    """Every size query for one plan -> {"query|arguments": answer}."""
    from viterbi_spl_amd import _lib
    A = np.ascontiguousarray(A, np.float32)
    pi = np.ascontiguousarray(pi, np.float32)
    S = A.shape[0]
    plan = ctypes.c_void_p()
    assert lib.vit_plan_create(A.ctypes.data, pi.ctypes.data, S, ctypes.byref(plan)) == 0
    out = {}
    for B, T in SHAPES:
        out[f"bytes|{B}|{T}"] = int(lib.vit_workspace_bytes(plan, B, T))
        for wh in (0, 2):
            assert lib.vit_plan_set_option(plan, b"wave_history", wh) == 0
            for algo in ALGOS:
                out[f"for|{B}|{T}|algo{algo}|wave_history{wh}"] = int(lib.vit_workspace_bytes_for(plan, B, T, algo))
        assert lib.vit_plan_set_option(plan, b"reset", 0) == 0
        out[f"f64|{B}|{T}"] = int(lib.vit_workspace_bytes_f64(plan, B, T))
        for K in SEGMENTS:
            out[f"checkpointed|{B}|{T}|{K}"] = int(lib.vit_workspace_bytes_checkpointed(plan, B, T, K))
            out[f"f64_checkpointed|{B}|{T}|{K}"] = int(lib.vit_workspace_bytes_f64_checkpointed(plan, B, T, K))
        for mode, spw in BUILDERS:
            obs = _lib.ObsParams(mode, S - 1, spw, 0.0, 1.0, 2.0, None)
            out[f"logits|{B}|{T}|mode{mode}|spw{spw}"] = int(lib.vit_workspace_bytes_logits(plan, ctypes.byref(obs), B, T))
        out[f"units|{B}"] = int(lib.vit_packed_bounded_units(plan, B))
    for lens in LENGTHS:
        off = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)
        B, tag = len(lens), ",".join(str(n) for n in lens)
        out[f"packed|{tag}"] = int(lib.vit_workspace_bytes_packed(plan, B, int(off[-1])))
        out[f"f64_packed|{tag}"] = int(lib.vit_workspace_bytes_f64_packed(plan, B, int(off[-1])))
        out[f"units|{B}"] = int(lib.vit_packed_bounded_units(plan, B))
        for K in SEGMENTS:
            out[f"packed_checkpointed|{tag}|{K}"] = int(lib.vit_workspace_bytes_packed_checkpointed(plan, B, off.ctypes.data, K))
            out[f"packed_bounded|{tag}|{K}"] = int(lib.vit_workspace_bytes_packed_bounded(plan, B, off.ctypes.data, K))
    lib.vit_plan_destroy(plan)
    return out


def all_sizes(lib, params):
    sizes = {name: plan_sizes(lib, params[f"{name}_logA_T"], params[f"{name}_log_pi"]) for name in plan_names(params)}
    sizes[SCAN_ONLY] = plan_sizes(lib, *scan_only_jdc722(params))
    return sizes


if __name__ == "__main__":
    from viterbi_spl_amd import _lib
    sizes = all_sizes(_lib.load(), np.load(os.path.join(HERE, "params.npz")))
    with open(OUT, "w") as fh:
        json.dump(sizes, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{OUT}: {len(sizes)} plans, {sum(len(v) for v in sizes.values())} answers")
