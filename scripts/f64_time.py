"""The float64-accumulating decode (decode_f64) at full size against its structural twin, the float32 decode of the same plan forced
to the one-target floor kernel (forward_form 1): [128, 30000, 361] fp32 (the tonet band) and [256, 30000, 722] fp16 (the jdc band).
Device events around whole synchronised calls, a warm-up round first, the two alternating in one process, ROUNDS rounds.  The
float32 twin is timed as a whole and as forward / back-trace; decode_f64 is one entry point and is timed as a whole (for a forward /
back-trace split of both arithmetics by one method, run this script under a kernel trace and read the kernels' durations).  For
scale: the NumPy restatement of the reference's float64 function (tests/f64_ref.py) on ONE 30000-frame song of the first grid, on
the host.  One JSON document to --out (default profiles/f64_decode_time.json).
BATCH_SCALE=0.25 / ROUNDS=3 select a smaller run."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import f64_ref
from viterbi_spl_amd import ViterbiDecoder, synth

ROUNDS = int(os.environ.get("ROUNDS", "5"))
SCALE = float(os.environ.get("BATCH_SCALE", "1"))
T = 30000


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f64_decode_time.json"))
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this script measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    params = np.load(os.path.join(ROOT, "tests", "golden", "params.npz"))
    report = {"T": T, "rounds": ROUNDS, "device": torch.cuda.get_device_name(dev)}
    for name, key, B, S, dt in (("S361_fp32", "tonet361", int(128 * SCALE), 361, torch.float32), ("S722_fp16", "jdc722", int(256 * SCALE), 722, torch.float16)):
        A, pi = params[f"{key}_logA_T"], params[f"{key}_log_pi"]
        dec = ViterbiDecoder(A, pi, dev)
        dec.set_option("forward_form", 1)            # the float32 twin: one target per lane, the floor form
        E = synth.emissions_peaks(B, T, S, seed=S, device=dev, dtype=dt)
        st = torch.empty((B, T), dtype=torch.int32, device=dev)
        ll = torch.empty((B,), dtype=torch.float32, device=dev)
        runs = {
            "f64_decode": lambda: dec.decode_f64(E, out_dtype=torch.int32),
            "f32_decode": lambda: dec.decode_into(E, st, ll, algo="group"),
            "f32_forward": lambda: dec.decode_into(E, st, ll, algo="group", phase="forward"),
            "f32_backtrace": lambda: dec.decode_into(E, st, ll, algo="group", phase="backtrace"),
        }
        for fn in runs.values():
            timed(fn)
        ms = {k: [] for k in runs}
        for _ in range(ROUNDS):
            for k, fn in runs.items():
                ms[k].append(round(timed(fn)[0], 3))
        s64, _ = dec.decode_f64(E, out_dtype=torch.int32)
        torch.cuda.synchronize()
        differ = int((s64 != st).sum())
        med = {k: float(np.median(v)) for k, v in ms.items()}
        report[name] = {"B": B, "S": S, "window": dec.info["group_window"], "ms": ms, "median_ms": med,
                        "range_ms": {k: [min(v), max(v)] for k, v in ms.items()},
                        "f64_over_f32_decode": round(med["f64_decode"] / med["f32_decode"], 3),
                        "Mframes_per_s": {k: round(B * T / med[k] / 1e3, 2) for k in ("f64_decode", "f32_decode")},
                        "frames_where_the_paths_differ": differ, "frames": B * T}
        if name == "S361_fp32" and not args.no_host:
            e0 = E[0].cpu().numpy()
            t0 = time.perf_counter()
            rs, _ = f64_ref.decode_f64(A, pi, e0)
            host_s = time.perf_counter() - t0
            assert np.array_equal(rs, s64[0].cpu().numpy())
            report[name]["host_restatement_s_per_song"] = round(host_s, 2)
            report[name]["gpu_ms_per_song_in_the_batch"] = round(med["f64_decode"] / B, 3)
            report[name]["host_over_gpu_per_song"] = round(host_s * 1e3 / (med["f64_decode"] / B), 0)
            report[name]["host_over_gpu_one_song_latency"] = None
            one = lambda: dec.decode_f64(E[:1], out_dtype=torch.int32)
            timed(one)
            lat = float(np.median([timed(one)[0] for _ in range(3)]))
            report[name]["gpu_ms_one_song_alone"] = round(lat, 2)
            report[name]["host_over_gpu_one_song_latency"] = round(host_s * 1e3 / lat, 1)
        del E, st, dec
        torch.cuda.empty_cache()
        print(name, json.dumps(report[name]["median_ms"]), flush=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
