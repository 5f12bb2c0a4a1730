"""Bounded-workspace decode of the 722-state grids (workgroup-form plans) at full size, against the normal decode.

Workload: [256, 30000, 722], fp16 emissions, for the jdc matrix (band of +/- 40, floor form) and the Durrieu matrix (step form),
segments of K = 1024 frames.  Timed per plan, alternating, device events around whole synchronised calls after a warm-up round:
  (i)  decode (one delta row per frame: a 22 GB workspace);
  (ii) decode_checkpointed into a caller-owned workspace (30 + 1026 rows per song: 0.78 GB).
Prints one JSON line per plan: milliseconds of every round, medians, Mframes/s, the ratio (ii)/(i) in throughput, the two
workspace sizes, and whether the two results are the same bytes."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from viterbi_spl_amd import ViterbiDecoder, synth

ROUNDS = int(os.environ.get("ROUNDS", "5"))
B, T, S, K = 256, 30000, 722, int(os.environ.get("SEGMENT_FRAMES", "1024"))


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), out


def main():
    dev = torch.device("cuda:0")
    E = bench.tiled_emissions(synth.emissions_peaks, B, T, S, 1234, dev, torch.float16)
    for name, (kind, dmax) in (("jdc722", ("tonet", 40)), ("durrieu722", ("durrieu", 0))):
        A, pi = bench.make_params(kind, S, dmax)
        dec = ViterbiDecoder(A, pi, dev)
        need_ck = dec.workspace_bytes_checkpointed(B, T, K)
        need_full = dec.workspace_bytes(B, T, "auto")
        ws = torch.empty(need_ck + 256, dtype=torch.uint8, device=dev)
        runs = {
            "normal": lambda: dec.decode(E, out_dtype=torch.int32),
            "checkpointed": lambda: dec.decode_checkpointed(E, segment_frames=K, out_dtype=torch.int32, workspace=ws),
        }
        ms = {k: [] for k in runs}
        out = {}
        for r in range(ROUNDS + 1):                       # round 0 warms up
            for k, fn in runs.items():
                t, o = timed(fn)
                if r > 0:
                    ms[k].append(round(t, 3))
                out[k] = o
                del o
        same = bool(torch.equal(out["normal"][0], out["checkpointed"][0]) and torch.equal(out["normal"][1], out["checkpointed"][1]))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        print(json.dumps({
            "plan": name, "shape": [B, T, S], "segment_frames": K, "rounds": ROUNDS, "ms": ms, "median_ms": med,
            "spread_normal_ms": [min(ms["normal"]), max(ms["normal"])],
            "Mframes_per_s": {k: round(B * T / med[k] / 1e3, 1) for k in med},
            "checkpointed_over_normal": round(med["normal"] / med["checkpointed"], 3),
            "workspace_GB": {"normal": round(need_full / 1e9, 2), "checkpointed": round(need_ck / 1e9, 2)},
            "checkpointed_equals_normal": same}), flush=True)
        del dec, ws, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
