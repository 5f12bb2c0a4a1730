"""The bounded-workspace float64 decode (decode_f64_checkpointed) at full size: [128, 30000, 361] fp32 (the tonet band) and
[256, 30000, 722] fp16 (the jdc band), at K = 1024 and at the K plan_workspace_f64 picks for a budget of one eighth of the whole
history.  Three ways to the same bits:
  (i)   decode_f64: the whole history;
  (ii)  decode_f64_checkpointed in a workspace of its own size;
  (iii) decode_f64 over consecutive sub-batches whose whole history fits (ii)'s bytes -- what a caller can do on the host without (ii).
Device events around whole synchronised calls, a warm-up round first, the three alternating in one process, ROUNDS rounds.  One JSON
document to --out (default profiles/f64_ckpt_time.json).  BATCH_SCALE=0.25 / ROUNDS=3 select a smaller run."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f64_ckpt_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this script measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    params = np.load(os.path.join(ROOT, "tests", "golden", "params.npz"))
    report = {"T": T, "rounds": ROUNDS, "device": torch.cuda.get_device_name(dev)}
    for name, key, B, S, dt in (("S361_fp32", "tonet361", int(128 * SCALE), 361, torch.float32), ("S722_fp16", "jdc722", int(256 * SCALE), 722, torch.float16)):
        A, pi = params[f"{key}_logA_T"], params[f"{key}_log_pi"]
        dec = ViterbiDecoder(A, pi, dev)
        E = synth.emissions_peaks(B, T, S, seed=S, device=dev, dtype=dt)
        full = dec.workspace_bytes_f64(B, T)
        picked = dec.plan_workspace_f64(B, T, full // 8)
        assert picked["mode"] == "checkpointed"
        ws_full = torch.empty(full + 256, dtype=torch.uint8, device=dev)
        ref_s, ref_l = dec.decode_f64(E, out_dtype=torch.int32, workspace=ws_full)
        torch.cuda.synchronize()
        entry = {"B": B, "S": S, "window": dec.info["group_window"], "frames": B * T, "full_workspace_bytes": full,
                 "budget_an_eighth_bytes": full // 8, "segment_frames_picked_for_an_eighth": picked["segment_frames"], "by_segment_frames": {}}
        for K in sorted({1024, picked["segment_frames"]}):
            need = dec.workspace_bytes_f64_checkpointed(B, T, K)
            ws_ck = torch.empty(need + 256, dtype=torch.uint8, device=dev)
            g = B                                       # (iii): the most songs whose whole history fits the checkpointed decode's bytes
            while g > 0 and dec.workspace_bytes_f64(g, T) > need:
                g -= 1

            def grouped():
                for b0 in range(0, B, g):
                    dec.decode_f64(E[b0:b0 + g], out_dtype=torch.int32, workspace=ws_ck)

            runs = {"full": lambda: dec.decode_f64(E, out_dtype=torch.int32, workspace=ws_full),
                    "checkpointed": lambda: dec.decode_f64_checkpointed(E, segment_frames=K, out_dtype=torch.int32, workspace=ws_ck)}
            if g > 0:
                runs["host_groups"] = grouped
            for fn in runs.values():
                timed(fn)
            ms = {k: [] for k in runs}
            for _ in range(ROUNDS):
                for k, fn in runs.items():
                    ms[k].append(round(timed(fn)[0], 3))
            cs, cl = dec.decode_f64_checkpointed(E, segment_frames=K, out_dtype=torch.int32, workspace=ws_ck)
            torch.cuda.synchronize()
            same = bool(torch.equal(cs, ref_s)) and bool(torch.equal(cl.view(torch.int64), ref_l.view(torch.int64)))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            entry["by_segment_frames"][str(K)] = {
                "workspace_bytes": need, "workspace_over_full": round(need / full, 4), "segments": -(-T // K),
                "songs_per_host_group": g, "host_groups": -(-B // g) if g > 0 else None,
                "ms": ms, "median_ms": med, "range_ms": {k: [min(v), max(v)] for k, v in ms.items()},
                "checkpointed_over_full": round(med["checkpointed"] / med["full"], 3),
                "host_groups_over_checkpointed": round(med["host_groups"] / med["checkpointed"], 3) if g > 0 else None,
                "checkpointed_equals_full_bit_for_bit": same}
            print(name, K, json.dumps(med), "same bits:", same, flush=True)
            del ws_ck
            torch.cuda.empty_cache()
        report[name] = entry
        del E, ws_full, dec, ref_s, ref_l
        torch.cuda.empty_cache()
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
