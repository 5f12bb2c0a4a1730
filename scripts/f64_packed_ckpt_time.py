"""Packed ragged float64 decode under a workspace budget (decode_f64_packed_checkpointed) at full size, against what it replaces.

Workloads: the recording sets of f64_packed_time.py (lengths uniform in [7500, 30000], seed 7):
  jdc722_fp16    S = 722, fp16 emissions, the jdc matrix, 401 recordings, 7.68 M frames;
  tonet361_fp32  S = 361, fp32 emissions, the tonet matrix, 202 recordings, 3.84 M frames.
Timed per grid, alternating in one process, device events around whole calls on the stream, ROUNDS rounds after a warm-up round:
  full          decode_f64_packed, the whole history;
  pc_K          decode_f64_packed_checkpointed at K = 1024 and K = 2048;
  groups_K      decode_f64_packed(max_workspace_bytes = the bytes of pc_K): consecutive groups of recordings, the fallback this replaces;
  padded_K      decode_f64_checkpointed at the same K on the batch padded to 30000 frames.
tonet361 also runs pc_K with "f64_units_per_cu" in {1, 2, 4} (units per compute unit and launch; it changes the workspace).  With 202
recordings on 256 compute units every u gives 202 units per launch, so a third set, tonet361_fp32_x4 (four times the frames, 808
recordings), runs `full` and that sweep alone: there u decides the units per launch.
One JSON document to --out (default profiles/f64_packed_ckpt_time.json): per grid and arm the milliseconds of every round, their range
(min, max) and median, the workspace bytes, whether the ranges of pc_K and groups_K are disjoint, and a bit-exact check of every arm
against `full`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from scripts.f64_packed_time import T, ragged_lengths, timed
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

ROUNDS = int(os.environ.get("ROUNDS", "5"))
SEGMENTS = (1024, 2048)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f64_packed_ckpt_time.json"))
    ap.add_argument("--grids", default="jdc722_fp16,tonet361_fp32,tonet361_fp32_x4")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this script measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    params = np.load(os.path.join(ROOT, "tests", "golden", "params.npz"))
    report = {"T": T, "rounds": ROUNDS, "device": torch.cuda.get_device_name(dev)}
    for name, key, S, dt, uni, sweep, sweep_only in (("jdc722_fp16", "jdc722", 722, torch.float16, 256, (), False),
                                                    ("tonet361_fp32", "tonet361", 361, torch.float32, 128, (1, 2, 4), False),
                                                    ("tonet361_fp32_x4", "tonet361", 361, torch.float32, 512, (1, 2, 4), True)):
        if name not in args.grids.split(","):
            continue
        lens = ragged_lengths(uni * T)
        B = len(lens)
        off = np.zeros(B + 1, np.int64)
        off[1:] = np.cumsum(lens)
        N = int(off[-1])
        dec = ViterbiDecoder(params[f"{key}_logA_T"], params[f"{key}_log_pi"], dev)
        E_pad = bench.tiled_emissions(synth.emissions_peaks, B, T, S, 1234, dev, dt)
        E_pk = torch.cat([E_pad[b, :lens[b]] for b in range(B)], dim=0).contiguous()
        lens_d = torch.from_numpy(lens).to(dev)
        units = lambda: int(_lib.load().vit_f64_packed_bounded_units(dec._plan, B))
        need = {"full": dec.workspace_bytes_f64_packed(B, N)}
        unit_count = {"default": units()}
        ws = torch.empty(need["full"] + 256, dtype=torch.uint8, device=dev)        # every arm decodes in the front of this one tensor
        runs = {"full": lambda: dec.decode_f64_packed(E_pk, off, out_dtype=torch.int32, workspace=ws)}
        for K in SEGMENTS:
            need[f"pc_{K}"] = dec.workspace_bytes_f64_packed_checkpointed(off, K)
            if not sweep_only:
                need[f"groups_{K}"] = dec.plan_workspace_f64_packed(off, need[f"pc_{K}"])["bytes"]
                need[f"padded_{K}"] = dec.workspace_bytes_f64_checkpointed(B, T, K)
                runs[f"pc_{K}"] = lambda K=K: dec.decode_f64_packed_checkpointed(E_pk, off, segment_frames=K, out_dtype=torch.int32, workspace=ws)
                runs[f"groups_{K}"] = lambda K=K: dec.decode_f64_packed(E_pk, off, out_dtype=torch.int32, workspace=ws, max_workspace_bytes=need[f"pc_{K}"])
                runs[f"padded_{K}"] = lambda K=K: dec.decode_f64_checkpointed(E_pad, segment_frames=K, lengths=lens_d, out_dtype=torch.int32, workspace=ws)
            for u in sweep:
                def swept(K=K, u=u):
                    dec.set_option("f64_units_per_cu", u)
                    try:
                        return dec.decode_f64_packed_checkpointed(E_pk, off, segment_frames=K, out_dtype=torch.int32, workspace=ws)
                    finally:
                        dec.set_option("f64_units_per_cu", 0)
                dec.set_option("f64_units_per_cu", u)
                need[f"pc_{K}_u{u}"] = dec.workspace_bytes_f64_packed_checkpointed(off, K)
                unit_count[f"u{u}"] = units()
                dec.set_option("f64_units_per_cu", 0)
                runs[f"pc_{K}_u{u}"] = swept
        assert max(need.values()) == need["full"], need
        ms = {k: [] for k in runs}
        same = {}
        base = None
        for r in range(ROUNDS + 1):                       # round 0 warms up
            for k, fn in runs.items():
                t, (s, l) = timed(fn)
                if r > 0:
                    ms[k].append(round(t, 3))
                elif k == "full":
                    base = (s.clone(), l.clone())
                elif k.startswith("padded"):
                    same[k] = bool(all(torch.equal(base[0][off[b]:off[b + 1]], s[b, :lens[b]]) for b in range(B))
                                   and torch.equal(l.view(torch.int64), base[1].view(torch.int64)))
                else:
                    same[k] = bool(torch.equal(s, base[0]) and torch.equal(l.view(torch.int64), base[1].view(torch.int64)))
                del s, l
        rng_ms = {k: [min(v), max(v)] for k, v in ms.items()}
        pairs = () if sweep_only else SEGMENTS
        report[name] = {
            "S": S, "window": int(dec.info["group_window"]), "songs": int(B), "real_frames": N, "units_per_launch": unit_count,
            "groups": {str(K): len(dec.plan_workspace_f64_packed(off, need[f"pc_{K}"])["groups"]) for K in pairs},
            "ms": ms, "range_ms": rng_ms, "median_ms": {k: float(np.median(v)) for k, v in ms.items()},
            "workspace_bytes": need,
            "ranges_disjoint_pc_below_groups": {str(K): bool(rng_ms[f"pc_{K}"][1] < rng_ms[f"groups_{K}"][0]) for K in pairs},
            "ranges_disjoint_pc_and_groups": {str(K): bool(rng_ms[f"pc_{K}"][1] < rng_ms[f"groups_{K}"][0] or rng_ms[f"groups_{K}"][1] < rng_ms[f"pc_{K}"][0])
                                              for K in pairs},
            "bits_equal_full": same}
        print(json.dumps({name: report[name]}), flush=True)
        del dec, ws, base, E_pad, E_pk, runs
        torch.cuda.empty_cache()
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
