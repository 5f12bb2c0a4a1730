"""The fused logits decode under a workspace budget (vit_decode_logits_checkpointed) at full size, against the three other ways to
get from logits to paths.

Workload: [B, 30000, 360] "shaun" logits resident in HBM, S = 361 (the tonet matrix), songs repeating with period 32 (bench.py's
pipeline block), B in {1024, 2048}; segment lengths K = 1024 and the K that plan_workspace_logits picks for an eighth of the whole
history's bytes.  One process; per (B, K) a warm-up of every path, then ROUNDS alternated rounds, device events around whole
synchronised calls:
  ckpt  decode_logits_checkpointed at K                                        -- no emission tensor, a bounded workspace
  (a)   decode_logits with the whole delta history                             -- no emission tensor, 46 MB of history per song
  (b)   shaun_log_emissions into a [B, T, 361] tensor + decode_checkpointed at K -- a bounded workspace, 43 MB of emissions per song
  (c)   decode_logits on consecutive sub-batches whose whole history fits the bytes of ckpt's workspace -- the only way to meet
        such a budget without an emission tensor before vit_decode_logits_checkpointed existed
Writes one JSON document (OUT, default profiles/fused_ckpt_time.json): per (B, K) the milliseconds of every round, min and max, the
ratios of ckpt's median to the others' and whether the ranges are disjoint, the peak device memory of each path above the resident
logits (torch.cuda.max_memory_allocated, each path with its own allocations), and a bit-equality check of ckpt against (a).
BATCHES="1024" / ROUNDS=5 select a subset."""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from viterbi_spl_amd import ViterbiDecoder, synth
from viterbi_spl_amd import emissions as em

ROUNDS = int(os.environ.get("ROUNDS", "5"))
BATCHES = [int(b) for b in os.environ.get("BATCHES", "1024,2048").split(",")]
OUT = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fused_ckpt_time.json"))
T, S, P = 30000, 361, 32


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
    A, pi = bench.make_params("tonet", S, 14)
    dec = ViterbiDecoder(A, pi, dev)
    obs = ViterbiDecoder.obs_params("shaun", S - 1, 5, math.log(0.32 / 0.68), math.log(0.8 / 0.2), 2.0)
    X32 = synth.pitch_logits(P, T, S - 1, seed=5, device=dev)
    results = []
    for B in BATCHES:
        X = X32.repeat(B // P, 1, 1).contiguous()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        full = dec.workspace_bytes_logits(obs, B, T)
        picked = dec.plan_workspace_logits(obs, B, T, full // 8)["segment_frames"]
        for K in sorted({1024, picked}):
            need = dec.workspace_bytes_logits_checkpointed(obs, B, T, K)
            n_sub = max(n for n in range(1, B + 1) if dec.workspace_bytes_logits(obs, n, T) <= need)

            def sub_batches(ws):
                return [dec.decode_logits(X[s:s + n_sub], obs, out_dtype=torch.int32, workspace=ws) for s in range(0, B, n_sub)]

            def two_step(E, ws):
                return dec.decode_checkpointed(em.shaun_log_emissions(X, 0.32, 5, out=E), segment_frames=K, out_dtype=torch.int32, workspace=ws)
            # ---- peak memory above the logits, each path with its own allocations (these calls are also the warm-up)
            peak = {}
            for name, fn in (("ckpt", lambda: dec.decode_logits_checkpointed(X, obs, segment_frames=K, out_dtype=torch.int32)),
                             ("a_full_history", lambda: dec.decode_logits(X, obs, out_dtype=torch.int32)),
                             ("b_emissions_ckpt", lambda: two_step(None, None)),
                             ("c_sub_batches", lambda: sub_batches(None))):
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats(dev)
                fn()
                torch.cuda.synchronize()
                peak[name] = int(torch.cuda.max_memory_allocated(dev) - base)
                print(f"B {B} K {K}: peak of {name} {peak[name] / 1e9:.2f} GB", flush=True)
            torch.cuda.empty_cache()
            # ---- timed rounds on buffers allocated once; (a)'s history and (b)'s emission tensor share one buffer (never live together)
            e_bytes = B * T * S * 4
            big = torch.empty(max(full + 256, e_bytes), dtype=torch.uint8, device=dev)
            E = big[:e_bytes].view(torch.float32).view(B, T, S)
            ws_ck = torch.empty(need + 256, dtype=torch.uint8, device=dev)
            paths = (("ckpt", lambda: dec.decode_logits_checkpointed(X, obs, segment_frames=K, out_dtype=torch.int32, workspace=ws_ck)),
                     ("a_full_history", lambda: dec.decode_logits(X, obs, out_dtype=torch.int32, workspace=big)),
                     ("b_emissions_ckpt", lambda: two_step(E, ws_ck)),
                     ("c_sub_batches", lambda: sub_batches(ws_ck)))
            ms, out = {k: [] for k, _ in paths}, {}
            for k, fn in paths:
                timed(fn)
            for r in range(ROUNDS):
                for k, fn in paths:
                    t, o = timed(fn)
                    ms[k].append(round(t, 3))
                    if k in ("ckpt", "a_full_history"):
                        out[k] = o
                    del o
                print(f"B {B} K {K}: round {r} " + " ".join(f"{k} {v[-1]}" for k, v in ms.items()), flush=True)
            same = bool(torch.equal(out["ckpt"][0], out["a_full_history"][0]) and
                        torch.equal(out["ckpt"][1].view(torch.int32), out["a_full_history"][1].view(torch.int32)))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            rec = {"B": B, "T": T, "S": S, "segment_frames": K, "picked_for_an_eighth": K == picked, "rounds": ROUNDS,
                   "workspace_bytes": {"ckpt": need, "whole_history": full}, "songs_per_sub_batch": n_sub, "sub_batches": -(-B // n_sub),
                   "ms": ms, "ms_min_max": {k: [min(v), max(v)] for k, v in ms.items()}, "ms_median": med,
                   "ratio_ckpt_over": {k: round(med["ckpt"] / med[k], 3) for k in med if k != "ckpt"},
                   "ranges_disjoint_from_ckpt": {k: bool(min(ms[k]) > max(ms["ckpt"]) or max(ms[k]) < min(ms["ckpt"])) for k in med if k != "ckpt"},
                   "mframes_per_s": {k: round(B * T / (med[k] * 1e3), 1) for k in med},
                   "peak_bytes_above_logits": peak, "logits_bytes": int(X.numel() * 4), "bit_identical_to_full_history": same}
            print(json.dumps(rec), flush=True)
            results.append(rec)
            del out, E, big, ws_ck
            torch.cuda.empty_cache()
        del X
        torch.cuda.empty_cache()
    with open(OUT, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
