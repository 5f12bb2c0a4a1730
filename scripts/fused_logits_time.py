"""Fused logits -> path decode (vit_decode_logits) at full size, against the two-step path it replaces.

Workload: [B, 30000, 360] "shaun" logits resident in HBM, S = 361 (the tonet matrix), songs repeating with period 32 (bench.py's
pipeline block), both voicing patterns, B in {256, 512, 1024, 2048}.  Timed per B, alternating in one process after a warm-up round,
device events around whole synchronised calls:
  (i)  shaun_log_emissions into a preallocated [B, T, 361] buffer + decode(algo="auto") -- what the ratio is measured against;
  (ii) decode_logits with emissions_out=None (no emission tensor exists).
Prints one JSON line per (B, voicing): milliseconds of every round, medians, Mframes/s, the ratio (ii)/(i) in time, the spread of (i)
across its own rounds (a difference smaller than that is not a finding), peak device memory of each path above the resident logits,
and a bit-equality spot check.  BATCHES="256,1024" / VOICINGS="toggle" / ROUNDS=5 select a subset."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from viterbi_spl_amd import ViterbiDecoder, synth
from viterbi_spl_amd import emissions as em
from viterbi_spl_amd import reference_api as ra

ROUNDS = int(os.environ.get("ROUNDS", "5"))
BATCHES = [int(b) for b in os.environ.get("BATCHES", "256,512,1024,2048").split(",")]
VOICINGS = os.environ.get("VOICINGS", "toggle,segments").split(",")
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
    import math
    obs = ViterbiDecoder.obs_params("shaun", S - 1, 5, math.log(0.32 / 0.68), math.log(0.8 / 0.2), 2.0)
    for voicing in VOICINGS:
        X32 = synth.pitch_logits(P, T, S - 1, seed=5, device=dev, voicing=voicing)
        for B in BATCHES:
            X = X32.repeat(B // P, 1, 1).contiguous()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            peak, ms, out = {}, {"two_step": [], "fused": []}, {}
            # peak memory of (ii) with its own allocations only, then of (i); the timed rounds share the decoder's workspace (both paths
            # keep a full wave-layout history of the same size), so that 2048 songs and their emission tensor fit one device
            ws = torch.empty(dec.workspace_bytes_logits(obs, B, T) + 256, dtype=torch.uint8, device=dev)
            torch.cuda.reset_peak_memory_stats(dev)
            timed(lambda: dec.decode_logits(X, obs, out_dtype=torch.int32, workspace=ws))
            peak["fused"] = torch.cuda.max_memory_allocated(dev) - base
            del ws
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            E = torch.empty((B, T, S), dtype=torch.float32, device=dev)
            two = lambda: dec.decode(em.shaun_log_emissions(X, 0.32, 5, out=E), algo="auto", out_dtype=torch.int32)
            timed(two)                                    # (the decoder allocates its workspace here: this round warms up)
            peak["two_step"] = torch.cuda.max_memory_allocated(dev) - base
            if dec._ws.numel() < dec.workspace_bytes_logits(obs, B, T) + 256:      # (the workgroup form's rows are narrower: 364 floats)
                dec._ws = None
                dec._ws = torch.empty(dec.workspace_bytes_logits(obs, B, T) + 256, dtype=torch.uint8, device=dev)
            ws = dec._ws
            fused = lambda: dec.decode_logits(X, obs, out_dtype=torch.int32, workspace=ws)
            timed(fused)
            for r in range(ROUNDS):
                for k, fn in (("two_step", two), ("fused", fused)):
                    t, o = timed(fn)
                    ms[k].append(round(t, 3))
                    out[k] = o
                    del o
            same = bool(torch.equal(out["two_step"][0], out["fused"][0]) and
                        torch.equal(out["two_step"][1].view(torch.int32), out["fused"][1].view(torch.int32)))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            print(json.dumps({
                "B": B, "T": T, "voicing": voicing, "rounds": ROUNDS, "forward_family_two_step": dec.forward_family(B), "ms": ms, "median_ms": med,
                "Mframes_per_s": {k: round(B * T / med[k] / 1e3, 1) for k in med},
                "fused_over_two_step_time": round(med["fused"] / med["two_step"], 4),
                "two_step_spread": round((max(ms["two_step"]) - min(ms["two_step"])) / med["two_step"], 4),
                "peak_GB_above_logits": {k: round(v / 1e9, 2) for k, v in peak.items()},
                "emission_tensor_GB": round(B * T * S * 4 / 1e9, 2),
                "fused_equals_two_step": same}), flush=True)
            del ws, E, X, out, fused, two
            dec._ws = None
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
