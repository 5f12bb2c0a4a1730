"""Packed ragged decode of the 722-state grids (workgroup-form plans) at full size, against the two alternatives.

Workload: S = 722, fp16 emissions, recordings with lengths uniform in [7500, 30000], as many as hold 256 x 30000 frames, for the jdc
matrix (band of +/- 40, floor form) and the Durrieu matrix (step form).  Timed per plan, alternating, device events around whole
synchronised calls after a warm-up round:
  (i)   decode(lengths=) on the batch padded to 30000 frames -- the only way before the packed decode served these plans;
  (ii)  decode_packed on the packed buffer;
  (iii) decode of a uniform [256, 30000, 722] batch (the same number of real frames, no raggedness).
Prints one JSON line per plan: milliseconds of every round, medians, real Mframes/s, the ratios (ii)/(i) and (ii)/(iii) in
throughput, workspace and emission bytes, and a bit-exact spot check of the packed result against the padded one."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from viterbi_spl_amd import ViterbiDecoder, synth

ROUNDS = int(os.environ.get("ROUNDS", "5"))
T = 30000
S = 722
TOTAL = 256 * T


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
    rng = np.random.default_rng(7)
    lens, left = [], TOTAL
    while left > 0:
        n = min(int(rng.integers(T // 4, T + 1)), left)
        lens.append(n)
        left -= n
    lens = np.asarray(lens, np.int64)
    B = len(lens)
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum(lens)
    E_pad = bench.tiled_emissions(synth.emissions_peaks, B, T, S, 1234, dev, torch.float16)
    E_pk = torch.cat([E_pad[b, :lens[b]] for b in range(B)], dim=0).contiguous()
    E_uni = E_pad[:256]
    lens_d = torch.from_numpy(lens).to(dev)
    for name, (kind, dmax) in (("jdc722", ("tonet", 40)), ("durrieu722", ("durrieu", 0))):
        A, pi = bench.make_params(kind, S, dmax)
        dec = ViterbiDecoder(A, pi, dev)
        need_pk = dec.workspace_bytes_packed(B, int(off[-1]))
        need_pad = dec.workspace_bytes(B, T, "auto")
        ws = torch.empty(need_pk + 256, dtype=torch.uint8, device=dev)
        runs = {
            "padded": lambda: dec.decode(E_pad, lengths=lens_d, out_dtype=torch.int32),
            "packed": lambda: dec.decode_packed(E_pk, off, out_dtype=torch.int32, workspace=ws),
            "uniform": lambda: dec.decode(E_uni, out_dtype=torch.int32),
        }
        ms = {k: [] for k in runs}
        out = {}
        for r in range(ROUNDS + 1):                       # round 0 warms up
            for k, fn in runs.items():
                t, o = timed(fn)
                if r > 0:
                    ms[k].append(round(t, 3))
                if k != "uniform":
                    out[k] = o
                del o
        ps, pl = out["padded"]
        ks, kl = out["packed"]
        same = all(torch.equal(ks[off[b]:off[b + 1]], ps[b, :lens[b]]) for b in (0, B // 2, B - 1, int(np.argmin(lens)), int(np.argmax(lens))))
        same = bool(same and torch.equal(kl, pl))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        frames = {"padded": int(off[-1]), "packed": int(off[-1]), "uniform": 256 * T}
        print(json.dumps({
            "plan": name, "songs": int(B), "real_frames": int(off[-1]), "rounds": ROUNDS, "ms": ms, "median_ms": med,
            "spread_padded_ms": [min(ms["padded"]), max(ms["padded"])],
            "Mframes_per_s": {k: round(frames[k] / med[k] / 1e3, 1) for k in med},
            "packed_over_padded": round(med["padded"] / med["packed"], 3),
            "packed_over_uniform": round((frames["packed"] / med["packed"]) / (frames["uniform"] / med["uniform"]), 3),
            "workspace_GB": {"padded": round(need_pad / 1e9, 2), "packed": round(need_pk / 1e9, 2)},
            "emissions_GB": {"padded": round(E_pad.numel() * 2 / 1e9, 2), "packed": round(E_pk.numel() * 2 / 1e9, 2)},
            "packed_equals_padded_sample": same}), flush=True)
        del dec, ws, out, ps, pl, ks, kl
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
