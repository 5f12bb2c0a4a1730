"""Packed ragged float64 decode (decode_f64_packed) at full size, against the two alternatives.

Workloads: recordings with lengths uniform in [7500, 30000], as many as hold the frame budget (the recipe of packed_group_time.py):
  jdc722_fp16    S = 722, fp16 emissions, the jdc matrix, 256 x 30000 frames;
  tonet361_fp32  S = 361, fp32 emissions, the tonet matrix, 128 x 30000 frames.
Timed per grid, alternating, device events around whole synchronised calls after a warm-up round:
  (i)   decode_f64(lengths=) on the batch padded to 30000 frames -- the only way before the packed decode;
  (ii)  decode_f64_packed on the packed buffer;
  (iii) decode_f64 of a uniform batch of the same frame count (no raggedness).
One JSON document to --out (default profiles/f64_packed_time.json): per grid the milliseconds of every round, medians and ranges, real
Mframes/s, the ratios (ii)/(i) and (ii)/(iii) in throughput with the ranges the rounds span, whether the ranges of (i) and (ii) are
disjoint, workspace and emission bytes, and a bit-exact check of (ii) against (i) over every recording."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from viterbi_spl_amd import ViterbiDecoder, synth

ROUNDS = int(os.environ.get("ROUNDS", "5"))
T = 30000


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), out


def ragged_lengths(total, seed=7):
    rng = np.random.default_rng(seed)
    lens, left = [], total
    while left > 0:
        n = min(int(rng.integers(T // 4, T + 1)), left)
        lens.append(n)
        left -= n
    return np.asarray(lens, np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f64_packed_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this script measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    params = np.load(os.path.join(ROOT, "tests", "golden", "params.npz"))
    report = {"T": T, "rounds": ROUNDS, "device": torch.cuda.get_device_name(dev)}
    for name, key, S, dt, uni in (("jdc722_fp16", "jdc722", 722, torch.float16, 256), ("tonet361_fp32", "tonet361", 361, torch.float32, 128)):
        lens = ragged_lengths(uni * T)
        B = len(lens)
        off = np.zeros(B + 1, np.int64)
        off[1:] = np.cumsum(lens)
        N = int(off[-1])
        A, pi = params[f"{key}_logA_T"], params[f"{key}_log_pi"]
        dec = ViterbiDecoder(A, pi, dev)
        E_pad = bench.tiled_emissions(synth.emissions_peaks, B, T, S, 1234, dev, dt)
        E_pk = torch.cat([E_pad[b, :lens[b]] for b in range(B)], dim=0).contiguous()
        E_uni = E_pad[:uni]
        lens_d = torch.from_numpy(lens).to(dev)
        need_pk = dec.workspace_bytes_f64_packed(B, N)
        need_pad = dec.workspace_bytes_f64(B, T)
        ws = torch.empty(need_pk + 256, dtype=torch.uint8, device=dev)
        runs = {
            "padded": lambda: dec.decode_f64(E_pad, lengths=lens_d, out_dtype=torch.int32),
            "packed": lambda: dec.decode_f64_packed(E_pk, off, out_dtype=torch.int32, workspace=ws),
            "uniform": lambda: dec.decode_f64(E_uni, out_dtype=torch.int32),
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
        same = all(torch.equal(ks[off[b]:off[b + 1]], ps[b, :lens[b]]) for b in range(B))
        same = bool(same and torch.equal(kl.view(torch.int64), pl.view(torch.int64)))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        rng_ms = {k: [min(v), max(v)] for k, v in ms.items()}
        frames = {"padded": N, "packed": N, "uniform": uni * T}
        isz = E_pad.element_size()
        report[name] = {
            "S": S, "window": int(dec.info["group_window"]), "songs": int(B), "real_frames": N, "uniform_songs": uni,
            "ms": ms, "median_ms": med, "range_ms": rng_ms,
            "Mframes_per_s": {k: round(frames[k] / med[k] / 1e3, 2) for k in med},
            "packed_over_padded": round(med["padded"] / med["packed"], 3),
            "packed_over_padded_range": [round(rng_ms["padded"][0] / rng_ms["packed"][1], 3), round(rng_ms["padded"][1] / rng_ms["packed"][0], 3)],
            "ranges_disjoint_packed_below_padded": bool(rng_ms["packed"][1] < rng_ms["padded"][0]),
            "packed_over_uniform": round((frames["packed"] / med["packed"]) / (frames["uniform"] / med["uniform"]), 3),
            "packed_over_uniform_range": [round((N / rng_ms["packed"][1]) / (uni * T / rng_ms["uniform"][0]), 3),
                                          round((N / rng_ms["packed"][0]) / (uni * T / rng_ms["uniform"][1]), 3)],
            "workspace_GB": {"padded": round(need_pad / 1e9, 2), "packed": round(need_pk / 1e9, 2)},
            "emissions_GB": {"padded": round(E_pad.numel() * isz / 1e9, 2), "packed": round(E_pk.numel() * isz / 1e9, 2)},
            "packed_equals_padded_every_recording": same}
        print(json.dumps({name: report[name]}), flush=True)
        del dec, ws, out, ps, pl, ks, kl, E_pad, E_pk, E_uni, runs
        torch.cuda.empty_cache()
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
