"""Bounded packed decode of the 722-state grids (vit_decode_packed_bounded) at full size, against the three alternatives.

Workload: the set of scripts/packed_group_time.py -- S = 722, fp16 emissions, recordings with lengths uniform in [7500, 30000] until
256 x 30000 frames are reached (401 of them) -- for the jdc matrix (floor form) and the Durrieu matrix (step form).  One process;
timed per plan, alternating, device events around whole synchronised calls after a warm-up round:
  (a) decode_packed, full history (one delta row per frame);
  (b) decode_packed_bounded with segments of K = 1024 frames, in a caller-owned workspace;
  (c) decode_checkpointed(lengths=, segment_frames=1024) on the batch padded to 30000 frames;
  (d) what a caller can do without (b) under the budget of (b)'s workspace: greedy groups of consecutive recordings whose
      workspace_bytes_packed fits, one decode_packed per group into that workspace.
Writes one JSON object per plan (milliseconds of every round, medians, ranges, Mframes/s, workspace bytes, the throughput ratios
(b)/(a), (b)/(c) and (b)/(d), whether the results are the same bytes) to OUT (default profiles/packed_bounded_time.json)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

ROUNDS = int(os.environ.get("ROUNDS", "5"))
K = int(os.environ.get("SEGMENT_FRAMES", "1024"))
T, S = 30000, 722
TOTAL = int(os.environ.get("TOTAL_FRAMES", str(256 * T)))
PLANS = os.environ.get("PLANS", "jdc722,durrieu722").split(",")
OUT = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "packed_bounded_time.json"))


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
    N = int(off[-1])
    E_pad = bench.tiled_emissions(synth.emissions_peaks, B, T, S, 1234, dev, torch.float16)
    E_pk = torch.cat([E_pad[b, :lens[b]] for b in range(B)], dim=0).contiguous()
    lens_d = torch.from_numpy(lens).to(dev)
    results = []
    for name, (kind, dmax) in (("jdc722", ("tonet", 40)), ("durrieu722", ("durrieu", 0))):
        if name not in PLANS:
            continue
        A, pi = bench.make_params(kind, S, dmax)
        dec = ViterbiDecoder(A, pi, dev)
        need_full = dec.workspace_bytes_packed(B, N)
        need_b = dec.workspace_bytes_packed_bounded(off, K)
        need_c = dec.workspace_bytes_checkpointed(B, T, K)
        ws_full = torch.empty(need_full + 256, dtype=torch.uint8, device=dev)
        ws_b = torch.empty(need_b + 256, dtype=torch.uint8, device=dev)
        groups, g0 = [], 0                    # (d): consecutive recordings while the packed decode's workspace fits the budget of (b)
        for b in range(1, B + 1):
            if b == B or dec.workspace_bytes_packed(b + 1 - g0, int(off[b + 1] - off[g0])) > need_b:
                assert dec.workspace_bytes_packed(b - g0, int(off[b] - off[g0])) <= need_b, "one recording does not fit the budget"
                groups.append((g0, b))
                g0 = b

        def grouped():
            st = torch.empty((N,), dtype=torch.int32, device=dev)
            ll = torch.empty((B,), dtype=torch.float32, device=dev)
            for g0, g1 in groups:
                s, l = dec.decode_packed(E_pk[off[g0]:off[g1]], off[g0:g1 + 1] - off[g0], out_dtype=torch.int32, workspace=ws_b)
                st[off[g0]:off[g1]] = s
                ll[g0:g1] = l
            return st, ll

        runs = {
            "full": lambda: dec.decode_packed(E_pk, off, out_dtype=torch.int32, workspace=ws_full),
            "bounded": lambda: dec.decode_packed_bounded(E_pk, off, segment_frames=K, out_dtype=torch.int32, workspace=ws_b),
            "padded_checkpointed": lambda: dec.decode_checkpointed(E_pad, segment_frames=K, lengths=lens_d, out_dtype=torch.int32),
            "grouped": grouped,
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
        fs, fl = out["full"]
        same = all(bool(torch.equal(fs, out[k][0]) and torch.equal(fl.view(torch.int32), out[k][1].view(torch.int32))) for k in ("bounded", "grouped"))
        ps, pl = out["padded_checkpointed"]
        same = bool(same and torch.equal(pl.view(torch.int32), fl.view(torch.int32)) and
                    all(torch.equal(fs[off[b]:off[b + 1]], ps[b, :lens[b]]) for b in (0, B // 2, B - 1, int(np.argmin(lens)), int(np.argmax(lens)))))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        units = int(_lib.load().vit_packed_bounded_units(dec._plan, B))
        nseg = (lens + K - 1) // K

        def ratio(k):             # throughput of (b) over k: median, and the range over the rounds' extremes
            return {"median": round(med[k] / med["bounded"], 3),
                    "range": [round(min(ms[k]) / max(ms["bounded"]), 3), round(max(ms[k]) / min(ms["bounded"]), 3)]}

        results.append({
            "plan": name, "workload": f"{B} recordings, lengths uniform in [{T // 4}, {T}], {N} frames, S = {S}, fp16 emissions",
            "segment_frames": K, "rounds": ROUNDS, "ms": ms, "median_ms": med, "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()},
            "Mframes_per_s": {k: round(N / med[k] / 1e3, 1) for k in med},
            "workspace_bytes": {"full": need_full, "bounded": need_b, "padded_checkpointed": need_c, "grouped": need_b},
            "emission_bytes": {"packed": E_pk.numel() * 2, "padded": E_pad.numel() * 2},
            "pass2_launches": int(max(nseg.max(), -(-int(nseg.sum()) // units))), "units": int(nseg.sum()), "units_per_launch": units,
            "groups": len(groups), "recordings_per_group": [int(min(b - a for a, b in groups)), int(max(b - a for a, b in groups))],
            "bounded_over_full": ratio("full"), "bounded_over_padded_checkpointed": ratio("padded_checkpointed"),
            "bounded_over_grouped": ratio("grouped"), "same_bytes": same})
        print(json.dumps(results[-1]), flush=True)
        del dec, ws_full, ws_b, out, fs, fl, ps, pl
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write(json.dumps(results) + "\n")


if __name__ == "__main__":
    main()
