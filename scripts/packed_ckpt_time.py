"""Packed checkpointed decode (vit_decode_packed_checkpointed) at full size, against the packed decode with the full history and
against host-side grouping under the same workspace budget.

Workload: the ragged row of bench.py -- recordings with lengths uniform in [7500, 30000] until 61.44 M frames are reached (3250 of
them), S = 361 (tonet matrix), fp32 emissions in ONE packed buffer.  Timed alternating, device events around whole synchronised
calls after a warm-up round:
  (a) decode_packed, full history (one delta row per frame);
  (b) decode_packed_checkpointed with segments of K = 1024 frames, in a caller-owned workspace;
  (c) what a caller can do without (b) under the budget of (b)'s workspace: greedy groups of consecutive recordings whose
      workspace_bytes_packed fits, one decode_packed per group into that workspace.
Writes one JSON object (milliseconds of every round, medians, Mframes/s, workspace bytes, the ratios (b)/(a) and (b)/(c) in
throughput, whether the three results are the same bytes) to OUT (default profiles/packed_ckpt_time.json) and prints it."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from viterbi_spl_amd import ViterbiDecoder, synth

ROUNDS = int(os.environ.get("ROUNDS", "5"))
K = int(os.environ.get("SEGMENT_FRAMES", "1024"))
T, TOTAL, S = 30000, int(os.environ.get("TOTAL_FRAMES", str(2048 * 30000))), 361
OUT = os.environ.get("OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "packed_ckpt_time.json"))


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), out


def ragged_lengths(total, seed=7):
    """bench.packed_row's lengths: uniform in [T/4, T] until `total` frames are reached."""
    rng = np.random.default_rng(seed)
    lens, left = [], total
    while left > 0:
        n = min(int(rng.integers(T // 4, T + 1)), left)
        lens.append(n)
        left -= n
    return np.asarray(lens, np.int64)


def main():
    dev = torch.device("cuda:0")
    A, pi = bench.make_params("tonet", S, 14)
    dec = ViterbiDecoder(A, pi, dev)
    lens = ragged_lengths(TOTAL)
    B = len(lens)
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum(lens)
    N = int(off[-1])
    base = synth.emissions_peaks(32, T, S, seed=1234, device=dev)
    E = torch.empty((N, S), dtype=torch.float32, device=dev)
    for b in range(B):
        E[off[b]:off[b + 1]] = base[b % 32, :lens[b]]
    del base
    need_full = dec.workspace_bytes_packed(B, N)
    need_ck = dec.workspace_bytes_packed_checkpointed(off, K)
    ws_full = torch.empty(need_full + 256, dtype=torch.uint8, device=dev)
    ws_ck = torch.empty(need_ck + 256, dtype=torch.uint8, device=dev)
    groups, g0 = [], 0                    # (c): consecutive recordings while the packed decode's workspace fits the budget of (b)
    for b in range(1, B + 1):
        if b == B or dec.workspace_bytes_packed(b + 1 - g0, int(off[b + 1] - off[g0])) > need_ck:
            assert dec.workspace_bytes_packed(b - g0, int(off[b] - off[g0])) <= need_ck, "one recording does not fit the budget"
            groups.append((g0, b))
            g0 = b

    def grouped():
        st = torch.empty((N,), dtype=torch.int32, device=dev)
        ll = torch.empty((B,), dtype=torch.float32, device=dev)
        for g0, g1 in groups:
            s, l = dec.decode_packed(E[off[g0]:off[g1]], off[g0:g1 + 1] - off[g0], out_dtype=torch.int32, workspace=ws_ck)
            st[off[g0]:off[g1]] = s
            ll[g0:g1] = l
        return st, ll

    runs = {
        "full": lambda: dec.decode_packed(E, off, out_dtype=torch.int32, workspace=ws_full),
        "checkpointed": lambda: dec.decode_packed_checkpointed(E, off, segment_frames=K, out_dtype=torch.int32, workspace=ws_ck),
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
    same = all(bool(torch.equal(out["full"][0], out[k][0]) and torch.equal(out["full"][1].view(torch.int32), out[k][1].view(torch.int32)))
               for k in ("checkpointed", "grouped"))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    n_units = min(B, 8 * torch.cuda.get_device_properties(dev).multi_processor_count)
    nseg = (lens + K - 1) // K
    res = {
        "workload": f"{B} recordings, lengths uniform in [{T // 4}, {T}], {N} frames, S = {S}, fp32 emissions, packed",
        "segment_frames": K, "rounds": ROUNDS, "ms": ms, "median_ms": med,
        "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()},
        "Mframes_per_s": {k: round(N / med[k] / 1e3, 1) for k in med},
        "workspace_bytes": {"full": need_full, "checkpointed": need_ck, "grouped": need_ck},
        "pass2_launches": int(max(nseg.max(), -(-int(nseg.sum()) // n_units))), "units": int(nseg.sum()), "units_per_launch": int(n_units),
        "groups": len(groups), "recordings_per_group": [int(min(b - a for a, b in groups)), int(max(b - a for a, b in groups))],
        "checkpointed_over_full": round(med["full"] / med["checkpointed"], 3),
        "checkpointed_over_grouped": round(med["grouped"] / med["checkpointed"], 3),
        "same_bytes": same,
    }
    text = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
