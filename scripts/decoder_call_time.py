#!/usr/bin/env python3
"""Host time per call of the decoder's entry points: what the Python layer costs, not what the kernels do.

    python scripts/decoder_call_time.py [--out result.json] [--calls 200] [--warmup 20]

Public API only, so that the same file times any commit.  B = 2, T = 64 on the tonet361 plan, a caller's workspace and preallocated
outputs wherever the method takes them: no allocation of a workspace and no synchronise falls inside a timed call.  Per row: the
median of `calls` host wall times (time.perf_counter around one call) after `warmup` calls, one device synchronise between rows.
Compare commits by interleaved runs (a, b, a, b): the gap between two runs of one commit is the spread a difference has to beat.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, T, K = 2, 64, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()

    import math
    from viterbi_spl_amd import ViterbiDecoder, decoder, synth
    dev = torch.device("cuda:0")
    p = np.load(os.path.join(ROOT, "tests", "golden", "params.npz"))
    dec = ViterbiDecoder(p["tonet361_logA_T"], p["tonet361_log_pi"], dev)
    S = dec.S
    E = synth.emissions_peaks(B, T, S, seed=3, device=dev)
    Ep = E.reshape(B * T, S).contiguous()
    off = np.arange(B + 1, dtype=np.int64) * T
    X = synth.pitch_logits(B, T, S - 1, seed=4, device=dev)
    obs = ViterbiDecoder.obs_params("shaun", S - 1, 5, math.log(0.32 / 0.68), math.log(0.8 / 0.2), 2.0)
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    loglik = torch.empty((B,), dtype=torch.float32, device=dev)

    def ws(need):
        return torch.empty(need + 256, dtype=torch.uint8, device=dev)

    i32 = dict(out_dtype=torch.int32)
    need_f64 = dec.workspace_bytes_f64(B, T)
    w = {"f64": ws(need_f64), "ck": ws(dec.workspace_bytes_checkpointed(B, T, K)), "f64_ck": ws(dec.workspace_bytes_f64_checkpointed(B, T, K)),
         "packed": ws(dec.workspace_bytes_packed(B, B * T)), "packed_ck": ws(dec.workspace_bytes_packed_checkpointed(off, K)),
         "packed_bd": ws(dec.workspace_bytes_packed_bounded(off, K)), "f64_packed": ws(dec.workspace_bytes_f64_packed(B, B * T)),
         "f64_packed_ck": ws(dec.workspace_bytes_f64_packed_checkpointed(off, K)), "logits": ws(dec.workspace_bytes_logits(obs, B, T)),
         "logits_ck": ws(dec.workspace_bytes_logits_checkpointed(obs, B, T, K))}
    n_appends = args.calls + args.warmup
    session = dec.stream(B, 4 * n_appends)
    chunk = E[:, :4].contiguous()
    commit_rows = torch.empty((B, 4 * n_appends), dtype=torch.int32, device=dev)
    committed = torch.zeros((B,), dtype=torch.int64, device=dev)

    rows = {
        "decode_into": lambda: dec.decode_into(E, states, loglik),
        "decode": lambda: dec.decode(E, **i32),
        "decode_f64": lambda: dec.decode_f64(E, workspace=w["f64"], **i32),
        "decode_f64(budget)": lambda: dec.decode_f64(E, workspace=w["f64"], max_workspace_bytes=need_f64, **i32),
        "decode_checkpointed": lambda: dec.decode_checkpointed(E, segment_frames=K, workspace=w["ck"], **i32),
        "decode_f64_checkpointed": lambda: dec.decode_f64_checkpointed(E, segment_frames=K, workspace=w["f64_ck"], **i32),
        "decode_packed": lambda: dec.decode_packed(Ep, off, workspace=w["packed"], **i32),
        "decode_packed_checkpointed": lambda: dec.decode_packed_checkpointed(Ep, off, segment_frames=K, workspace=w["packed_ck"], **i32),
        "decode_packed_bounded": lambda: dec.decode_packed_bounded(Ep, off, segment_frames=K, workspace=w["packed_bd"], **i32),
        "decode_f64_packed": lambda: dec.decode_f64_packed(Ep, off, workspace=w["f64_packed"], **i32),
        "decode_f64_packed_checkpointed": lambda: dec.decode_f64_packed_checkpointed(Ep, off, segment_frames=K, workspace=w["f64_packed_ck"], **i32),
        "decode_logits": lambda: dec.decode_logits(X, obs, workspace=w["logits"], **i32),
        "decode_logits_checkpointed": lambda: dec.decode_logits_checkpointed(X, obs, segment_frames=K, workspace=w["logits_ck"], **i32),
        "stream.append": lambda: session.append(chunk),
        "stream.commit_into": lambda: session.commit_into(commit_rows, committed),
    }
    result = {"B": B, "T": T, "S": S, "segment_frames": K, "calls": args.calls, "warmup": args.warmup, "unit": "us",
              "decoder_module": os.path.relpath(decoder.__file__, ROOT), "median_us": {}}
    for name, call in rows.items():
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize(dev)
        times = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
        torch.cuda.synchronize(dev)
        result["median_us"][name] = round(1e6 * statistics.median(times), 2)
    session.close()
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(result, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
