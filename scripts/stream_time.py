#!/usr/bin/env python3
"""Streaming decode timing -> profiles/stream_time.json.  One process, one warm-up round, five alternated rounds, device events,
min-max per figure (milliseconds).  tonet's 361-state grid, float32, recordings of 30000 frames, appends of 768 and of 1200 frames.

  tail_unstreamed   RecordingAccumulator(streaming=False): last append done -> finish() done (builder, forward, back-trace, maps)
  append / tail_streamed   RecordingAccumulator(streaming=True): every append (transpose, builder, forward over the chunk), and
                    last append done -> finish() done (back-trace, maps)
  forward_whole / appends_sum   one recording: vit_forward with forward_form 1 against the sum of the stream's append launches
  decode16 / stream16   16 recordings: decode() of the batch against all appends + decode() of one session

    python scripts/stream_time.py [--out profiles/stream_time.json] [--frames 30000]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from viterbi_spl_amd import synth  # noqa: E402
from viterbi_spl_amd import reference_api as ra  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    return (e0, e1), out


def ms(pair):
    return pair[0].elapsed_time(pair[1])


def span(xs):
    return {"min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_time.json"))
    ap.add_argument("--frames", type=int, default=30000)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "stream_time.py measures on the GPU; there is no fallback"
    dev = torch.device("cuda:0")
    T, U = args.frames, 360
    vit = ra.Viterbi(synth.tonet_transition(U, 14), synth.floored_prior(U + 1), device=dev)
    dec = vit._decoder
    result = {"device": torch.cuda.get_device_name(dev), "frames": T, "states": U + 1, "rounds": args.rounds, "unit": "ms", "chunks": {}}

    for chunk in (768, 1200):
        n_snip, F = (6, 128) if chunk == 768 else (1, 1200)
        n_batches = -(-T // chunk)
        pad_last = n_batches * chunk - T
        snips = [(torch.randn((n_snip, U + 1, F), generator=torch.Generator().manual_seed(k)) * 3.0).to(dev) for k in range(min(n_batches, 8))]
        accs = {False: ra.RecordingAccumulator(vit, T, streaming=False), True: ra.RecordingAccumulator(vit, T, streaming=True)}
        rows = {"tail_unstreamed": [], "tail_streamed": [], "append_mean": [], "append_max": [], "appends_sum": []}
        for rnd in range(args.rounds + 1):
            for streaming in (False, True):
                acc = accs[streaming]
                per = []
                for k in range(n_batches):
                    pair, _ = timed(lambda: acc.append(snips[k % len(snips)], pad_last if k == n_batches - 1 else 0))
                    per.append(pair)
                tail, out = timed(lambda: acc.finish())
                torch.cuda.synchronize()
                assert out[0].shape[0] == T
                if rnd == 0:
                    continue                                   # warm-up
                if streaming:
                    a = [ms(p) for p in per]
                    rows["tail_streamed"].append(ms(tail))
                    rows["append_mean"].append(sum(a) / len(a))
                    rows["append_max"].append(max(a))
                    rows["appends_sum"].append(sum(a))
                else:
                    rows["tail_unstreamed"].append(ms(tail))
        result["chunks"][str(chunk)] = {k: span(v) for k, v in rows.items()}
        result["chunks"][str(chunk)]["appends"] = n_batches

        # one recording: the stream's append launches alone against one forward pass (forward_form 1), and 16 recordings in one session
        for B, key in ((1, "one_recording"), (16, "sixteen_recordings")):
            E = synth.emissions_peaks(B, T, U + 1, seed=3, device=dev)
            st = dec.stream(B, T)
            states = torch.empty((B, T), dtype=torch.int32, device=dev)
            r = {"forward_whole": [], "appends_sum": [], "decode": [], "stream_total": []}
            for rnd in range(args.rounds + 1):
                dec.set_option("forward_form", 1)
                fw, _ = timed(lambda: dec.decode_into(E, states, algo="group", phase="forward"))
                dec.set_option("reset", 0)
                dc, _ = timed(lambda: dec.decode(E, out_dtype=torch.int32))
                st.reset()
                per = []
                for t in range(0, T, chunk):
                    c = E[:, t:t + chunk].contiguous()
                    per.append(timed(lambda: st.append(c))[0])
                bt, _ = timed(lambda: st.decode(out_dtype=torch.int32))
                torch.cuda.synchronize()
                if rnd == 0:
                    continue
                r["forward_whole"].append(ms(fw))
                r["decode"].append(ms(dc))
                r["appends_sum"].append(sum(ms(p) for p in per))
                r["stream_total"].append(sum(ms(p) for p in per) + ms(bt))
            st.close()
            result["chunks"][str(chunk)][key] = {k: span(v) for k, v in r.items()}
            del E

    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
