#!/usr/bin/env python3
"""Commit-point timing of a streaming session -> profiles/stream_commit_time.json.  One process, one warm-up round, five alternated
rounds (commit first / back-trace first), device events, min-max over the rounds (milliseconds).  tonet's 361-state grid, float32,
recordings of 30000 frames in appends of 768; one recording and sixteen; synth.emissions_peaks and synth.emissions_dense; no
lookback cap and a cap of 256 frames.

Per append: `commit` (vit_stream_commit of the new frames) against `backtrace` (vit_stream_backtrace of the recording as it stands:
the only way to a partial result without the commit point), the frames the merge walk went back and the frames committed (read
from the frontiers afterwards, not inside the timed region).  Per recording: the sums, and `tail` = the last append's commit plus
the whole back-trace that gives the frames behind the last frontier (there is no back-trace of a tail alone).

    python scripts/stream_commit_time.py [--out profiles/stream_commit_time.json] [--frames 30000]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from viterbi_spl_amd import ViterbiDecoder, synth  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def ms(pair):
    return pair[0].elapsed_time(pair[1])


def span(xs):
    return {"min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_commit_time.json"))
    ap.add_argument("--frames", type=int, default=30000)
    ap.add_argument("--append", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "stream_commit_time.py measures on the GPU; there is no fallback"
    dev = torch.device("cuda:0")
    T, S = args.frames, 361
    dec = ViterbiDecoder(*synth.log_params(synth.tonet_transition(S - 1, 14), synth.floored_prior(S)), dev)
    sizes = [min(args.append, T - t) for t in range(0, T, args.append)]
    result = {"device": torch.cuda.get_device_name(dev), "frames": T, "states": S, "append": args.append, "rounds": args.rounds,
              "unit": "ms", "cases": {}}
    for kind, gen in (("peaks", synth.emissions_peaks), ("dense", synth.emissions_dense)):
        for B in (1, 16):
            E = gen(B, T, S, seed=21, device=dev)
            whole, _ = dec.decode(E, out_dtype=torch.int32)
            st = dec.stream(B, T)
            states = torch.empty((B, T), dtype=torch.int32, device=dev)
            bt = torch.empty((B, T), dtype=torch.int32, device=dev)
            committed = torch.zeros((B,), dtype=torch.int64, device=dev)
            for cap in (None, 256):
                rows = {"commit_mean": [], "commit_max": [], "commit_sum": [], "backtrace_mean": [], "backtrace_max": [],
                        "backtrace_sum": [], "tail": []}
                walked = done = None
                for rnd in range(args.rounds + 1):
                    st.reset()
                    states.fill_(-5)
                    pc, pb, fronts = [], [], []
                    t = 0
                    for n in sizes:
                        st.append(E[:, t:t + n].contiguous())
                        t += n
                        for what in (("c", "b") if rnd % 2 else ("b", "c")):
                            if what == "c":
                                pc.append(timed(lambda: st.commit_into(states, committed, max_lookback=cap)))
                            else:
                                pb.append(timed(lambda: st.decode_into(bt, None)))
                        fronts.append(committed.clone())
                    torch.cuda.synchronize()
                    fr = torch.stack(fronts).cpu().numpy()                     # [appends, B]
                    for b in range(B):
                        k = int(fr[-1, b])
                        assert torch.equal(states[b, :k], whole[b, :k]) and bool((states[b, k:] == -5).all()), (kind, B, cap, b, k)
                    assert torch.equal(bt, whole)
                    if rnd == 0:
                        continue                                               # warm-up
                    c, b_ = [ms(p) for p in pc], [ms(p) for p in pb]
                    rows["commit_mean"].append(sum(c) / len(c))
                    rows["commit_max"].append(max(c))
                    rows["commit_sum"].append(sum(c))
                    rows["backtrace_mean"].append(sum(b_) / len(b_))
                    rows["backtrace_max"].append(max(b_))
                    rows["backtrace_sum"].append(sum(b_))
                    rows["tail"].append(c[-1] + b_[-1])
                    ends = torch.tensor(sizes).cumsum(0).numpy()[:, None]      # frames appended after each append
                    prev = fr.copy()
                    prev[1:], prev[0] = fr[:-1], 0
                    moved = fr > prev
                    back = (ends - fr) * moved + (~moved) * (ends - 1 - prev if cap is None else (ends - 1 - prev).clip(max=cap))
                    walked = {"mean": round(float(back.mean()), 2), "max": int(back.max())}
                    done = {"mean": round(float((fr - prev).mean()), 2), "min": int((fr - prev).min()), "max": int((fr - prev).max()),
                            "final_frontier_min": int(fr[-1].min()), "calls_without_commit": int((~moved).sum())}
                case = {k: span(v) for k, v in rows.items()}
                case["merge_frames_walked_per_append"] = walked
                case["frames_committed_per_append"] = done
                result["cases"][f"{kind}_B{B}_lookback_{'none' if cap is None else cap}"] = case
                print(kind, B, cap, json.dumps(case), flush=True)
            st.close()
            del E
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
