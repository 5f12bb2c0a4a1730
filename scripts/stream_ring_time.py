#!/usr/bin/env python3
"""Ring-session timing -> profiles/stream_ring_time.json.  One process, one warm-up round, five alternated rounds (ring first /
linear first), device events, min-max over the rounds (milliseconds).  tonet's 361-state grid, float32, one recording of 30000
frames of synth.emissions_peaks in appends of 768; the ring holds 2048 rows.

  (a) append      mean time of one vit_stream_append: ring session against linear session (the linear session runs the Stream kernels,
                  whose code this change leaves as it was: profiles/stream_ring_resources.txt)
  (b) commit      per append: vit_stream_commit_rel on the ring (the host-only vit_stream_commit_ack is outside the device time and is
                  reported as wall time) against vit_stream_commit on the linear session
  (c) finish      from the last append to the whole result: commit_rel + vit_stream_tail against commit + vit_stream_backtrace
  (d) workspace   bytes of the ring and of the linear session, for one recording and for 1024

    python scripts/stream_ring_time.py [--out profiles/stream_ring_time.json] [--frames 30000] [--ring 2048]
"""
import argparse
import json
import os
import sys
import time

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


def overlap(a, b):
    return a["min"] <= b["max"] and b["min"] <= a["max"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_ring_time.json"))
    ap.add_argument("--frames", type=int, default=30000)
    ap.add_argument("--append", type=int, default=768)
    ap.add_argument("--ring", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "stream_ring_time.py measures on the GPU; there is no fallback"
    dev = torch.device("cuda:0")
    T, S, R = args.frames, 361, args.ring
    dec = ViterbiDecoder(*synth.log_params(synth.tonet_transition(S - 1, 14), synth.floored_prior(S)), dev)
    sizes = [min(args.append, T - t) for t in range(0, T, args.append)]
    E = synth.emissions_peaks(1, T, S, seed=21, device=dev)
    chunks, t = [], 0
    for n in sizes:
        chunks.append(E[:, t:t + n].contiguous())
        t += n
    whole, wl = dec.decode(E, out_dtype=torch.int32)
    ring, lin = dec.stream(1, ring_frames=R), dec.stream(1, T)
    r_states = torch.empty((1, R), dtype=torch.int32, device=dev)
    r_first = torch.zeros((1,), dtype=torch.int64, device=dev)
    r_comm = torch.zeros((1,), dtype=torch.int64, device=dev)
    l_states = torch.empty((1, T), dtype=torch.int32, device=dev)
    l_comm = torch.zeros((1,), dtype=torch.int64, device=dev)
    l_full = torch.empty((1, T), dtype=torch.int32, device=dev)
    loglik = torch.empty((1,), dtype=torch.float32, device=dev)

    def run_ring(check):
        ring.reset()
        ap_ev, cm_ev, ack_s, parts = [], [], 0.0, []
        for k, c in enumerate(chunks):
            ap_ev.append(timed(lambda: ring.append(c)))
            last = k == len(chunks) - 1
            if last:
                fin = timed(lambda: (ring.commit_rel_into(r_states, r_first, r_comm), None))
            else:
                cm_ev.append(timed(lambda: ring.commit_rel_into(r_states, r_first, r_comm)))
            f0, f1 = int(r_first.item()), int(r_comm.item())          # (synchronises: the read a ring needs between appends)
            w0 = time.perf_counter()
            ring.ack([f1])
            ack_s += time.perf_counter() - w0
            if check:
                parts.append(r_states[0, :f1 - f0].clone())
            if last:
                tl = timed(lambda: ring.tail_into(r_states, r_first, loglik))
                torch.cuda.synchronize()
                if check:
                    parts.append(r_states[0, :T - f1].clone())
                    assert torch.equal(torch.cat(parts), whole[0]) and torch.equal(loglik.view(torch.int32), wl.view(torch.int32))
                finish = ms(fin) + ms(tl)
        return {"append": sum(ms(p) for p in ap_ev) / len(ap_ev), "commit": sum(ms(p) for p in cm_ev) / len(cm_ev), "finish": finish,
                "ack_wall": 1e3 * ack_s / len(chunks)}

    def run_lin(check):
        lin.reset()
        ap_ev, cm_ev = [], []
        for k, c in enumerate(chunks):
            ap_ev.append(timed(lambda: lin.append(c)))
            if k == len(chunks) - 1:
                fin = timed(lambda: (lin.commit_into(l_states, l_comm), lin.decode_into(l_full, loglik)))
            else:
                cm_ev.append(timed(lambda: lin.commit_into(l_states, l_comm)))
            torch.cuda.synchronize()                                  # (the same host rhythm as the ring's frontier read)
        if check:
            assert torch.equal(l_full, whole) and torch.equal(loglik.view(torch.int32), wl.view(torch.int32))
        return {"append": sum(ms(p) for p in ap_ev) / len(ap_ev), "commit": sum(ms(p) for p in cm_ev) / len(cm_ev), "finish": ms(fin)}

    run_ring(True)
    run_lin(True)                                                     # warm-up round, with the results checked
    rows = {"ring": [], "linear": []}
    for r in range(args.rounds):
        order = ("ring", "linear") if r % 2 == 0 else ("linear", "ring")
        for which in order:
            rows[which].append(run_ring(False) if which == "ring" else run_lin(False))
    out = {"device": torch.cuda.get_device_name(dev), "frames": T, "states": S, "append": args.append, "ring_rows": R, "rounds": args.rounds,
           "unit": "ms", "emissions": "peaks"}
    for key, a_name, b_name in (("append", "ring", "linear"), ("commit", "commit_rel", "commit"), ("finish", "commit_rel+tail", "commit+backtrace")):
        a, b = span([x[key] for x in rows["ring"]]), span([x[key] for x in rows["linear"]])
        out[key] = {a_name: a, b_name: b, "ranges_overlap": overlap(a, b)}
    out["commit"]["ack_wall_ms_per_append"] = span([x["ack_wall"] for x in rows["ring"]])
    out["workspace_bytes"] = {str(B): {"ring": dec.workspace_bytes_stream_ring(B, R), "linear": dec.workspace_bytes_stream(B, T)} for B in (1, 1024)}
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
