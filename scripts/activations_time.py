"""imm's activation front-end (vit_obs_activations) at full size: [B, 30000, 721] = B recordings of 30000 frames side by side in one
HF0 [721, B * 30000] matrix resident in HBM, fp32 and fp16 emission storage.  Device events around whole synchronised calls, a
warm-up round first, the variants alternating in one process.  Reports
  * the builder's time and its share of its own roofline: bytes = two reads of HF0 + one write of the emissions, over the
    measured float4-copy bandwidth of the MI355X (6.29 TB/s) and over the 8.0 TB/s datasheet figure;
  * HF0 -> path (builder + decode) against the decode alone on the same emissions;
  * the project's host ``process_HF0_fn`` on one core for ONE recording, for scale (the builder does B of them).
One JSON document to --out (default profiles/activations_time.json).  BATCH=64 / ROUNDS=3 select a smaller run."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viterbi_spl_amd import ImmViterbi, synth
from viterbi_spl_amd.emissions import activation_log_emissions

ROUNDS = int(os.environ.get("ROUNDS", "5"))
B = int(os.environ.get("BATCH", "256"))
T, U, P = 30000, 721, 16                  # P distinct recordings, repeated
COPY_TBS, SPEC_TBS = 6.29, 8.0


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "activations_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this script measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    torch.set_num_threads(1)
    vit = ImmViterbi(20, U, device=dev)
    dec = vit._decoder
    hf0 = torch.empty((U, B * T), dtype=torch.float32, device=dev)
    for b in range(min(P, B)):
        hf0[:, b * T:(b + 1) * T] = synth.hf0_activations(U, T, seed=500 + b, device=dev)
    for b in range(P, B):
        hf0[:, b * T:(b + 1) * T] = hf0[:, (b % P) * T:(b % P + 1) * T]
    offsets = torch.arange(B + 1, dtype=torch.int64, device=dev) * T
    report = {"B": B, "T": T, "U": U, "rounds": ROUNDS, "device": torch.cuda.get_device_name(dev)}
    for name, dt, esz in (("float32", torch.float32, 4), ("float16", torch.float16, 2)):
        E = torch.empty((B * T, U + 1), dtype=dt, device=dev)
        build = lambda: activation_log_emissions(hf0, offsets=offsets, out=E, dtype=dt)
        decode = lambda: dec.decode(E.view(B, T, U + 1), out_dtype=torch.int32)
        both = lambda: (build(), decode())[1]
        for fn in (build, decode, both):                 # warm-up (the decoder allocates its workspace here)
            timed(fn)
        ms = {"builder": [], "decode": [], "hf0_to_path": []}
        for r in range(ROUNDS):
            for k, fn in (("builder", build), ("decode", decode), ("hf0_to_path", both)):
                t, o = timed(fn)
                ms[k].append(round(t, 3))
                del o
        med = {k: float(np.median(v)) for k, v in ms.items()}
        nbytes = 2 * U * B * T * 4 + B * T * (U + 1) * esz
        report[name] = {
            "ms": ms, "median_ms": med, "builder_bytes": nbytes,
            "builder_TB_per_s": round(nbytes / med["builder"] / 1e9, 3),
            "builder_fraction_of_copy_bandwidth": round(nbytes / (COPY_TBS * 1e12) / (med["builder"] * 1e-3), 3),
            "builder_fraction_of_spec_bandwidth": round(nbytes / (SPEC_TBS * 1e12) / (med["builder"] * 1e-3), 3),
            "Mframes_per_s": {k: round(B * T / med[k] / 1e3, 1) for k in med},
            "hf0_to_path_over_decode": round(med["hf0_to_path"] / med["decode"], 3),
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
        }
        del E
        dec._ws = None
        torch.cuda.empty_cache()
    # the host front-end, one recording, one core
    x = hf0[:, :T].cpu().numpy()
    host = []
    for r in range(3):
        t0 = time.perf_counter()
        vit.process_HF0_fn(x)
        host.append(round((time.perf_counter() - t0) * 1e3, 2))
    report["host_process_HF0_fn_one_recording_ms"] = host
    report["host_process_HF0_fn_batch_estimate_ms"] = round(min(host) * B, 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
