"""The emission builders with float16 storage (vit_obs_build) at the sizes the benchmark measures, against the only way to float16
emission rows there was before them.  Two shapes:
  tonet  [1024 x 30000, 360] logits, mode 0 ("shaun"), peak half-width 5, decoded on the wave form;
  jdc    [256 x 30000, 722] logits (unvoiced column first), mode 1 (softmax), half-width 15, decoded with algo="auto".
Four variants, each timed as the builder alone and as builder + decode:
  a  float32 logits -> float32 rows                          (the path every release has had)
  b  float32 logits -> float32 rows, then a torch cast of the emission tensor to float16 (copy_ into a float16 tensor kept across
     rounds: the pass .half() makes, without its allocation)  (float16 rows before this change)
  c  float32 logits -> float16 rows
  d  float16 logits -> float16 rows
One process, a warm-up round, ROUNDS (5) alternated rounds, device events around whole calls, min / median / max per variant.
Also: peak device memory above the resident logits of one builder + decode per variant with every buffer allocated inside it
(torch.cuda.max_memory_allocated), and the share of frames whose decoded state differs between a and c on these synthetic logits
(information for users, not a bar).  The script asserts nothing about a / c / d; it exits 1 when c does not beat b with disjoint ranges, builder alone and with the decode.
One JSON document to --out (default profiles/obs_half_time.json).  SCALE=8 divides both batch sizes (a smaller run)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from viterbi_spl_amd import ViterbiDecoder, synth
from viterbi_spl_amd import emissions as em

ROUNDS = int(os.environ.get("ROUNDS", "5"))
SCALE = int(os.environ.get("SCALE", "1"))
T, P = 30000, 16                           # P distinct songs, repeated
F32, F16 = torch.float32, torch.float16


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), out


def make_logits(B, U, unvoiced_column, dev):
    cols = U + (1 if unvoiced_column else 0)
    x = torch.empty((B, T, cols), dtype=F32, device=dev)
    for b in range(min(P, B)):
        x[b, :, cols - U:] = synth.pitch_logits(1, T, U, seed=700 + b, device=dev, voicing="segments")[0]
    if unvoiced_column:
        x[:, :, 0] = 0.0                    # (the pitch logits are relative to the unvoiced channel)
    for b in range(P, B):
        x[b] = x[b % P]
    return x


def shape_report(name, B, U, mode, spw, d_max, algo, dev):
    S = U + 1
    dec = ViterbiDecoder(*synth.log_params(synth.tonet_transition(U, d_max), synth.floored_prior(S)), dev)
    x32 = make_logits(B, U, mode == 1, dev)
    x16 = x32.half()
    n = B * T

    def build(x, out=None, dtype=F32):
        if mode == 0:
            return em.shaun_log_emissions(x, single_side_peak_width=spw, out=out, dtype=dtype)
        return em.softmax_log_emissions(x, single_side_peak_width=spw, out=out, dtype=dtype)

    def decode(E):
        return dec.decode(E, algo=algo, out_dtype=torch.int32)

    # ---- peak memory above the logits: every buffer of one builder + decode allocated inside the measured region
    def cast_path(x):
        return build(x).half()
    paths = {"a": lambda: decode(build(x32)), "b": lambda: decode(cast_path(x32)),
             "c": lambda: decode(build(x32, dtype=F16)), "d": lambda: decode(build(x16, dtype=F16))}
    peak, states = {}, {}
    for k, fn in paths.items():
        dec._ws = None
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        st, _ = fn()
        torch.cuda.synchronize()
        peak[k] = int(torch.cuda.max_memory_allocated(dev) - base)
        states[k] = st if k in ("a", "c") else None
        del st
    differ = float((states["a"] != states["c"]).float().mean())
    b_equals_c = None
    states = None
    dec._ws = None
    torch.cuda.empty_cache()

    # ---- times: the buffers kept across rounds
    E32 = torch.empty((B, T, S), dtype=F32, device=dev)
    E16 = torch.empty((B, T, S), dtype=F16, device=dev)

    def cast():
        build(x32, out=E32)
        return E16.copy_(E32)
    builders = {"a": lambda: build(x32, out=E32), "b": cast, "c": lambda: build(x32, out=E16, dtype=F16),
                "d": lambda: build(x16, out=E16, dtype=F16)}
    both = {k: (lambda k=k: decode(builders[k]())) for k in builders}
    for k in builders:                                     # warm-up (the decoder allocates its workspaces here)
        timed(builders[k])
        timed(both[k])
    cast()
    b_rows = E16.clone()
    builders["c"]()
    torch.cuda.synchronize()
    b_equals_c = bool(torch.equal(b_rows.view(torch.int16), E16.view(torch.int16)))
    del b_rows
    ms = {f"{k}_{w}": [] for k in builders for w in ("builder", "pipeline")}
    for r in range(ROUNDS):
        for k in builders:
            ms[f"{k}_builder"].append(round(timed(builders[k])[0], 3))
            t, o = timed(both[k])
            ms[f"{k}_pipeline"].append(round(t, 3))
            del o
    summ = {k: {"min": min(v), "median": float(np.median(v)), "max": max(v)} for k, v in ms.items()}
    rep = {
        "shape": [B, T, U + (mode == 1)], "mode": mode, "spw": spw, "algo": algo, "states": S, "frames": n,
        "ms": ms, "summary_ms": summ,
        "Mframes_per_s_median": {k: round(n / v["median"] / 1e3, 1) for k, v in summ.items()},
        "c_beats_b_disjoint": {w: summ[f"c_{w}"]["max"] < summ[f"b_{w}"]["min"] for w in ("builder", "pipeline")},
        "slower_than_a_disjoint": {f"{k}_{w}": summ[f"{k}_{w}"]["min"] > summ[f"a_{w}"]["max"] for k in ("c", "d") for w in ("builder", "pipeline")},
        "faster_than_a_disjoint": {f"{k}_{w}": summ[f"{k}_{w}"]["max"] < summ[f"a_{w}"]["min"] for k in ("c", "d") for w in ("builder", "pipeline")},
        "peak_bytes_above_logits": peak,
        "emission_tensor_bytes": {"float32": n * S * 4, "float16": n * S * 2},
        "share_of_frames_decoded_differently_a_vs_c": differ,
        "rows_of_b_equal_rows_of_c_bitwise": b_equals_c,
    }
    del E32, E16, x32, x16
    dec._ws = None
    torch.cuda.empty_cache()
    return name, rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "obs_half_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this script measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda:0")
    torch.set_num_threads(1)
    report = {"rounds": ROUNDS, "device": torch.cuda.get_device_name(dev), "scale": SCALE,
              "variants": {"a": "float32 logits -> float32 rows", "b": "a, then a torch cast of the rows to float16",
                           "c": "float32 logits -> float16 rows", "d": "float16 logits -> float16 rows"}}
    for name, B, U, mode, spw, d_max, algo in (("tonet", 1024 // SCALE, 360, 0, 5, 14, "wave"), ("jdc", 256 // SCALE, 721, 1, 15, 40, "auto")):
        k, rep = shape_report(name, B, U, mode, spw, d_max, algo, dev)
        report[k] = rep
        print(k, json.dumps(rep["summary_ms"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(json.dumps({k: {"c_beats_b_disjoint": report[k]["c_beats_b_disjoint"], "differ": report[k]["share_of_frames_decoded_differently_a_vs_c"]}
                      for k in ("tonet", "jdc")}))
    # the one condition: (b) does all of (a)'s work plus a pass over the emission tensor, so (c) must beat it everywhere
    lost = [f"{k} {w}" for k in ("tonet", "jdc") for w, ok in report[k]["c_beats_b_disjoint"].items() if not ok]
    if lost:
        print("float32 -> float16 does not beat builder + cast with disjoint ranges: " + ", ".join(lost), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
