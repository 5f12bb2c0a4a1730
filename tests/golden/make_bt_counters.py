#!/usr/bin/env python3
"""Record the back-trace event counters (``ViterbiDecoder.backtrace_counters``) of a few small, fixed decodes
(tests/golden/bt_counters.json, compared key by key by tests/test_gpu_bt_counters.py).

The counters are integer sums of per-wave counts: the same for any order in which the waves run.  They are behaviour the parity
tests only sample -- a chunk driver that repairs one chunk too many still decodes the right path.  Needs a GPU.  Run it only
where a count is MEANT to change; a refactor of the back-trace kernels must reproduce the file.

    python tests/golden/make_bt_counters.py [output.json]
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "bt_counters.json")

B, T = 3, 700
LENGTHS = (700, 333, 2)
CHUNKINGS = ((7, 0), (32, 1))              # (bt_chunks, bt_warm): no warm-up, most guesses wrong | one warm-up frame
# name -> (plan of params.npz, emission kind, seed, algo, options)
CASES = {
    "tonet361_full_form0": ("tonet361", "dense", 77, "wave", {"wave_history": 1, "backtrace_form": 0}),    # sparse fetch
    "tonet361_half": ("tonet361", "dense", 78, "wave", {"wave_history": 2}),                               # even rows only
    "tonet361_form2": ("tonet361", "ties", 79, "group", {"backtrace_form": 2}),                            # whole rows, lean
    "tonet361_form4": ("tonet361", "dense", 80, "group", {"backtrace_form": 4}),                           # one stream per lane
    "jdc722_form0": ("jdc722", "peaks", 81, "banded", {"backtrace_form": 0}),                              # sparse fetch, two slots
    "durrieu722_lazy": ("durrieu722", "dense", 82, "auto", {}),                                            # step plan: generic kernel
}


def case_inputs(name, dev):
    from viterbi_spl_amd import synth
    gen = {"peaks": synth.emissions_peaks, "dense": synth.emissions_dense, "ties": synth.emissions_ties}
    plan, kind, seed, _, _ = CASES[name]
    S = 722 if "722" in plan else 361
    E = gen[kind](B, T, S, seed=seed, device=dev)
    return E, torch.tensor(LENGTHS, dtype=torch.int64, device=dev)


def case_counters(dec, name, E, lens, check=None):
    """{"chunks|warm": counters} of one case; `check(states, loglik, key)` sees every decode."""
    _, _, _, algo, opts = CASES[name]
    out = {}
    for chunks, warm in CHUNKINGS:
        dec.set_option("reset", 0)
        for k, v in opts.items():
            dec.set_option(k, v)
        dec.set_option("bt_chunks", chunks)
        dec.set_option("bt_warm", warm)
        st, ll = dec.decode(E, lengths=lens, algo=algo, out_dtype=torch.int32)
        key = f"{chunks}|{warm}"
        out[key] = dec.backtrace_counters(B, T)
        if check is not None:
            check(st, ll, key)
    dec.set_option("reset", 0)
    return out


if __name__ == "__main__":
    from viterbi_spl_amd import ViterbiDecoder
    dev = torch.device("cuda:0")
    params = np.load(os.path.join(HERE, "params.npz"))
    rec = {}
    for name, (plan, *_rest) in CASES.items():
        dec = ViterbiDecoder(params[f"{plan}_logA_T"], params[f"{plan}_log_pi"], dev)
        E, lens = case_inputs(name, dev)
        rec[name] = case_counters(dec, name, E, lens)
        again = case_counters(dec, name, E, lens)
        assert again == rec[name], f"{name}: the counters differ between two runs: {rec[name]} / {again}"
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{out}: {len(rec)} cases")
    for name, v in rec.items():
        print(name, json.dumps(v, sort_keys=True))
