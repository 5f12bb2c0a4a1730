#!/usr/bin/env python3
"""Record what every budgeted, packed, float64, fused-logits and session entry of ``ViterbiDecoder`` answers on a plan that serves
none of them (``dense97`` of params.npz: an unstructured matrix): the exception type with its full text, or the returned value
(tests/golden/decoder_unserved.json, compared exactly by tests/test_gpu_decoder_calls.py).  The texts and which size queries
raise and which answer 0 are part of the call surface.  Needs a GPU.  Run it only where an answer is MEANT to change; a refactor
of the host layer must reproduce the file.

    python tests/golden/make_decoder_unserved.py [output.json]
"""
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "decoder_unserved.json")

PLAN = "dense97"
B, T, K = 3, 130, 64
LENGTHS = (130, 1, 67)
BUDGET = 1000                                   # bytes: below every need, so that each plan_workspace_* has to look for a fit


def shaun_obs(n_bins):
    from viterbi_spl_amd import ViterbiDecoder
    return ViterbiDecoder.obs_params("shaun", n_bins, 5, math.log(0.32 / 0.68), math.log(0.8 / 0.2), 2.0)


def inputs(S, dev, seed=5):
    """(E [B, T, S], lengths, packed rows, host offsets, logits [B, T, S - 1], obs) -- the shapes of tests/test_gpu_decoder_calls.py."""
    from viterbi_spl_amd import synth
    E = synth.emissions_peaks(B, T, S, seed=seed, device=dev)
    lens = torch.tensor(LENGTHS, dtype=torch.int64, device=dev)
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    Ep = torch.cat([E[b, :n] for b, n in enumerate(LENGTHS)], dim=0).contiguous()
    X = synth.pitch_logits(B, T, S - 1, seed=seed + 1, device=dev)
    return E, lens, Ep, off, X, shaun_obs(S - 1)


def _answer(fn):
    try:
        got = fn()
    except Exception as e:                      # (the type is part of the record)
        return {"raises": type(e).__name__, "text": str(e)}
    if isinstance(got, tuple) and all(isinstance(x, torch.Tensor) for x in got):
        return {"returns": [[str(x.dtype), list(x.shape)] for x in got]}
    if got.__class__.__name__ == "DecodeStream":
        got.close()
        return {"returns": "DecodeStream"}
    return {"returns": got}


def record(dec, dev):
    """name -> answer of every entry on decoder `dec`; the generator and the test share this function."""
    E, lens, Ep, off, X, obs = inputs(dec.S, dev)
    N = int(off[-1])
    calls = {
        "workspace_bytes": lambda: dec.workspace_bytes(B, T),
        "workspace_bytes(wave)": lambda: dec.workspace_bytes(B, T, "wave"),
        "workspace_bytes_checkpointed": lambda: dec.workspace_bytes_checkpointed(B, T, K),
        "workspace_bytes_checkpointed_or_zero": lambda: dec.workspace_bytes_checkpointed_or_zero(B, T, K),
        "workspace_bytes_f64": lambda: dec.workspace_bytes_f64(B, T),
        "workspace_bytes_f64_checkpointed": lambda: dec.workspace_bytes_f64_checkpointed(B, T, K),
        "workspace_bytes_f64_packed": lambda: dec.workspace_bytes_f64_packed(B, N),
        "workspace_bytes_f64_packed_checkpointed": lambda: dec.workspace_bytes_f64_packed_checkpointed(off, K),
        "workspace_bytes_packed": lambda: dec.workspace_bytes_packed(B, N),
        "workspace_bytes_packed_checkpointed": lambda: dec.workspace_bytes_packed_checkpointed(off, K),
        "workspace_bytes_packed_bounded": lambda: dec.workspace_bytes_packed_bounded(off, K),
        "workspace_bytes_logits": lambda: dec.workspace_bytes_logits(obs, B, T),
        "workspace_bytes_logits_checkpointed": lambda: dec.workspace_bytes_logits_checkpointed(obs, B, T, K),
        "workspace_bytes_stream": lambda: dec.workspace_bytes_stream(2, 64),
        "workspace_bytes_stream_ring": lambda: dec.workspace_bytes_stream_ring(2, 64),
        "decode(budget)": lambda: dec.decode(E, lengths=lens, max_workspace_bytes=BUDGET),
        "decode_checkpointed": lambda: dec.decode_checkpointed(E, segment_frames=K, lengths=lens),
        "decode_f64": lambda: dec.decode_f64(E, lengths=lens),
        "decode_f64(budget)": lambda: dec.decode_f64(E, lengths=lens, max_workspace_bytes=BUDGET),
        "decode_f64_checkpointed": lambda: dec.decode_f64_checkpointed(E, segment_frames=K, lengths=lens),
        "decode_f64_packed": lambda: dec.decode_f64_packed(Ep, off),
        "decode_f64_packed(budget)": lambda: dec.decode_f64_packed(Ep, off, max_workspace_bytes=BUDGET),
        "decode_f64_packed_checkpointed": lambda: dec.decode_f64_packed_checkpointed(Ep, off, segment_frames=K),
        "decode_f64_packed_bounded": lambda: dec.decode_f64_packed_bounded(Ep, off),
        "decode_f64_packed_bounded(budget)": lambda: dec.decode_f64_packed_bounded(Ep, off, max_workspace_bytes=BUDGET),
        "decode_packed": lambda: dec.decode_packed(Ep, off),
        "decode_packed(budget)": lambda: dec.decode_packed(Ep, off, max_workspace_bytes=BUDGET),
        "decode_packed_checkpointed": lambda: dec.decode_packed_checkpointed(Ep, off, segment_frames=K),
        "decode_packed_bounded": lambda: dec.decode_packed_bounded(Ep, off, segment_frames=K),
        "decode_logits": lambda: dec.decode_logits(X, obs, lengths=lens),
        "decode_logits(budget)": lambda: dec.decode_logits(X, obs, lengths=lens, max_workspace_bytes=BUDGET),
        "decode_logits_checkpointed": lambda: dec.decode_logits_checkpointed(X, obs, segment_frames=K, lengths=lens),
        "plan_workspace(budget)": lambda: dec.plan_workspace(B, T, "auto", BUDGET),
        "plan_workspace_f64(budget)": lambda: dec.plan_workspace_f64(B, T, BUDGET),
        "plan_workspace_f64_packed(budget)": lambda: dec.plan_workspace_f64_packed(off, BUDGET),
        "plan_workspace_f64_packed_bounded(budget)": lambda: dec.plan_workspace_f64_packed_bounded(off, BUDGET),
        "plan_workspace_logits(budget)": lambda: dec.plan_workspace_logits(obs, B, T, BUDGET),
        "plan_workspace_packed(budget)": lambda: dec.plan_workspace_packed(off, BUDGET),
        "plan_workspace_packed_bounded(budget)": lambda: dec.plan_workspace_packed_bounded(off, BUDGET),
        "stream(2, 64)": lambda: dec.stream(2, 64),
        "stream(2, ring_frames=64)": lambda: dec.stream(2, ring_frames=64),
    }
    rec = {name: _answer(fn) for name, fn in calls.items()}
    torch.cuda.synchronize(dev)
    return rec


if __name__ == "__main__":
    from viterbi_spl_amd import ViterbiDecoder
    dev = torch.device("cuda:0")
    params = np.load(os.path.join(HERE, "params.npz"))
    rec = record(ViterbiDecoder(params[f"{PLAN}_logA_T"], params[f"{PLAN}_log_pi"], dev), dev)
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{out}: {len(rec)} entries, {sum('raises' in v for v in rec.values())} raise")
    for name, v in rec.items():
        print(name, json.dumps(v, sort_keys=True))
