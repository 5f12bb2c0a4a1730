"""Forward pass of the one-target floor kernel (forward_form 1) against the split-window kernel (forward_form 6) in one
library, alternated: S = 361 and 321, fp32 and fp16 emissions, one and two songs per CU.  Decides the launcher's default.
usage: floor_split_ab.py [repeats]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viterbi_spl_amd import ViterbiDecoder, synth  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
dev = torch.device("cuda:0")
T = 30000
for S, dmax in ((361, 14), (321, 12)):
    A, pi = synth.log_params(synth.tonet_transition(S - 1, dmax), synth.floored_prior(S))
    dec = ViterbiDecoder(A, pi, dev)
    for dt in (torch.float32, torch.float16):
        base = synth.emissions_peaks(32, T, S, seed=1234, device=dev, dtype=dt)
        for B in (128, 256):
            E = base.repeat(B // 32, 1, 1).contiguous()
            st = torch.empty((B, T), dtype=torch.int32, device=dev)
            ll = torch.empty((B,), dtype=torch.float32, device=dev)
            res = {1: [], 6: []}
            for _ in range(reps):
                for form in (1, 6):
                    dec.set_option("forward_form", form)
                    dec.decode_into(E, st, ll, algo="group", phase="forward")
                    torch.cuda.synchronize()
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record()
                    for _ in range(5):
                        dec.decode_into(E, st, ll, algo="group", phase="forward")
                    ev[1].record()
                    torch.cuda.synchronize()
                    res[form].append(ev[0].elapsed_time(ev[1]) / 5)
            f = lambda v: " ".join(f"{x:.3f}" for x in v)
            print(f"S {S} {str(dt).split('.')[-1]} B {B}: one-target {f(res[1])} ms | split {f(res[6])} ms | "
                  f"split/one-target {min(res[6]) / min(res[1]):.4f}", flush=True)
            del E, st, ll
            dec._ws = None
            torch.cuda.empty_cache()
        del base
