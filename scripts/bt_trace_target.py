#!/usr/bin/env python3
"""One small decode for a kernel trace of the back-trace launch sequence: tonet361, [4, 2000, 361], eight chunks per song.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 scripts/bt_trace_target.py

Two builds decode the same way when their traces list the same kernels, in the same order, with the same launch counts."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viterbi_spl_amd import ViterbiDecoder, synth  # noqa: E402

params = np.load(os.path.join(ROOT, "tests", "golden", "params.npz"))
dev = torch.device("cuda:0")
dec = ViterbiDecoder(params["tonet361_logA_T"], params["tonet361_log_pi"], dev)
E = synth.emissions_peaks(4, 2000, 361, seed=5, device=dev)
dec.set_option("bt_chunks", 8)
states, loglik = dec.decode(E, out_dtype=torch.int32)
torch.cuda.synchronize()
print("decoded", tuple(states.shape), int(states.sum()), dec.backtrace_counters(4, 2000))
