"""Randomised parity run (test infrastructure; run on the GPU box): the cases of tests/random_cases.py past any table --
case(seed, 0), case(seed, 1), ... -- each through tests/random_check.check_case, the per-case check of
tests/test_gpu_random_parity.py: every decode entry point against its reference bit for bit (the C restatement in oracle/, the
float64 restatement, the builder's rows, the commit and ring references), the served set against the size queries, refusals with
untouched outputs.  A failure prints the case id (seed, index), the entry point and its options: paste (seed, index) into the suite
or rerun it with random_cases.case(seed, index).  argv: seconds to run (default 240), seed (default 1)."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import random_cases as rc  # noqa: E402
from tests import random_check as ck  # noqa: E402
from viterbi_spl_amd import ViterbiDecoder  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 240.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
dev = torch.device("cuda:0")

t0 = time.time()
index = n_runs = 0
fails = []
while time.time() - t0 < budget:
    c = rc.case(seed, index)
    try:
        n_runs += ck.check_case(ViterbiDecoder(c["A"], c["pi"], dev), c, dev, guarded=index % 4 == 0)
    except AssertionError as e:
        fails.append((seed, index, str(e)))
        print("FAIL", e, flush=True)
    index += 1
    if index % 30 == 0:
        print(f"{index} cases, {n_runs} decodes, {len(fails)} failures, {time.time() - t0:.0f} s", flush=True)
print(f"done: seed {seed}, {index} cases, {n_runs} decodes, {len(fails)} failures")
sys.exit(1 if fails else 0)
