"""Shared helpers for the tests (input regeneration from the golden manifest)."""
import hashlib

import numpy as np
import torch

from viterbi_spl_amd import synth

GEN = {"peaks": synth.emissions_peaks, "dense": synth.emissions_dense, "ties": synth.emissions_ties,
       "scaled": synth.emissions_scaled}


def case_params(golden, case):
    p = golden["params"]
    return p[f"{case['params']}_logA_T"], p[f"{case['params']}_log_pi"]


def case_emissions(case, device="cpu", as_stored=False):
    """[T,S] emissions of a golden case.  as_stored=True keeps fp16 storage for f16 cases."""
    dt = torch.float16 if case["f16"] else torch.float32
    e = GEN[case["kind"]](1, case["T"], case["S"], seed=case["seed"], dtype=dt, device=device)[0]
    return e if as_stored else e.to(torch.float32)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def logits_case(seed, n_frames, n_bins):
    """Seeded pitch logits for the emission-builder tests: weak noise floor (unvoiced frames), melody-like
    bumps in two frames out of three, and some exactly tied values."""
    rng = np.random.default_rng(seed)
    x = rng.normal(-8.0, 1.5, (n_frames, n_bins)).astype(np.float32)
    for f in range(n_frames):
        if f % 3:
            c = int(rng.integers(8, n_bins - 8))
            x[f, c - 2:c + 3] += np.asarray([1.0, 3.0, 6.0, 3.0, 1.0], np.float32) * np.float32(rng.uniform(0.5, 2.5))
    x[:, ::37] = np.round(x[:, ::37])
    return x


# spans (nats below a frame's top logit) of the range-edge frames: e^-d is a normal float32 up to d ~ 87.3, a subnormal
# from there to ~103.3 (103.0 - 103.6 is left out: there the rounding to the smallest subnormal decides) and 0 beyond
RANGE_SPANS = (80, 86, 88, 90, 95, 100, 102, 106, 120)
RANGE_TOPS = (0, 10, -20, 37)


def range_edge_logits(n_bins, spw, tops=RANGE_TOPS, unvoiced_column=False):
    """Deterministic pitch logits at the float32 range edge of exp: integer values, a constant background 130 below the
    frame's top, and isolated peaks (2*spw + 2 bins apart, so that exactly these bins are peaks) at the top and at
    top - d for every d of RANGE_SPANS, rotated through the slots frame by frame.  The first slot is bin 0 (the left-end
    rule) or bin spw // 2 + 1 (the first bin past those that are never a peak).  -> float32 [n, n_bins].
    unvoiced_column=True: [n, n_bins + 1] with column 0 the unvoiced logit, 5 below the top, and one more frame per top and
    span in which the unvoiced logit is the far one (top - d)."""
    seq = (0,) + RANGE_SPANS
    rows, unv = [], []
    for top in tops:
        for start in (0, spw // 2 + 1):
            for r in range(len(seq)):
                x = np.full(n_bins, top - 130, np.float32)
                for j, b in enumerate(range(start, n_bins, 2 * spw + 2)):
                    x[b] = top - seq[(j + r) % len(seq)]
                rows.append(x)
                unv.append(top - 5)
        if unvoiced_column:
            for d in RANGE_SPANS:
                x = np.full(n_bins, top - 130, np.float32)
                x[spw + 1::2 * spw + 2] = top - 3
                x[spw + 1] = top
                rows.append(x)
                unv.append(top - d)
    x = np.stack(rows)
    if unvoiced_column:
        x = np.concatenate([np.asarray(unv, np.float32)[:, None], x], axis=1)
    return np.ascontiguousarray(x, np.float32)
