"""Emission builders on the GPU: pitch logits -> log observation probabilities.

The reference builds the observation probabilities of a song with Python loops over its frames on the
host (``Viterbi.observation_probs_fn`` tonet/for_paper.py:1733-1778, ``SoftMaxViterbi.observation_probs_fn``
:1911-1944) and takes ``log(p + tiny)`` inside ``viterbi_librosa_fn``.  These functions do both steps in
one kernel launch (``vit_obs_build``) and return the ``[..., T, n_bins+1]`` float32 (or float16)
log-emission tensor that ``decode()`` consumes, so logits produced by an acoustic model on the GPU never
visit the host (the ``.cpu().numpy()`` round trip at tonet/for_paper.py:2282).
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from . import _lib


_DTYPES = {torch.float32: _lib.VIT_F32, torch.float16: _lib.VIT_F16}


def _check(logits: torch.Tensor, last: int) -> torch.Tensor:
    if not isinstance(logits, torch.Tensor) or logits.device.type != "cuda":
        raise ValueError("logits must be a torch tensor on a ROCm GPU (there is no CPU path)")
    if logits.dtype not in _DTYPES or logits.dim() < 2 or logits.shape[-1] != last:
        raise ValueError(f"logits must be float32 or float16 [..., frames, {last}]")
    if not logits.is_contiguous():
        raise ValueError("logits must be C-contiguous")
    return logits


def _out(out, shape, device, dtype=torch.float32) -> torch.Tensor:
    if dtype not in _DTYPES:
        raise ValueError("dtype must be torch.float32 or torch.float16")
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or out.device != device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {dtype} {tuple(shape)} tensor on the logits' device")
    return out


def _build(mode: int, logits: torch.Tensor, n_bins: int, spw: int, threshold_logit: float, offset: float, scale: float,
           prior: torch.Tensor | None, out: torch.Tensor) -> torch.Tensor:
    """One ``vit_obs_build`` launch: ``logits`` and ``out`` in their own dtypes (float32 or float16 each)."""
    obs = _lib.ObsParams(mode, n_bins, spw, threshold_logit, offset, scale, prior.data_ptr() if prior is not None else None)
    n = out.numel() // (n_bins + 1)
    with torch.cuda.device(logits.device):
        rc = _lib.load().vit_obs_build(obs, logits.data_ptr(), _DTYPES[logits.dtype], n, out.data_ptr(), _DTYPES[out.dtype],
                                       torch.cuda.current_stream(logits.device).cuda_stream)
    _lib.check(rc, "vit_obs_build")
    return out


# Storage types of the three builders below.  ``logits`` may be float32 or float16 (a model under autocast): a float16 logit is
# widened exactly, so the result is that of the float32 call on ``logits.float()``, bit for bit.  ``dtype`` is the emission dtype:
# with ``torch.float16`` every float32 result is rounded to nearest even as it is stored (the call on float32 followed by
# ``.half()``, bit for bit, without the float32 tensor ever existing) -- half the bytes for the decoder to read.  Float16 emissions
# are a DIFFERENT decoder input: a decode of them is the reference decoder's result on the rounded rows, not on the float32 rows
# (on the synthetic logits of scripts/obs_half_time.py 3.75e-5 of the frames at [1024 x 30000, 360] and 1.9e-5 at [256 x 30000, 722] decode
# to another state than with float32 rows: profiles/obs_half_time.json).


def shaun_log_emissions(logits: torch.Tensor, voicing_threshold: float = 0.32, single_side_peak_width: int = 5,
                        p: float = 0.8, scale: float = 2.0, out: torch.Tensor | None = None,
                        dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``Viterbi.observation_probs_fn`` + log: logits ``[..., T, n_bins]`` (float32 or float16) -> log-emissions
    ``[..., T, n_bins+1]`` in ``dtype`` (float32 or float16; into ``out`` when given: a caller's emission buffer of that dtype).
    Float16 emissions are the float32 ones rounded to nearest even -- a different decoder input, see above."""
    n_bins = logits.shape[-1]
    logits = _check(logits, n_bins)
    assert 0 < voicing_threshold < 1
    out = _out(out, logits.shape[:-1] + (n_bins + 1,), logits.device, dtype)
    return _build(0, logits, n_bins, single_side_peak_width, math.log(voicing_threshold / (1.0 - voicing_threshold)),
                  math.log(p / (1.0 - p)), scale, None, out)


def softmax_log_emissions(logits: torch.Tensor, single_side_peak_width: int = 15, out: torch.Tensor | None = None,
                          dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``SoftMaxViterbi.observation_probs_fn`` + log: logits ``[..., T, n_bins+1]`` (column 0 = unvoiced; float32 or float16) ->
    log-emissions ``[..., T, n_bins+1]`` in ``dtype`` (float32 or float16) with the unvoiced state last.  Float16 emissions are
    the float32 ones rounded to nearest even -- a different decoder input, see above."""
    S = logits.shape[-1]
    logits = _check(logits, S)
    out = _out(out, logits.shape, logits.device, dtype)
    return _build(1, logits, S - 1, single_side_peak_width, 0.0, 0.0, 0.0, None, out)


def softmax_scaled_log_emissions(logits: torch.Tensor, voicing_threshold_prob: float, prior: torch.Tensor | None,
                                 single_side_peak_width: int = 5, out: torch.Tensor | None = None,
                                 dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """dcnet's ``SoftMaxViterbi.observation_probs_fn`` (dcnet/softmax_viterbi.py:2530-2579) + log: logits ``[..., T, n_bins]``
    (float32 or float16) -> log of the scaled likelihoods ``[..., T, n_bins+1]`` in ``dtype`` (float32 or float16; unvoiced last;
    values above 0 are normal).  ``prior``: the state prior ``[n_bins+1]`` (float32, unvoiced last) on the GPU, or None for the
    unscaled variant.  ``out``: a caller's emission buffer of ``dtype``.  Float16 emissions are the float32 ones rounded to nearest
    even -- a different decoder input, see above."""
    n_bins = logits.shape[-1]
    logits = _check(logits, n_bins)
    assert 0 < voicing_threshold_prob < 1
    if prior is not None:
        if prior.device != logits.device or prior.dtype != torch.float32 or tuple(prior.shape) != (n_bins + 1,) or not prior.is_contiguous():
            raise ValueError(f"prior must be a contiguous float32 [{n_bins + 1}] tensor on the logits' device")
    out = _out(out, logits.shape[:-1] + (n_bins + 1,), logits.device, dtype)
    # the reference pads with log(vth / (1. - vth)) computed from an np.float32 scalar (dcnet/softmax_viterbi.py:2546-2548): float32
    # arithmetic under NumPy >= 2 -- the NumPy that generated tests/golden/obs_goldens.npz -- (NumPy 1.x promoted the scalar
    # expression to float64 before the float32 pad: at most one ulp apart); hand the kernel exactly the float32 value
    vth = np.float32(voicing_threshold_prob)
    unvoiced_logit = float(np.log(vth / (np.float32(1) - vth)))
    return _build(2, logits, n_bins, single_side_peak_width, unvoiced_logit, 0.0, 0.0, prior, out)


@functools.lru_cache(maxsize=None)
def activation_clamp_constants():
    """``(clamp_below, clamp_to)`` of ``vit_obs_activations`` as float32 scalars: the reference replaces the smallest positive
    activation ``t`` by ``exp(-87)`` when ``np.log(t) < -87`` (imm/tf_imm.py:81-82).  ``clamp_below`` is the smallest float32 whose
    NumPy float32 log is NOT below -87, found by bisection over the bit patterns of the positive floats, so that the kernel
    decides the clamp with an integer compare and agrees with the host for every input."""
    def below(bits):
        return bool(np.log(np.uint32(bits).view(np.float32)) < -87)
    lo, hi = 1, 0x3F800000                 # the smallest subnormal (log = -103.3) .. 1.0
    assert below(lo) and not below(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if below(mid):
            lo = mid
        else:
            hi = mid
    return np.uint32(hi).view(np.float32), np.float32(np.exp(-87))


def activation_log_emissions(hf0: torch.Tensor, offsets=None, out: torch.Tensor | None = None, dtype: torch.dtype = torch.float32,
                             return_stats: bool = False):
    """imm's ``Viterbi.process_HF0_fn`` (imm/tf_imm.py:70-88) on the GPU: source activations ``hf0 [U, N]`` (bins x frames,
    float32, unit stride along frames; a column slice of a wider buffer is fine) -> log-emissions ``[N, U + 1]`` in ``dtype``
    (float32 or float16), the layout ``decode`` / ``decode_packed`` read: ``log(hf0 + t)`` transposed, the unvoiced column
    filled with the minimum of the others (``vit_obs_activations``).  ``offsets``: B + 1 frame offsets from 0 to N when ``hf0``
    holds B recordings side by side (host sequence or int64 tensor; None: one recording) -- ``t`` and the minimum are per
    recording, as the reference computes them.  ``return_stats=True``: also the float32 ``[B, 4]`` tensor
    ``{min positive, min, t, _min}`` per recording.  Entries must be finite and >= 0 with a positive one in every recording."""
    if not isinstance(hf0, torch.Tensor) or hf0.device.type != "cuda":
        raise ValueError("hf0 must be a torch tensor on a ROCm GPU (there is no CPU path)")
    if hf0.dtype != torch.float32 or hf0.dim() != 2 or hf0.shape[0] < 1 or hf0.shape[0] > 1023 or hf0.shape[1] < 1:
        raise ValueError("hf0 must be float32 [U, N] with 1 <= U <= 1023 and N >= 1")
    U, N = int(hf0.shape[0]), int(hf0.shape[1])
    if hf0.stride(1) != 1 or (U > 1 and hf0.stride(0) < N):
        raise ValueError("hf0 must have unit stride along frames and a row stride >= N")
    ld = int(hf0.stride(0)) if U > 1 else N
    if dtype not in (torch.float32, torch.float16):
        raise ValueError("dtype must be torch.float32 or torch.float16")
    if offsets is None:
        offsets = [0, N]
    if isinstance(offsets, torch.Tensor) and offsets.device == hf0.device:
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 2 or not offsets.is_contiguous():
            raise ValueError("offsets must be a contiguous int64 [B + 1] tensor")
        off_dev = offsets                                       # (device-resident: taken as it is, no host visit)
    else:
        off = np.ascontiguousarray(offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64)
        if off.ndim != 1 or off.size < 2 or off[0] != 0 or (np.diff(off) < 1).any() or off[-1] != N:
            raise ValueError("offsets must be B + 1 strictly increasing frame offsets from 0 to the number of frames")
        off_dev = torch.from_numpy(off).to(hf0.device)
    B = int(off_dev.numel()) - 1
    shape = (N, U + 1)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=hf0.device)
    elif out.dtype != dtype or tuple(out.shape) != shape or out.device != hf0.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {dtype} {shape} tensor on hf0's device")
    stats = torch.empty((B, 4), dtype=torch.float32, device=hf0.device)
    clamp_below, clamp_to = activation_clamp_constants()
    with torch.cuda.device(hf0.device):
        rc = _lib.load().vit_obs_activations(hf0.data_ptr(), ld, U, B, off_dev.data_ptr(), N, float(clamp_below), float(clamp_to),
                                             stats.data_ptr(), out.data_ptr(), _lib.VIT_F16 if dtype == torch.float16 else _lib.VIT_F32,
                                             torch.cuda.current_stream(hf0.device).cuda_stream)
    _lib.check(rc, "vit_obs_activations")
    return (out, stats) if return_stats else out
