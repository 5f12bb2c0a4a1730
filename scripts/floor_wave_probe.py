"""Per-wave probe of the floor forward kernels (hooks build only: make -C viterbi_spl_amd/csrc TIMING=1).
For each forward_form given: forward time without a probe, cycles per frame (timing option 16) and, per wave, the SIMD it
ran on, the mean cycles from the barrier release to the return of the frame's first s_waitcnt (the split kernel) and to "last
max3 done", and the mean cycles from its s_waitcnt lgkmcnt(0) to the next barrier release (timing option 64), mean over the songs
of a [B, 30000, 361] batch.
usage: floor_wave_probe.py [B] [forward_form ...]   (default 128, forms 1)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from viterbi_spl_amd import _lib  # noqa: E402

_lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libviterbi_hip_timing.so")
from viterbi_spl_amd import ViterbiDecoder, synth  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
forms = [int(x) for x in sys.argv[2:]] or [1]
T, S = 30000, 361
dev = torch.device("cuda:0")
A, pi = synth.log_params(synth.tonet_transition(S - 1, 14), synth.floored_prior(S))
dec = ViterbiDecoder(A, pi, dev)
base = synth.emissions_peaks(min(B, 32), T, S, seed=1234, device=dev)
E = base if B <= 32 else base.repeat((B + 31) // 32, 1, 1)[:B].contiguous()
st = torch.empty((B, T), dtype=torch.int32, device=dev)
ll = torch.empty((B,), dtype=torch.float32, device=dev)


def forward(n):
    dec.decode_into(E, st, ll, algo="group", phase="forward")
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(n):
        dec.decode_into(E, st, ll, algo="group", phase="forward")
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / n


def scratch():
    ws = dec._ws
    pad = (-ws.data_ptr()) % 256
    off = pad + (B * T * ((S + 5) // 4 * 4) * 4 + 255) // 256 * 256     # the history, then [B][64] floats of scratch
    return ws[off:off + B * 64 * 4].view(torch.float32).view(B, 64).cpu().numpy()


for form in forms:
    dec.set_option("reset", 0)
    dec.set_option("forward_form", form)
    print(f"forward_form {form}, B {B}: forward {forward(5):.3f} ms without a probe", flush=True)
    dec.set_option("timing", 16)
    ms = forward(3)
    c = scratch()[:, 63]
    print(f"  cycle probe: forward {ms:.3f} ms; cycles per frame median {np.median(c):.1f} min {c.min():.1f} max {c.max():.1f}")
    dec.set_option("timing", 64)
    ms = forward(3)
    sc = scratch()
    print(f"  per-wave probe: forward {ms:.3f} ms (two s_memtime round trips a frame more)")
    for w in range(16):
        q = sc[:, 4 * w:4 * w + 4]
        if w * 4 + 3 >= 63 or not (q[:, 3] == T - 1).all():
            break
        simd = q[:, 0].astype(np.int64)
        d = sc[:, 48 + w]      # barrier release -> behind the frame's first s_waitcnt (the split kernel only; 0 elsewhere)
        print(f"  wave {w}: SIMD {np.bincount(simd, minlength=4).tolist()} (songs by SIMD_ID)  barrier -> first data {d.mean():6.1f}"
              f" (min {d.min():.1f} max {d.max():.1f})  barrier -> last max3 {q[:,1].mean():6.1f}"
              f" (min {q[:,1].min():.1f} max {q[:,1].max():.1f})  lgkmcnt(0) -> barrier release {q[:,2].mean():6.1f} cycles")
