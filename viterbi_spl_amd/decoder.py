"""Host side of the MI355X Viterbi decoder: torch tensors in, ctypes C ABI underneath.

``decode(emission_logits, transition_matrix, init_probs)`` is the call surface named by
BASELINE.json; it follows the reference's log-domain core
``viterbi_librosa_fn(*, log_transition_matrix_T, log_prob_init, log_probs_st)``
(imm/tf_viterbi.py:75-109 in the reference repo) with these conventions:

* ``transition_matrix`` -- LOG-domain, transposed: ``[S, S]`` float32 with row ``j`` = log-probabilities
  INTO target ``j`` (what the reference calls ``log_transition_matrix_T`` / ``B``,
  tonet/for_paper.py:1798-1815);
* ``init_probs``        -- LOG-domain ``[S]`` float32 (``log_prob_init``);
* ``emission_logits``   -- LOG-domain ``[T, S]`` or ``[B, T, S]`` float32/float16, C-contiguous, on the GPU
  (time-major rows, the layout the reference hands its core: dcnet/tf_viterbi_decoding.py:145).

PyTorch is plumbing only here (device memory, streams); all arithmetic happens in
libviterbi_hip.so.  Nothing in this module falls back to the CPU.
"""
from __future__ import annotations

import contextlib
import ctypes
import hashlib
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .stream import DecodeStream  # noqa: F401  (the sessions' module; this one stays the surface callers import)


_NO_F64 = ("banded, its floor form proven, without dense rows (unstructured matrices, the Durrieu step matrices and scan-only plans "
           "are not served)")
_NO_LOGITS = ("the fused logits decode needs a plan with the wave form whose extra column is the last state (S = 321 / 361), "
              "n_bins = S - 1, and a builder geometry of the reference (shaun / scaled softmax with peak width 5, softmax with 15): "
              "build the emissions and use decode()")
# The entry table: `entry` names the pair ``vit_workspace_bytes_<entry>`` / ``vit_decode_<entry>`` (sessions: ``vit_stream_open*``,
# ``vit_stream_commit_begin``) -> what a caller is told when the size query answers 0: the plan, or the segment length, is not served.
_NOT_SERVED = {
    "checkpointed": "the checkpointed decode needs 64 <= segment_frames <= 2**24 and a plan with the wave form, the floor form (banded, "
                    "no dense rows) or the step form (unstructured matrices and scan-only banded plans: decode() with the full history)",
    "f64": "the float64 decode needs a banded plan whose floor form is proven, without dense rows (unstructured matrices, the Durrieu "
           "step matrices and scan-only plans are not served)",
    "f64_checkpointed": "the checkpointed float64 decode needs 64 <= segment_frames <= 2**24 and a plan decode_f64 serves: " + _NO_F64,
    "f64_packed": "the packed float64 decode needs a banded plan whose floor form is proven, without dense rows (unstructured matrices, "
                  "the Durrieu step matrices and scan-only plans are not served)",
    "f64_packed_checkpointed": "the packed checkpointed float64 decode needs 64 <= segment_frames <= 2**24 and a plan decode_f64 "
                               "serves: " + _NO_F64,
    "packed": "the packed decode needs a plan with the wave form, the floor form or the step form (unstructured matrices and scan-only "
              "banded plans: pad and use decode(lengths=))",
    "packed_checkpointed": "the packed checkpointed decode needs 64 <= segment_frames <= 2**24 and a plan with the wave form (S = 321 / "
                           "361; the 722-state grids: pad and use decode_checkpointed(lengths=), or split the recordings into groups "
                           "whose workspace_bytes_packed fits)",
    "packed_bounded": "the bounded packed decode needs 64 <= segment_frames <= 2**24 and a plan with the wave form, the floor form with "
                      "the sparse back-trace, or the step form (unstructured matrices and scan-only banded plans: pad and use "
                      "decode(lengths=))",
    "logits": _NO_LOGITS,
    "logits_checkpointed": "the checkpointed fused logits decode needs 64 <= segment_frames <= 2**24; " + _NO_LOGITS,
    "stream": "no streaming decode for this plan: it needs a banded plan whose floor form is proven (no dense rows) or a "
              "step-structured plan of the Durrieu geometry",
    "stream_ring": "no ring session for this plan or size: it needs a banded session plan (one with a commit point) and 64 <= "
                   "ring_frames <= 2**30",
    "stream_commit": "no commit point for this plan: it needs a banded session plan (step-structured plans decide back-pointers by whole "
                     "rows)",
}


def _as_host_f32(x, shape=None) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    a = np.ascontiguousarray(x, dtype=np.float32)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """The address of an optional tensor argument (None stays None: the library's NULL)."""
    return t.data_ptr() if t is not None else None


class ViterbiDecoder:
    """A transition matrix + prior analysed once and resident on one GPU.

    Mirrors the reference's ``Viterbi.__init__`` (tonet/for_paper.py:1685-1701): parameters are
    prepared once, then many songs are decoded.
    """

    def __init__(self, log_transition_matrix_T, log_prob_init, device: Optional[torch.device] = None):
        lib = _lib.load()
        A = _as_host_f32(log_transition_matrix_T)
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise ValueError("log_transition_matrix_T must be [S, S]")
        S = A.shape[0]
        pi = _as_host_f32(log_prob_init, (S,))
        if np.isnan(A).any() or np.isnan(pi).any():
            raise ValueError("NaN in HMM parameters")
        self.S = S
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise ValueError("ViterbiDecoder needs a GPU device (there is no CPU path)")
        self._plan = ctypes.c_void_p()
        _lib.check(lib.vit_plan_create(A.ctypes.data, pi.ctypes.data, S, ctypes.byref(self._plan)), "vit_plan_create")
        info = _lib.PlanInfo()
        _lib.check(lib.vit_plan_query(self._plan, ctypes.byref(info)), "vit_plan_query")
        self.info = {
            "S": int(info.S), "banded_ok": bool(info.banded_ok), "n_extras": int(info.n_extras),
            "n_dense_rows": int(info.reserved[0]), "floor_ok": bool(info.reserved[1]), "lo_affine": bool(info.reserved[2] & 1), "pair_ok": bool(info.reserved[2] & 2), "step_ok": bool(info.reserved[2] & 4), "wave_ok": bool(info.reserved[2] & 8), "max_window": int(info.max_window),
            "group_window": int(info.group_window), "row_constant": float(info.consts[0]),
            "extras": [int(info.extras[k]) for k in range(int(info.n_extras))],
        }
        nbytes = int(lib.vit_plan_image_bytes(self._plan))
        with torch.cuda.device(self.device):
            self._image = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
            self._image_ptr = (self._image.data_ptr() + 255) & ~255
            stream = torch.cuda.current_stream(self.device)
            _lib.check(lib.vit_plan_upload(self._plan, self._image_ptr, nbytes, stream.cuda_stream), "vit_plan_upload")
            stream.synchronize()  # host image is pageable: make the copy visible before anything else
        self._ws: Optional[torch.Tensor] = None
        self._ws_slots: dict = {}
        self._options: dict = {}

    def __del__(self):
        try:
            if getattr(self, "_plan", None) is not None and self._plan.value:
                _lib.load().vit_plan_destroy(self._plan)
                self._plan = ctypes.c_void_p()
        except Exception:
            pass

    def set_option(self, key: str, value: int) -> None:
        """Kernel-selection override (``vit_plan_set_option``; keys in include/viterbi_hip.h).  Every setting decodes the
        same bits; ``set_option("reset", 0)`` restores the defaults."""
        _lib.check(_lib.load().vit_plan_set_option(self._plan, key.encode(), int(value)), f"vit_plan_set_option({key})")
        if key == "reset":
            self._options = {}
        else:
            self._options[key] = int(value)

    @contextlib.contextmanager
    def _option(self, key: str, value: int):
        """Hold option `key` at `value` inside a ``with`` block, then put back what was set before (0: the library's default)."""
        prev = self._options.get(key, 0)
        self.set_option(key, value)
        try:
            yield
        finally:
            self.set_option(key, prev)

    def chunks_beside_forward(self, B: int) -> int:
        """``bt_chunks`` for the two-stream schedule (the back-trace of batch i beside the forward pass of batch i + 1): while one
        song per workgroup leaves compute units idle (B below the CU count), the back-trace gets the chunks that fill THOSE units
        -- sixteen waves each -- instead of every unit of the chip, where its workgroups sit next to the latency-bound forward
        workgroups and slow them down (B = 128: 10.04 instead of 10.22 ms per step, scripts/overlap_ab.py).  0 = the library's own
        count (what a single stream should use: the back-trace alone is fastest with every unit)."""
        n_cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        if B <= 0 or 2 * (n_cus - B) < B:                  # fewer idle units than half the songs: the idle units alone would serialise the
            return 0                                        # back-trace (B = 250 on 256 units: ONE chunk per song) -- the library's own count
        return max(4, min(32, 16 * (n_cus - B) // B))      # (32: the library's cap, kBtMaxChunks)

    FAMILIES = {1: "dense", 2: "group", 3: "wave"}

    def forward_family(self, B: int, algo: str = "auto") -> str:
        """The forward kernel family the library launches for this batch size (``vit_forward_family``): "dense" (any matrix, or
        the step-structured kernel), "group" (banded, one song per workgroup) or "wave" (banded, one song per wavefront).  The
        thresholds scale with the device's compute units -- ask, do not guess."""
        fam = int(_lib.load().vit_forward_family(self._plan, int(B), _lib.ALGO[algo]))
        if fam < 0:
            _lib.check(fam, "vit_forward_family")
        return self.FAMILIES[fam]

    # ------------------------------------------------------------------ workspace
    def workspace_bytes(self, B: int, T: int, algo: Optional[str] = None) -> int:
        """Bytes of workspace a [B,T,S] decode needs: for one `algo` (``vit_workspace_bytes_for`` -- the wave form keeps
        half a history), or enough for any of them (``vit_workspace_bytes``) when `algo` is None."""
        lib = _lib.load()
        if algo is None:
            return int(lib.vit_workspace_bytes(self._plan, B, T))
        need = int(lib.vit_workspace_bytes_for(self._plan, B, T, _lib.ALGO[algo]))
        if need == 0 and B > 0:
            raise _lib.ViterbiHipError(f"algo {algo!r} is not available for this plan")
        return need

    def history_mode(self, B: int, T: int, algo: str = "auto") -> str:
        """"half" if the forward kernel `algo` resolves to for this batch stores only the delta rows of even frames (the wave form;
        the back-trace rebuilds the odd ones), else "full" -- read off the workspace the library asks for."""
        need = self.workspace_bytes(B, T, algo)
        return "half" if need * 1.5 < self.workspace_bytes(B, T) else "full"

    def _workspace(self, B: int, T: int, slot: int = 0, algo: Optional[str] = None) -> Tuple[int, int]:
        """Workspace `slot` (callers that overlap the back-trace of one batch with the forward pass of the next on
        two streams give each batch in flight its own slot; slot 0 is the default).  A buffer that is already large
        enough is kept, so alternating algos on one decoder settle on the largest need."""
        need = self.workspace_bytes(B, T, algo)
        ws = self._ws if slot == 0 else self._ws_slots.get(slot)
        if ws is None or ws.numel() < need + 256:
            ws = None
            if slot == 0:
                self._ws = None
            else:
                self._ws_slots.pop(slot, None)
            ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
            if slot == 0:
                self._ws = ws
            else:
                self._ws_slots[slot] = ws
        return (ws.data_ptr() + 255) & ~255, ws.numel() - 256

    def _call_workspace(self, need: int, workspace: Optional[torch.Tensor]) -> Tuple[torch.Tensor, int, int, bool]:
        """The workspace of ONE call of a bounded, packed or fused decode: the caller's tensor, or ``need + 256`` bytes allocated here
        -> (tensor, its first 256-byte aligned address, the bytes usable from there, allocated here).  A buffer allocated here must
        outlive the kernels: the decode synchronises the stream before it returns."""
        ws = workspace if workspace is not None else torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        if ws.dtype != torch.uint8 or ws.device != self.device or ws.numel() < need + 256:
            raise ValueError(f"workspace must be a uint8 tensor of at least {need + 256} bytes on the decoder's device")
        return ws, (ws.data_ptr() + 255) & ~255, ws.numel() - 256, workspace is None

    # ------------------------------------------------------------------ the one call path of the decodes that take a workspace
    def _need(self, entry: str, required: bool, *args) -> int:
        """``vit_workspace_bytes_<entry>(plan, *args)``.  0 means the plan (or the segment length) is not served: ViterbiHipError
        with the entry's text of ``_NOT_SERVED`` when `required`, else the 0."""
        need = int(getattr(_lib.load(), "vit_workspace_bytes_" + entry)(self._plan, *args))
        if need == 0 and required:
            raise _lib.ViterbiHipError(_NOT_SERVED[entry])
        return need

    def _enqueue(self, entry: str, *args) -> None:
        """``vit_decode_<entry>(plan, *args, stream)`` on the current stream of the decoder's device."""
        with torch.cuda.device(self.device):
            rc = getattr(_lib.load(), "vit_decode_" + entry)(self._plan, *args, torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(rc, "vit_decode_" + entry)

    def _finish(self, states: torch.Tensor, loglik: torch.Tensor, out_dtype: torch.dtype, allocated: bool, single: bool = False
                ) -> Tuple[torch.Tensor, torch.Tensor]:
        """The end of every such decode: a workspace `allocated` by the call must outlive its kernels, so the stream is synchronised
        then and only then; the states as ``out_dtype``; a `single` [T, S] input gets its [T] path and scalar back."""
        if allocated:
            torch.cuda.current_stream(self.device).synchronize()
        if out_dtype != torch.int32:
            states = states.to(out_dtype)
        return (states[0], loglik[0]) if single else (states, loglik)

    def _decode_entry(self, entry: str, B: int, shape: tuple, loglik_dtype: torch.dtype, out_dtype: torch.dtype,
                      workspace: Optional[torch.Tensor], size_args: tuple, head: tuple, mid: tuple = (), tail: tuple = (),
                      single: bool = False, own_buffer: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """One decode of B recordings through ``vit_decode_<entry>``, after the caller's argument checks: the outputs (int32 states of
        `shape`, loglik [B]), the size query (``vit_workspace_bytes_<entry>(plan, *size_args)``; not served raises), the workspace, the
        call -- the library takes ``head..., workspace, bytes, mid..., states, loglik, tail...`` -- and the finish.  The workspace is
        the caller's tensor, else one allocated for this call (followed by a stream synchronise); `own_buffer` (``decode_f64``): else
        the decoder's slot-0 buffer, shared with ``decode`` and grown like it, and no synchronisation.  B == 0 asks the library
        nothing."""
        states = torch.empty(shape, dtype=torch.int32, device=self.device)
        loglik = torch.empty((B,), dtype=loglik_dtype, device=self.device)
        ws, allocated = None, False                         # (ws: a buffer allocated here lives until the synchronise in _finish)
        if B > 0:
            need = self._need(entry, True, *size_args)
            if own_buffer and workspace is None:
                if self._ws is None or self._ws.numel() < need + 256:
                    self._ws = None
                    self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
                workspace = self._ws
            ws, ws_ptr, ws_bytes, allocated = self._call_workspace(need, workspace)
            self._enqueue(entry, *head, ws_ptr, ws_bytes, *mid, states.data_ptr(), loglik.data_ptr(), *tail)
        return self._finish(states, loglik, out_dtype, allocated, single)

    # ------------------------------------------------------------------ checks
    def _check_emissions(self, logE: torch.Tensor) -> Tuple[torch.Tensor, bool, int]:
        if not isinstance(logE, torch.Tensor):
            raise TypeError("emission_logits must be a torch tensor on the GPU")
        if logE.device != self.device:
            raise ValueError(f"emission_logits is on {logE.device}, decoder is on {self.device}")
        dt = self._emission_dtype(logE)
        single = logE.dim() == 2
        if single:
            logE = logE.unsqueeze(0)
        if logE.dim() != 3 or logE.shape[2] != self.S or logE.shape[1] < 1:
            raise ValueError(f"emission_logits must be [B,T,{self.S}] or [T,{self.S}] with T >= 1")
        if not logE.is_contiguous():
            raise ValueError("emission_logits must be C-contiguous (the reference requires it too)")
        return logE, single, dt

    @staticmethod
    def _emission_dtype(logE: torch.Tensor) -> int:
        """The library's storage type of an emission tensor (``VIT_F32`` / ``VIT_F16``)."""
        if logE.dtype == torch.float32:
            return _lib.VIT_F32
        if logE.dtype == torch.float16:
            return _lib.VIT_F16
        raise TypeError("emission_logits must be float32 or float16")

    def _check_lengths(self, lengths: Optional[torch.Tensor], B: int) -> None:
        if lengths is not None and (lengths.dtype != torch.int64 or tuple(lengths.shape) != (B,) or lengths.device != self.device):
            raise ValueError("lengths must be an int64 [B] tensor on the decoder's device")

    # ------------------------------------------------------------------ decode
    def decode_into(self, logE: torch.Tensor, states: torch.Tensor, loglik: Optional[torch.Tensor] = None,
                    lengths: Optional[torch.Tensor] = None, algo: str = "auto", phase: str = "both", slot: int = 0) -> None:
        """Enqueue a decode on the current stream.  states: int32 [B,T]; loglik: float32 [B].
        `phase` "forward" / "backtrace" run the two halves separately (same `slot` = same workspace).

        Lifetime rule of the split form: `logE` must be the SAME tensor, unchanged, in both phases -- with the wave form's half
        history (``set_option("wave_history", 2)``) the back-trace reads 32 emission values of every odd frame again.  The
        back-trace phase hands the pointer to the library (``vit_backtrace_checked``), which refuses a tensor other than the one
        its forward pass decoded ("invalid argument"); a caller that double-buffers its emissions must keep a batch's buffer
        untouched until that batch's back-trace has run.

        A slot must not grow while a batch that uses it is in flight: ``_workspace`` replaces a buffer that is too small, so
        allocate every slot at the size it will need (``_workspace(B, T, slot, None)`` serves any form) before anything is
        enqueued, as ``bench.py`` and tests/test_gpu_two_streams.py do."""
        lib = _lib.load()
        logE, _, dt = self._check_emissions(logE)
        B, T, _ = logE.shape
        if states.dtype != torch.int32 or tuple(states.shape) != (B, T) or not states.is_contiguous():
            raise ValueError("states must be a contiguous int32 [B,T] tensor")
        if loglik is not None and (loglik.dtype != torch.float32 or tuple(loglik.shape) != (B,)):
            raise ValueError("loglik must be float32 [B]")
        self._check_lengths(lengths, B)
        ws_ptr, ws_bytes = self._workspace(B, T, slot, algo)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            len_ptr = lengths.data_ptr() if lengths is not None else None
            ll_ptr = loglik.data_ptr() if loglik is not None else None
            a = _lib.ALGO[algo]
            if phase == "both":
                rc = lib.vit_decode(self._plan, logE.data_ptr(), dt, B, T, len_ptr, ws_ptr, ws_bytes,
                                    states.data_ptr(), ll_ptr, a, stream)
            elif phase == "forward":
                rc = lib.vit_forward(self._plan, logE.data_ptr(), dt, B, T, len_ptr, ws_ptr, ws_bytes, ll_ptr, a, stream)
            elif phase == "backtrace":
                rc = lib.vit_backtrace_checked(self._plan, logE.data_ptr(), dt, B, T, len_ptr, ws_ptr, ws_bytes, states.data_ptr(), a, stream)
            else:
                raise ValueError(phase)
        _lib.check(rc, f"vit_{phase if phase != 'both' else 'decode'}")

    COUNTERS = ("tiles_fetched", "span_misses", "whole_row_evaluations", "odd_rows_rebuilt", "chunks_repaired", "frames_repaired")

    def backtrace_counters(self, B: int, T: int, slot: int = 0) -> dict:
        """Event counts of the last back-trace that ran on workspace `slot` (``vit_backtrace_counters``), summed over the songs.
        Synchronises the device."""
        ws = self._ws if slot == 0 else self._ws_slots.get(slot)
        if ws is None:
            raise _lib.ViterbiHipError("no workspace in this slot")
        base = (ws.data_ptr() + 255) & ~255
        off, n = ctypes.c_size_t(), ctypes.c_int32()
        _lib.check(_lib.load().vit_backtrace_counters(self._plan, B, T, base, ctypes.byref(off), ctypes.byref(n)), "vit_backtrace_counters")
        torch.cuda.synchronize(self.device)
        start = base - ws.data_ptr() + off.value
        ct = ws[start:start + B * n.value * 4].view(torch.int32).view(B, n.value).sum(dim=0).cpu().tolist()
        return {k: int(ct[i]) for i, k in enumerate(self.COUNTERS)}

    def plan_workspace(self, B: int, T: int, algo: str = "auto", max_workspace_bytes: Optional[int] = None) -> dict:
        """How a [B, T, S] batch is decoded under a workspace budget (bytes; None = whatever `algo` asks for):

        * ``{"mode": "full"}``  -- the normal decode fits (one delta row per frame, or what the options already select);
        * ``{"mode": "half"}``  -- the wave form with the rows of even frames only (``wave_history`` 2: half the workspace, a
          slower back-trace), where the plan has it;
        * ``{"mode": "checkpointed", "segment_frames": K}`` -- ``vit_decode_checkpointed`` with the largest K that fits (about
          twice the forward work; wave-form plans, and the workgroup-form plans of the 722-state grids: banded with the floor
          form proven, or step-structured -- those have no half history and fall straight from "full" to here).

        Raises ViterbiHipError when nothing fits.  Every mode decodes the same bits."""
        need = self.workspace_bytes(B, T, algo)
        if max_workspace_bytes is None or need <= max_workspace_bytes:
            return {"mode": "full", "workspace_bytes": need}
        wave = self.info["wave_ok"] and algo in ("auto", "banded", "wave") and T >= 2
        # plans without the wave form: the workgroup kernels of the checkpointed decode stand in for the banded workgroup family
        # or (step plans) for what "auto" picks; an `algo` that means the dense kernel keeps raising
        group = not self.info["wave_ok"] and ((self.info["banded_ok"] and algo in ("auto", "banded", "group")) or
                                              (not self.info["banded_ok"] and self.info["step_ok"] and algo == "auto"))
        if wave:
            with self._option("wave_history", 2):
                half = int(_lib.load().vit_workspace_bytes_for(self._plan, B, T, _lib.ALGO["wave"]))
            if 0 < half <= max_workspace_bytes:
                return {"mode": "half", "workspace_bytes": half}
        def checkpointed(K):                                # (0: an `algo` the checkpointed decode does not stand in for)
            return self._need("checkpointed", False, B, T, K) if wave or group else 0
        return self._plan_segments(need, checkpointed, max_workspace_bytes,
                                   lambda _: f"no decode of a [{B}, {T}, {self.S}] batch fits a workspace of {max_workspace_bytes} bytes "
                                             f"(the normal decode needs {need})")

    def decode(self, emission_logits: torch.Tensor, lengths: Optional[torch.Tensor] = None, algo: str = "auto",
               out_dtype: torch.dtype = torch.int64, max_workspace_bytes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Returns (states [B,T] or [T] of ``out_dtype`` (reference: int64), loglik float32 [B] or scalar).

        ``max_workspace_bytes``: a budget for the delta history (the reference keeps its work buffers for ONE song,
        tonet/for_paper.py:1852-1853; a batch of 2048 full-length songs asks for 94 GB, 178 GB with 722 states).  The decode falls
        from the full history to the wave form's half history (where the plan has one) to the checkpointed decode
        (``plan_workspace``) instead of running out of memory; the result is the same in every mode."""
        logE, single, _ = self._check_emissions(emission_logits)
        B, T, _ = logE.shape
        if B > 0 and max_workspace_bytes is not None:
            mode = self.plan_workspace(B, T, algo, int(max_workspace_bytes))
            if mode["mode"] == "checkpointed":
                st, ll = self.decode_checkpointed(logE, segment_frames=mode["segment_frames"], lengths=lengths, out_dtype=out_dtype)
                return (st[0], ll[0]) if single else (st, ll)
            if mode["mode"] == "half":
                with self._option("wave_history", 2):
                    self._ws = None                          # (a larger buffer kept from an earlier decode would defeat the budget)
                    st, ll = self.decode(logE, lengths=lengths, algo="wave", out_dtype=out_dtype)
                return (st[0], ll[0]) if single else (st, ll)
        states = torch.empty((B, T), dtype=torch.int32, device=self.device)
        loglik = torch.empty((B,), dtype=torch.float32, device=self.device)
        if B > 0:
            self.decode_into(logE, states, loglik, lengths, algo)
        if out_dtype != torch.int32:
            states = states.to(out_dtype)
        return (states[0], loglik[0]) if single else (states, loglik)

    def _decode_padded(self, entry: str, emission_logits: torch.Tensor, lengths: Optional[torch.Tensor], out_dtype: torch.dtype,
                       loglik_dtype: torch.dtype, workspace: Optional[torch.Tensor], extra: tuple = (), own_buffer: bool = False
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
        """``decode_checkpointed`` / ``decode_f64_checkpointed`` / the unbudgeted ``decode_f64``: the checks of a padded batch, then
        ``_decode_entry``; `extra`: the arguments size query and decode take behind the shape (the segment length)."""
        logE, single, dt = self._check_emissions(emission_logits)
        B, T, _ = logE.shape
        self._check_lengths(lengths, B)
        return self._decode_entry(entry, B, (B, T), loglik_dtype, out_dtype, workspace, (B, T) + extra,
                                  (logE.data_ptr(), dt, B, T, _ptr(lengths)), tail=extra, single=single, own_buffer=own_buffer)

    # ------------------------------------------------------------------ float64-accumulating decode
    def workspace_bytes_f64(self, B: int, T: int) -> int:
        """Workspace bytes of ``decode_f64``; raises ViterbiHipError for a plan it does not serve."""
        return self._need("f64", B > 0, B, T)

    def workspace_bytes_f64_checkpointed(self, B: int, T: int, segment_frames: int) -> int:
        """Workspace bytes of ``decode_f64_checkpointed``; raises ViterbiHipError for a plan or a segment length it does not serve."""
        return self._need("f64_checkpointed", B > 0, int(B), int(T), int(segment_frames))

    @staticmethod
    def _plan_segments(full_need: int, size_of, budget: Optional[int], no_fit=None) -> dict:
        """The budget policy of the checkpointed decodes as a pure function: ``full_need`` bytes of the whole history, ``size_of(K)``
        the bytes at segment length K (0 = not served), ``budget`` bytes or None.  ``{"mode": "full", ...}`` when the whole history
        fits, else the largest K of 8192, 4096, ..., 64 that fits (the fewest launches); ViterbiHipError when none does, with the
        caller's text ``no_fit(least)`` (``least``: the smallest need any K had, 0 when none is served)."""
        if budget is None or full_need <= budget:
            return {"mode": "full", "workspace_bytes": int(full_need)}
        least, K = 0, 8192
        while K >= 64:
            ck = int(size_of(K))
            if 0 < ck <= budget:
                return {"mode": "checkpointed", "segment_frames": K, "workspace_bytes": ck}
            least = ck if least == 0 or 0 < ck < least else least
            K //= 2
        raise _lib.ViterbiHipError(no_fit(least) if no_fit else f"no decode fits a workspace of {budget} bytes (the whole history needs {full_need})")

    def plan_workspace_f64(self, B: int, T: int, max_workspace_bytes: Optional[int] = None) -> dict:
        """How ``decode_f64`` decodes a [B, T, S] batch under a workspace budget (bytes; None = whatever it takes):
        ``{"mode": "full", "workspace_bytes": n}`` -- ``vit_decode_f64`` fits -- or ``{"mode": "checkpointed", "segment_frames": K,
        "workspace_bytes": n}`` -- ``vit_decode_f64_checkpointed`` with the largest K of 8192, 4096, ..., 64 that fits.  Raises
        ViterbiHipError when nothing fits or the plan is not served.  Both modes decode the same bits."""
        need, budget = self.workspace_bytes_f64(B, T), None if max_workspace_bytes is None else int(max_workspace_bytes)
        return self._plan_segments(need, lambda K: self._need("f64_checkpointed", False, B, T, K), budget,
                                   lambda _: f"no float64 decode of a [{B}, {T}, {self.S}] batch fits a workspace of {budget} bytes "
                                             f"(the whole history needs {need})")

    def decode_f64_checkpointed(self, emission_logits: torch.Tensor, segment_frames: int = 1024, lengths: Optional[torch.Tensor] = None,
                                out_dtype: torch.dtype = torch.int64, workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``decode_f64`` with a bounded workspace (``vit_decode_f64_checkpointed``): about ``T / segment_frames + segment_frames``
        rows of doubles per song instead of ``T``.  Same states, same float64 log-likelihood, bit for bit; about twice the forward
        work.  Plans: those of ``decode_f64``; any other raises ``ViterbiHipError`` before anything is enqueued.  ``workspace``: an
        optional uint8 tensor of at least ``workspace_bytes_f64_checkpointed(...) + 256`` bytes to decode in (the caller then keeps it
        alive until the stream has run the decode: the call does not synchronise); without one the call allocates its own and
        synchronises the stream before it returns."""
        return self._decode_padded("f64_checkpointed", emission_logits, lengths, out_dtype, torch.float64, workspace, (int(segment_frames),))

    def decode_f64(self, emission_logits: torch.Tensor, lengths: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.int64,
                   workspace: Optional[torch.Tensor] = None, max_workspace_bytes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The reference's float64 Viterbi variant (dcnet/tf_viterbi_decoding.py:209-263) on float32 / float16 emissions
        (``vit_decode_f64``): the running score is kept in float64, bit for bit what that NumPy loop computes on float32 parameters.
        Returns (states [B,T] or [T] of ``out_dtype``, loglik float64 [B] or scalar).  On long inputs the path differs from
        ``decode``'s in a few frames out of thousands; this one scores better.  ``workspace``: a uint8 tensor of at least
        ``workspace_bytes_f64(B, T) + 256`` bytes on the decoder's device (the caller keeps it alive until the stream has run the
        decode), else the decoder's own buffer, the one ``decode`` uses (twice that decode's bytes: rows of doubles; it stays that
        large until the decoder goes).  The call does not synchronise.

        ``max_workspace_bytes``: a budget for the workspace (``plan_workspace_f64``).  Where the whole history does not fit, the call
        goes through ``decode_f64_checkpointed`` with the largest segment length that does -- the same bits -- and raises
        ``ViterbiHipError`` before anything is enqueued when none does.  Under a budget the decoder's own buffer is not used where
        it is larger than the budget: it is dropped and allocated anew at the size needed."""
        logE, single, _ = self._check_emissions(emission_logits)
        B, T, _ = logE.shape
        self._check_lengths(lengths, B)
        if B > 0 and max_workspace_bytes is not None:
            mode = self.plan_workspace_f64(B, T, int(max_workspace_bytes))
            if mode["mode"] == "checkpointed":
                st, ll = self.decode_f64_checkpointed(logE, segment_frames=mode["segment_frames"], lengths=lengths, out_dtype=out_dtype,
                                                      workspace=workspace)
                return (st[0], ll[0]) if single else (st, ll)
            if workspace is None and self._ws is not None and self._ws.numel() > int(max_workspace_bytes) + 256:
                self._ws = None                              # (a larger buffer kept from an earlier decode would defeat the budget)
        return self._decode_padded("f64", emission_logits, lengths, out_dtype, torch.float64, workspace, own_buffer=True)

    # ------------------------------------------------------------------ the same over a packed (ragged) batch
    def workspace_bytes_f64_packed(self, B: int, total_frames: int) -> int:
        """Workspace bytes of ``decode_f64_packed`` for B recordings of ``total_frames`` frames together; raises ViterbiHipError for
        a plan it does not serve (the plans of ``decode_f64``)."""
        return self._need("f64_packed", True, int(B), int(total_frames))

    @staticmethod
    def _greedy_groups(offsets, size_of, budget: int) -> list:
        """Consecutive groups ``[(b0, b1), ...]`` of the recordings ``offsets`` describes: each takes recordings in order while
        ``size_of(recordings, frames)`` of the group fits ``budget``.  ValueError (naming the recording) when one alone does not."""
        off = [int(x) for x in offsets]
        groups, b0, B = [], 0, len(off) - 1
        while b0 < B:
            b1 = b0
            while b1 < B and size_of(b1 + 1 - b0, off[b1 + 1] - off[b0]) <= budget:
                b1 += 1
            if b1 == b0:
                raise ValueError(f"recording {b0} ({off[b0 + 1] - off[b0]} frames) alone needs {size_of(1, off[b0 + 1] - off[b0])} bytes")
            groups.append((b0, b1))
            b0 = b1
        return groups

    def plan_workspace_f64_packed(self, offsets, max_workspace_bytes: Optional[int] = None) -> dict:
        """How ``decode_f64_packed`` meets a workspace budget (bytes; None = whatever it takes): the checkpointed float64 decode
        the recordings are decoded in consecutive groups, each taking recordings in order while its
        ``workspace_bytes_f64_packed`` fits (``plan_workspace_f64_packed_bounded`` / ``decode_f64_packed_bounded`` meet a budget by
        segments instead: one decode over all recordings, and no recording is too long for it).  Returns ``{"groups": [(b0, b1), ...], "bytes": the largest group's need}``; raises
        ViterbiHipError when one recording alone does not fit, or for a plan that is not served."""
        off = self._host_offsets(offsets)
        B = off.size - 1
        if B == 0:
            return {"groups": [], "bytes": 0}
        if max_workspace_bytes is None:
            return {"groups": [(0, B)], "bytes": self.workspace_bytes_f64_packed(B, int(off[-1]))}
        try:
            groups = self._greedy_groups(off, self.workspace_bytes_f64_packed, int(max_workspace_bytes))
        except ValueError as e:
            raise _lib.ViterbiHipError(f"no packed float64 decode fits a workspace of {max_workspace_bytes} bytes: {e}") from None
        return {"groups": groups, "bytes": max(self.workspace_bytes_f64_packed(b1 - b0, int(off[b1] - off[b0])) for b0, b1 in groups)}

    def decode_f64_packed(self, emission_logits: torch.Tensor, offsets, out_dtype: torch.dtype = torch.int64,
                          workspace: Optional[torch.Tensor] = None, max_workspace_bytes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``decode_f64`` of B recordings of different lengths without padding (``vit_decode_f64_packed``): the arguments of
        ``decode_packed`` -- ``emission_logits [sum T_b, S]``, ``offsets`` a host sequence of B + 1 frame offsets from 0 -- and the
        recursion of ``decode_f64``.  Returns ``(states [sum T_b], loglik float64 [B])``, bit for bit ``decode_f64`` of each
        recording alone.  Plans: those of ``decode_f64``; any other raises ``ViterbiHipError`` before anything is enqueued.

        ``max_workspace_bytes``: a budget for the workspace, met by decoding consecutive groups of recordings one after the other
        in one workspace (``plan_workspace_f64_packed``) -- the same bytes out; ``ViterbiHipError`` before anything is enqueued when
        one recording alone does not fit.  ``workspace``: an optional uint8 tensor of at least the need + 256 bytes (the caller
        then keeps it alive until the stream has run the decode: the call does not synchronise)."""
        dt, off = self._check_packed(emission_logits, offsets)
        B, N = off.size - 1, int(off[-1])
        states = torch.empty((N,), dtype=torch.int32, device=self.device)
        loglik = torch.empty((B,), dtype=torch.float64, device=self.device)
        ws, allocated = None, False                         # (ws: one buffer for every group, alive until the synchronise in _finish)
        if B > 0:
            mode = self.plan_workspace_f64_packed(off, max_workspace_bytes)
            ws, ws_ptr, ws_bytes, allocated = self._call_workspace(mode["bytes"], workspace)
            for b0, b1 in mode["groups"]:                   # (a group: the same entry point on a row slice with rebased offsets)
                goff = np.ascontiguousarray(off[b0:b1 + 1] - off[b0])
                self._enqueue("f64_packed", emission_logits[int(off[b0]):].data_ptr(), dt, b1 - b0, goff.ctypes.data, ws_ptr, ws_bytes,
                              states[int(off[b0]):].data_ptr(), loglik[b0:].data_ptr())
        return self._finish(states, loglik, out_dtype, allocated)

    # ------------------------------------------------------------------ the packed float64 decode under a workspace budget
    def workspace_bytes_f64_packed_checkpointed(self, offsets, segment_frames: int) -> int:
        """Workspace bytes of ``decode_f64_packed_checkpointed`` for the recordings ``offsets`` describes (B + 1 host frame offsets);
        raises ViterbiHipError for a plan or a segment length it does not serve."""
        off = self._host_offsets(offsets)
        return self._need("f64_packed_checkpointed", True, off.size - 1, off.ctypes.data, int(segment_frames))

    def decode_f64_packed_checkpointed(self, emission_logits: torch.Tensor, offsets, segment_frames: int = 1024,
                                       out_dtype: torch.dtype = torch.int64, workspace: Optional[torch.Tensor] = None
                                       ) -> Tuple[torch.Tensor, torch.Tensor]:
        """``decode_f64_packed`` with a bounded workspace (``vit_decode_f64_packed_checkpointed``): ``n_units * (K + 1)`` rows of doubles
        for the (recording, segment) units being walked (``n_units = min(B, u x compute units)``, ``K = segment_frames``) plus one row
        per K frames of every recording, instead of one row per frame.  Same arguments, same states, same float64 log-likelihoods,
        bit for bit; about twice the forward work.  Plans: those of ``decode_f64``; any other raises ``ViterbiHipError`` before
        anything is enqueued.  ``workspace``: an optional uint8 tensor of at least ``workspace_bytes_f64_packed_checkpointed(...) +
        256`` bytes to decode in (the caller then keeps it alive until the stream has run the decode: the call does not synchronise);
        without one the call allocates its own and synchronises the stream before it returns."""
        return self._decode_packed_segments("f64_packed_checkpointed", emission_logits, offsets, segment_frames, out_dtype, workspace,
                                            torch.float64)

    def plan_workspace_f64_packed_bounded(self, offsets, max_workspace_bytes: Optional[int] = None) -> dict:
        """How ``decode_f64_packed_bounded`` decodes the recordings ``offsets`` describes under a workspace budget (bytes; None =
        whatever it takes): ``{"mode": "full", "workspace_bytes": n}`` -- ``vit_decode_f64_packed`` fits -- or ``{"mode":
        "checkpointed", "segment_frames": K, "workspace_bytes": n}`` -- ``vit_decode_f64_packed_checkpointed`` with the largest K of
        8192, 4096, ..., 64 that fits.  Raises ViterbiHipError when nothing fits or the plan is not served.  Both modes decode the
        same bits."""
        off = self._host_offsets(offsets)
        B, N = off.size - 1, int(off[-1])
        if B == 0:
            return {"mode": "full", "workspace_bytes": 0}
        need, budget = self.workspace_bytes_f64_packed(B, N), None if max_workspace_bytes is None else int(max_workspace_bytes)
        return self._plan_segments(need, lambda K: self._need("f64_packed_checkpointed", False, B, off.ctypes.data, K), budget,
                                   lambda least: f"no packed float64 decode of {B} recordings ({N} frames) fits a workspace of {budget} "
                                                 f"bytes (the whole history needs {need}, the checkpointed decode at least {least})")

    def decode_f64_packed_bounded(self, emission_logits: torch.Tensor, offsets, max_workspace_bytes: Optional[int] = None,
                                  out_dtype: torch.dtype = torch.int64, workspace: Optional[torch.Tensor] = None
                                  ) -> Tuple[torch.Tensor, torch.Tensor]:
        """``decode_f64_packed`` under a workspace budget met by segments, not by groups of recordings (``plan_workspace_f64_packed_bounded``):
        the whole history where it fits, else ``decode_f64_packed_checkpointed`` with the largest segment length that does -- one
        launch sequence over all recordings, and a recording longer than the budget's worth of rows is decoded all the same.  The
        same bits either way; ``ViterbiHipError`` before anything is enqueued when nothing fits.  Without ``workspace`` the call
        decodes in a tensor of its own of the planned bytes + 256, never more, and synchronises the stream before it returns."""
        _, off = self._check_packed(emission_logits, offsets)
        mode = self.plan_workspace_f64_packed_bounded(off, max_workspace_bytes)
        if mode["mode"] == "checkpointed":
            return self.decode_f64_packed_checkpointed(emission_logits, off, segment_frames=mode["segment_frames"], out_dtype=out_dtype,
                                                       workspace=workspace)
        return self.decode_f64_packed(emission_logits, off, out_dtype=out_dtype, workspace=workspace)

    # ------------------------------------------------------------------ bounded-workspace decode
    def workspace_bytes_checkpointed(self, B: int, T: int, segment_frames: int) -> int:
        """Workspace bytes of ``decode_checkpointed``; raises ViterbiHipError for a plan or a segment length it does not serve."""
        return self._need("checkpointed", B > 0, B, T, int(segment_frames))

    def workspace_bytes_checkpointed_or_zero(self, B: int, T: int, segment_frames: int) -> int:
        """The same without the exception: 0 when the checkpointed decode does not serve this plan or segment length."""
        return self._need("checkpointed", False, int(B), int(T), int(segment_frames))

    def decode_checkpointed(self, emission_logits: torch.Tensor, segment_frames: int = 1024, lengths: Optional[torch.Tensor] = None,
                            out_dtype: torch.dtype = torch.int64, workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``decode`` with a bounded workspace (``vit_decode_checkpointed``): about ``T / segment_frames + segment_frames`` delta
        rows per song instead of ``T`` -- the reference keeps its work buffers for one song at a time
        (tonet/for_paper.py:1852-1853).  Same states, same log-likelihood; about twice the forward work.  For plans with the wave
        form (S = 321 / 361), banded plans whose floor form is proven (the 722-state jdc grids) and step-structured plans (the
        Durrieu matrix); any other plan raises ``ViterbiHipError`` before anything is enqueued.  ``workspace``: an optional uint8
        tensor of at least ``workspace_bytes_checkpointed(...) + 256`` bytes to decode in (the caller then keeps it alive until the
        stream has run the decode: the call does not synchronise)."""
        return self._decode_padded("checkpointed", emission_logits, lengths, out_dtype, torch.float32, workspace, (int(segment_frames),))

    # ------------------------------------------------------------------ packed (ragged) decode
    def _check_packed(self, emission_logits: torch.Tensor, offsets) -> Tuple[int, np.ndarray]:
        """The argument checks of the packed decodes -> (emission storage type, host int64 offsets)."""
        if not isinstance(emission_logits, torch.Tensor) or emission_logits.device != self.device:
            raise ValueError("emission_logits must be a torch tensor on the decoder's device")
        if emission_logits.dim() != 2 or emission_logits.shape[1] != self.S or not emission_logits.is_contiguous():
            raise ValueError(f"emission_logits must be a C-contiguous [sum T_b, {self.S}] tensor")
        dt = self._emission_dtype(emission_logits)
        off = self._host_offsets(offsets)
        if off[-1] != emission_logits.shape[0]:
            raise ValueError("offsets must be B + 1 strictly increasing frame offsets from 0 to the number of emission rows")
        return dt, off

    @staticmethod
    def _host_offsets(offsets) -> np.ndarray:
        off = np.ascontiguousarray(offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64)
        if off.ndim != 1 or off.size < 1 or off[0] != 0 or (np.diff(off) < 1).any():
            raise ValueError("offsets must be B + 1 strictly increasing frame offsets from 0 to the number of emission rows")
        return off

    def decode_packed(self, emission_logits: torch.Tensor, offsets, out_dtype: torch.dtype = torch.int64,
                      workspace: Optional[torch.Tensor] = None, max_workspace_bytes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Decode B recordings of different lengths without padding (``vit_decode_packed``): ``emission_logits`` is
        ``[sum T_b, S]`` (the rows of recording b are ``offsets[b] : offsets[b+1]``), ``offsets`` a host sequence of B + 1
        frame offsets starting at 0.  Returns ``(states [sum T_b], loglik [B])``, packed like the input -- what the reference
        computes recording by recording (tonet/for_paper.py:2304-2309).  For plans with the wave form (S = 321 / 361), banded
        plans whose floor form is proven (the 722-state jdc grids, one workgroup per forward slot) and step-structured plans (the
        Durrieu matrix); any other plan (unstructured matrices, banded plans with only the scan form) raises ``ViterbiHipError``.

        ``max_workspace_bytes``: a budget for the workspace: where the full history does not fit, the decode falls to the
        checkpointed form with the largest segment length that does -- the same states and log-likelihoods -- and raises
        ``ViterbiHipError`` when nothing fits.  Plans with the wave form: ``plan_workspace_packed`` and
        ``decode_packed_checkpointed``; the other plans (the 722-state grids): ``plan_workspace_packed_bounded`` and
        ``decode_packed_bounded``.  ``None``: the full history, whatever it takes."""
        dt, off = self._check_packed(emission_logits, offsets)
        B, N = off.size - 1, int(off[-1])
        if B > 0 and max_workspace_bytes is not None:
            if self.info["wave_ok"]:
                mode = self.plan_workspace_packed(off, int(max_workspace_bytes))
                if mode["mode"] == "checkpointed":
                    return self.decode_packed_checkpointed(emission_logits, off, segment_frames=mode["segment_frames"], out_dtype=out_dtype,
                                                           workspace=workspace)
            else:
                mode = self.plan_workspace_packed_bounded(off, int(max_workspace_bytes))
                if mode["mode"] == "checkpointed":
                    return self.decode_packed_bounded(emission_logits, off, segment_frames=mode["segment_frames"], out_dtype=out_dtype,
                                                      workspace=workspace)
        return self._decode_entry("packed", B, (N,), torch.float32, out_dtype, workspace, (B, N),
                                  (emission_logits.data_ptr(), dt, B, off.ctypes.data))

    # ------------------------------------------------------------------ streaming
    def workspace_bytes_stream(self, B: int, max_frames: int) -> int:
        """Workspace bytes of a ``stream(B, max_frames)`` session (``vit_workspace_bytes_stream``); 0 when the plan has no stream
        form (see ``stream``)."""
        return self._need("stream", False, int(B), int(max_frames))

    def workspace_bytes_stream_ring(self, B: int, ring_frames: int) -> int:
        """Workspace bytes of a ``stream(B, ring_frames=R)`` session (``vit_workspace_bytes_stream_ring``); 0 when the plan has no
        commit point or R is outside [64, 2**30]."""
        return self._need("stream_ring", False, int(B), int(ring_frames))

    def stream(self, B: int, max_frames: Optional[int] = None, workspace: Optional[torch.Tensor] = None,
               ring_frames: Optional[int] = None) -> "DecodeStream":
        """A streaming session for B recordings of at most ``max_frames`` frames: ``append`` advances the forward pass chunk by
        chunk as emission rows arrive, ``decode`` back-traces the recordings as they stand -- the states and log-likelihoods of
        ``decode`` on the same frames, bit for bit, for any chunking.  For banded plans whose floor form is proven (the 321-, 361-
        and 722-state grids) and step-structured plans (the Durrieu matrix); any other plan raises ``ViterbiHipError``.
        ``workspace``: a uint8 tensor of at least ``workspace_bytes_stream(B, max_frames) + 256`` bytes, or None to allocate one.

        ``ring_frames=R`` (64 <= R <= 2**30) opens a RING session instead: R history rows per recording whatever its length
        (``max_frames`` is not needed), for the plans that have a commit point (the banded session plans).  Output then comes from
        ``commit()`` -- the frames that became final, which also lets the ring advance -- and ``tail()``, the frames behind the
        frontier; ``decode()`` and ``commit_into`` raise.  An ``append`` that would overwrite rows a commit may still need raises
        ``ViterbiHipError`` (commit first, or open with a larger R); where survivors do not merge inside R frames the session
        cannot advance.  ``workspace``: at least ``workspace_bytes_stream_ring(B, R) + 256`` bytes."""
        return DecodeStream(self, B, max_frames, workspace, ring_frames)

    def workspace_bytes_packed(self, B: int, total_frames: int) -> int:
        """Workspace bytes of ``decode_packed`` for B recordings of ``total_frames`` frames together; 0 when the plan has none of
        the forms the packed decode runs (see ``decode_packed``)."""
        return self._need("packed", False, int(B), int(total_frames))

    # ------------------------------------------------------------------ packed decode under a workspace budget
    def workspace_bytes_packed_checkpointed(self, offsets, segment_frames: int) -> int:
        """Workspace bytes of ``decode_packed_checkpointed`` for the recordings ``offsets`` describes (B + 1 host frame offsets); raises
        ViterbiHipError for a plan or a segment length it does not serve."""
        off = self._host_offsets(offsets)
        return self._need("packed_checkpointed", True, off.size - 1, off.ctypes.data, int(segment_frames))

    def decode_packed_checkpointed(self, emission_logits: torch.Tensor, offsets, segment_frames: int = 1024, out_dtype: torch.dtype = torch.int64,
                                   workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``decode_packed`` with a bounded workspace (``vit_decode_packed_checkpointed``): ``n_units * (K + 1)`` delta rows for the
        segments being walked (``n_units = min(B, 8 x compute units)``, ``K = segment_frames``) plus one row per K frames, instead of
        one row per frame.  Same arguments, same states, same log-likelihoods; about twice the forward work.  For plans with the
        wave form (S = 321 / 361); any other plan raises ``ViterbiHipError`` before anything is enqueued.  ``workspace``: an optional
        uint8 tensor of at least ``workspace_bytes_packed_checkpointed(...) + 256`` bytes to decode in (the caller then keeps it
        alive until the stream has run the decode: the call does not synchronise)."""
        return self._decode_packed_segments("packed_checkpointed", emission_logits, offsets, segment_frames, out_dtype, workspace)

    def _decode_packed_segments(self, entry: str, emission_logits: torch.Tensor, offsets, segment_frames: int, out_dtype: torch.dtype,
                                workspace: Optional[torch.Tensor], loglik_dtype: torch.dtype = torch.float32
                                ) -> Tuple[torch.Tensor, torch.Tensor]:
        """``decode_packed_checkpointed`` / ``decode_packed_bounded`` / ``decode_f64_packed_checkpointed``: the checks of a packed
        batch, then ``_decode_entry``."""
        dt, off = self._check_packed(emission_logits, offsets)
        B, K = off.size - 1, int(segment_frames)
        return self._decode_entry(entry, B, (int(off[-1]),), loglik_dtype, out_dtype, workspace, (B, off.ctypes.data, K),
                                  (emission_logits.data_ptr(), dt, B, off.ctypes.data), tail=(K,))

    def plan_workspace_packed(self, offsets, max_workspace_bytes: Optional[int] = None) -> dict:
        """How the recordings ``offsets`` describes are decoded under a workspace budget (bytes; None = whatever it takes):

        * ``{"mode": "full", "workspace_bytes": ...}`` -- ``decode_packed`` fits (one delta row per frame);
        * ``{"mode": "checkpointed", "segment_frames": K, "workspace_bytes": ...}`` -- ``decode_packed_checkpointed`` with the
          largest K of 8192, 4096, ..., 64 that fits (fewest launches; the rule of ``plan_workspace``).

        Raises ViterbiHipError naming the need when nothing fits or the plan is not served.  Both modes decode the same bits."""
        return self._plan_packed(offsets, max_workspace_bytes, "packed_checkpointed", "checkpointed",
                                 "no packed checkpointed decode (wave-form plans only: split the recordings into groups whose "
                                 "workspace_bytes_packed fits)")

    def _plan_packed(self, offsets, max_workspace_bytes: Optional[int], entry: str, kind: str, unserved: str) -> dict:
        """``plan_workspace_packed`` / ``plan_workspace_packed_bounded``: `entry` is the budgeted decode whose size query is asked,
        `kind` and `unserved` what the errors call it."""
        off = self._host_offsets(offsets)
        B, N = off.size - 1, int(off[-1])
        need = self._need("packed", B > 0, B, N)
        def no_fit(least):
            if least == 0:
                return (f"the packed decode of {B} recordings ({N} frames) needs a workspace of {need} bytes, the budget is "
                        f"{max_workspace_bytes}, and this plan has {unserved}")
            return (f"no packed decode of {B} recordings ({N} frames) fits a workspace of {max_workspace_bytes} bytes "
                    f"(the full history needs {need}, the {kind} decode at least {least})")
        return self._plan_segments(need, lambda K: self._need(entry, False, B, off.ctypes.data, K), max_workspace_bytes, no_fit)

    # ------------------------------------------------------------------ the same for every plan with a packed decode
    def workspace_bytes_packed_bounded(self, offsets, segment_frames: int) -> int:
        """Workspace bytes of ``decode_packed_bounded`` for the recordings ``offsets`` describes (B + 1 host frame offsets); raises
        ViterbiHipError for a plan or a segment length it does not serve."""
        off = self._host_offsets(offsets)
        return self._need("packed_bounded", True, off.size - 1, off.ctypes.data, int(segment_frames))

    def decode_packed_bounded(self, emission_logits: torch.Tensor, offsets, segment_frames: int = 1024, out_dtype: torch.dtype = torch.int64,
                              workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``decode_packed`` with a bounded workspace for every plan it serves (``vit_decode_packed_bounded``).  Plans with the wave form
        run ``decode_packed_checkpointed`` (the same size, the same bits).  The 722-state floor and step plans run its scheme with one
        workgroup per forward slot and per (recording, segment) unit: ``n_units * (K + 2)`` (step plans: ``K + 1``) delta rows for the
        segments being walked (``n_units = min(B, u x compute units)``, u = 1 / 2, ``K = segment_frames``) plus one row per K frames.
        Same arguments, same states, same log-likelihoods as ``decode_packed``; about twice the forward work.  Any other plan raises
        ``ViterbiHipError`` before anything is enqueued.  ``workspace``: an optional uint8 tensor of at least
        ``workspace_bytes_packed_bounded(...) + 256`` bytes to decode in (the caller then keeps it alive until the stream has run the
        decode: the call does not synchronise)."""
        return self._decode_packed_segments("packed_bounded", emission_logits, offsets, segment_frames, out_dtype, workspace)

    def plan_workspace_packed_bounded(self, offsets, max_workspace_bytes: Optional[int] = None) -> dict:
        """``plan_workspace_packed`` over ``decode_packed_bounded``: ``{"mode": "full", "workspace_bytes": ...}`` when ``decode_packed``
        fits the budget, else ``{"mode": "checkpointed", "segment_frames": K, "workspace_bytes": ...}`` with the largest K of 8192,
        4096, ..., 64 whose ``workspace_bytes_packed_bounded`` fits.  Raises ViterbiHipError naming the least need when nothing fits
        or the plan is not served."""
        return self._plan_packed(offsets, max_workspace_bytes, "packed_bounded", "bounded",
                                 "no bounded packed decode (pad and use decode_checkpointed(lengths=))")

    # ------------------------------------------------------------------ fused logits -> path decode
    @staticmethod
    def obs_params(mode: str, n_bins: int, single_side_peak_width: int, threshold_logit: float = 0.0, offset: float = 0.0,
                   scale: float = 0.0, prior: Optional[torch.Tensor] = None) -> dict:
        """The emission-builder arguments ``decode_logits`` takes (``vit_obs_params``): ``mode`` "shaun" (``vit_obs_shaun``:
        threshold logit, offset, scale), "softmax" (``vit_obs_softmax``: logits carry the unvoiced column first) or
        "softmax_scaled" (``vit_obs_softmax_scaled``: ``threshold_logit`` is the unvoiced logit, ``prior`` the state prior on the
        GPU or None)."""
        modes = {"shaun": 0, "softmax": 1, "softmax_scaled": 2}
        if mode not in modes:
            raise ValueError(f"mode must be one of {sorted(modes)}")
        return {"mode": modes[mode], "n_bins": int(n_bins), "spw": int(single_side_peak_width), "threshold_logit": float(threshold_logit),
                "offset": float(offset), "scale": float(scale), "prior": prior}

    def _obs_struct(self, obs: dict) -> "_lib.ObsParams":
        prior = obs.get("prior")
        if prior is not None:
            if (not isinstance(prior, torch.Tensor) or prior.device != self.device or prior.dtype != torch.float32 or
                    tuple(prior.shape) != (obs["n_bins"] + 1,) or not prior.is_contiguous()):
                raise ValueError(f"prior must be a contiguous float32 [{obs['n_bins'] + 1}] tensor on the decoder's device")
        return _lib.ObsParams(obs["mode"], obs["n_bins"], obs["spw"], obs["threshold_logit"], obs["offset"], obs["scale"],
                              prior.data_ptr() if prior is not None else None)

    def workspace_bytes_logits(self, obs: dict, B: int, T: int) -> int:
        """Workspace bytes of ``decode_logits`` (a full delta history in the wave layout, nothing for emissions); 0 when the
        fused kernel does not serve this plan or builder geometry (see ``decode_logits``)."""
        return self._need("logits", False, ctypes.byref(self._obs_struct(obs)), int(B), int(T))

    def workspace_bytes_logits_checkpointed(self, obs: dict, B: int, T: int, segment_frames: int) -> int:
        """Workspace bytes of ``decode_logits_checkpointed`` (what ``workspace_bytes_checkpointed`` answers for the same plan); 0 when
        the fused kernel does not serve this plan or builder geometry, or ``segment_frames`` is outside 64 .. 2**24."""
        return self._need("logits_checkpointed", False, ctypes.byref(self._obs_struct(obs)), int(B), int(T), int(segment_frames))

    def plan_workspace_logits(self, obs: dict, B: int, T: int, max_workspace_bytes: Optional[int] = None) -> dict:
        """How ``decode_logits`` decodes ``[B, T, cols]`` logits under a workspace budget (bytes; None = whatever it takes):
        ``{"mode": "full", "workspace_bytes": n}`` -- ``vit_decode_logits`` with the whole delta history fits -- or ``{"mode":
        "checkpointed", "segment_frames": K, "workspace_bytes": n}`` -- ``vit_decode_logits_checkpointed`` with the largest K of 8192,
        4096, ..., 64 that fits.  Raises ViterbiHipError when nothing fits (the text names the least need) or the plan or builder is
        not served.  Both modes decode the same bits."""
        need = self._need("logits", B > 0, ctypes.byref(self._obs_struct(obs)), B, T)
        budget = None if max_workspace_bytes is None else int(max_workspace_bytes)
        return self._plan_segments(need, lambda K: self.workspace_bytes_logits_checkpointed(obs, B, T, K), budget,
                                   lambda least: f"no fused logits decode of a [{B}, {T}] batch fits a workspace of {budget} bytes: the least "
                                                 f"any segment length needs is {least} (the whole history needs {need})")

    def _check_logits(self, logits: torch.Tensor, obs: dict, lengths: Optional[torch.Tensor]) -> Tuple[torch.Tensor, bool]:
        """The argument checks of the fused logits decodes -> (the logits as [B, T, cols], whether the caller's were [T, cols])."""
        if not isinstance(logits, torch.Tensor) or logits.device != self.device:
            raise ValueError("logits must be a torch tensor on the decoder's device")
        cols = obs["n_bins"] + (1 if obs["mode"] == 1 else 0)
        single = logits.dim() == 2
        lg = logits.unsqueeze(0) if single else logits
        if lg.dtype != torch.float32 or lg.dim() != 3 or lg.shape[2] != cols or lg.shape[1] < 1 or not lg.is_contiguous():
            raise ValueError(f"logits must be a C-contiguous float32 [B,T,{cols}] or [T,{cols}] tensor with T >= 1")
        self._check_lengths(lengths, lg.shape[0])
        return lg, single

    def decode_logits_checkpointed(self, logits: torch.Tensor, obs: dict, segment_frames: int = 1024, lengths: Optional[torch.Tensor] = None,
                                   out_dtype: torch.dtype = torch.int64, workspace: Optional[torch.Tensor] = None
                                   ) -> Tuple[torch.Tensor, torch.Tensor]:
        """``decode_logits`` with a bounded workspace (``vit_decode_logits_checkpointed``): about ``T / segment_frames +
        segment_frames`` delta rows per song instead of ``T``, and still no emission tensor -- a segment's emission rows are built
        again from the logits, inside the workgroup that consumes them.  Same states, same log-likelihood, bit for bit; about twice
        the forward work.  There is no ``emissions_out``: the call exists to save memory.  Plans and builders: those of
        ``decode_logits``; anything else raises ``ViterbiHipError`` before anything is enqueued.  ``workspace``: as for
        ``decode_checkpointed``."""
        lg, single = self._check_logits(logits, obs, lengths)
        B, T, _ = lg.shape
        K, op = int(segment_frames), ctypes.byref(self._obs_struct(obs))
        return self._decode_entry("logits_checkpointed", B, (B, T), torch.float32, out_dtype, workspace, (op, B, T, K),
                                  (lg.data_ptr(), op, B, T, _ptr(lengths)), tail=(K,), single=single)

    def decode_logits(self, logits: torch.Tensor, obs: dict, lengths: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.int64,
                      emissions_out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                      max_workspace_bytes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Pitch logits -> (states, loglik) in one forward launch (``vit_decode_logits``): the emission builder runs inside the
        forward pass and its rows never reach device memory -- no ``[B, T, S]`` emission tensor (44 GB for 1024 songs of 30000
        frames).  ``logits``: ``[B, T, cols]`` or ``[T, cols]`` float32 on the GPU, ``cols`` = n_bins ("softmax": n_bins + 1,
        unvoiced first); ``obs``: ``obs_params(...)``.  States and log-likelihoods are bit-identical to the builder of
        ``emissions.py`` followed by ``decode(algo="wave")``.  ``emissions_out``: an optional contiguous float32 ``[B, T, S]`` (or
        ``[T, S]``) tensor that also receives the emission rows (frames inside a song's length).  For plans with the wave form
        whose extra column is the last state (S = 321 / 361) and the reference's builder geometries; anything else raises
        ``ViterbiHipError`` before anything is enqueued.  ``workspace``: as for ``decode_checkpointed``.
        ``max_workspace_bytes``: a budget for the delta history (``plan_workspace_logits``): where the whole history does not fit,
        the decode runs as ``decode_logits_checkpointed`` with the largest segment length that does -- the same bits; that form
        writes no emissions, so ``emissions_out`` with such a budget is a ``ValueError``."""
        lg, single = self._check_logits(logits, obs, lengths)
        B, T, _ = lg.shape
        if B > 0 and max_workspace_bytes is not None:
            mode = self.plan_workspace_logits(obs, B, T, int(max_workspace_bytes))
            if mode["mode"] == "checkpointed":
                if emissions_out is not None:
                    raise ValueError(f"emissions_out needs the full-history decode, whose {self.workspace_bytes_logits(obs, B, T)} bytes of "
                                     f"workspace exceed max_workspace_bytes = {int(max_workspace_bytes)}")
                return self.decode_logits_checkpointed(logits, obs, segment_frames=mode["segment_frames"], lengths=lengths,
                                                       out_dtype=out_dtype, workspace=workspace)
        if emissions_out is not None:
            eo = emissions_out
            if (eo.dtype != torch.float32 or eo.device != self.device or not eo.is_contiguous() or
                    tuple(eo.shape) != ((T, self.S) if single else (B, T, self.S))):
                raise ValueError(f"emissions_out must be a contiguous float32 tensor shaped like the logits with {self.S} columns")
        op = ctypes.byref(self._obs_struct(obs))
        return self._decode_entry("logits", B, (B, T), torch.float32, out_dtype, workspace, (op, B, T),
                                  (lg.data_ptr(), op, B, T, _ptr(lengths)), mid=(_ptr(emissions_out),), single=single)

    def voicing(self, states: torch.Tensor, n_bins: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """voiced = state < n_bins, bins = min(state, n_bins-1) (tonet/for_paper.py:1828-1829)."""
        n_bins = self.S - 1 if n_bins is None else int(n_bins)
        st = states.to(torch.int32).contiguous()
        voiced = torch.empty(st.shape, dtype=torch.uint8, device=st.device)
        bins = torch.empty(st.shape, dtype=torch.int32, device=st.device)
        with torch.cuda.device(st.device):
            rc = _lib.load().vit_voicing_map(st.data_ptr(), st.numel(), n_bins, voiced.data_ptr(), bins.data_ptr(),
                                             torch.cuda.current_stream(st.device).cuda_stream)
        _lib.check(rc, "vit_voicing_map")
        return voiced.bool(), bins


    def voicing_notes(self, states: torch.Tensor, note_range, n_bins: Optional[int] = None):
        """(voiced, bins, notes): the voicing map plus ``notes = note_range[bins]`` with 0 where unvoiced
        (tonet/for_paper.py:2106-2115, :2207), all on the GPU."""
        n_bins = self.S - 1 if n_bins is None else int(n_bins)
        st = states.to(torch.int32).contiguous()
        nr = note_range if isinstance(note_range, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(note_range, np.float32))
        nr = nr.to(device=st.device, dtype=torch.float32).contiguous()
        if tuple(nr.shape) != (n_bins,):
            raise ValueError(f"note_range must have {n_bins} entries")
        voiced = torch.empty(st.shape, dtype=torch.uint8, device=st.device)
        bins = torch.empty(st.shape, dtype=torch.int32, device=st.device)
        notes = torch.empty(st.shape, dtype=torch.float32, device=st.device)
        with torch.cuda.device(st.device):
            rc = _lib.load().vit_voicing_notes(st.data_ptr(), st.numel(), n_bins, nr.data_ptr(), voiced.data_ptr(), bins.data_ptr(),
                                               None, notes.data_ptr(), torch.cuda.current_stream(st.device).cuda_stream)
        _lib.check(rc, "vit_voicing_notes")
        return voiced.bool(), bins, notes


_DECODERS: dict = {}


def get_decoder(transition_matrix, init_probs, device=None) -> ViterbiDecoder:
    """Decoder cache keyed by the parameter bits and the device (parameters are prepared once per
    process in the reference too: tonet/for_paper.py:281-286)."""
    A = _as_host_f32(transition_matrix)
    pi = _as_host_f32(init_probs)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (hashlib.sha256(A.tobytes()).digest(), hashlib.sha256(pi.tobytes()).digest(), A.shape, str(dev))
    dec = _DECODERS.get(key)
    if dec is None:
        if len(_DECODERS) >= 8:
            _DECODERS.pop(next(iter(_DECODERS)))
        dec = ViterbiDecoder(A, pi, dev)
        _DECODERS[key] = dec
    return dec


def decode(emission_logits: torch.Tensor, transition_matrix, init_probs, lengths: Optional[torch.Tensor] = None,
           algo: str = "auto", out_dtype: torch.dtype = torch.int64,
           max_workspace_bytes: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """decode(emission_logits, transition_matrix, init_probs) -> (states, loglik).  See module docstring.
    ``max_workspace_bytes``: the workspace budget of ``ViterbiDecoder.decode``."""
    if not isinstance(emission_logits, torch.Tensor) or emission_logits.device.type != "cuda":
        raise ValueError("emission_logits must be a torch tensor on a ROCm GPU (there is no CPU path)")
    dec = get_decoder(transition_matrix, init_probs, emission_logits.device)
    return dec.decode(emission_logits, lengths=lengths, algo=algo, out_dtype=out_dtype, max_workspace_bytes=max_workspace_bytes)
