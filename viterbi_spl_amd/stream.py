"""Streaming sessions of a ``ViterbiDecoder`` (``vit_stream_*``): the forward pass advances as emission chunks arrive.

``ViterbiDecoder.stream`` opens one; ``decoder.py`` re-exports ``DecodeStream``.  The module needs the decoder only through the
instance a session is opened on (its plan, its checks, its table of size queries), so it imports on its own.
"""
from __future__ import annotations

import ctypes
from typing import TYPE_CHECKING, Optional, Tuple

import numpy as np
import torch

from . import _lib

if TYPE_CHECKING:
    from .decoder import ViterbiDecoder


class DecodeStream:
    """One streaming session of a ``ViterbiDecoder`` (``vit_stream_*``): see ``ViterbiDecoder.stream``.  Calls are enqueued on the
    current stream of the decoder's device; the caller orders the calls of one session as for any other tensor work (one stream, or
    events).  A chunk tensor may be rewritten as soon as its ``append`` has run in stream order: nothing reads emission rows again."""

    def __init__(self, decoder: ViterbiDecoder, B: int, max_frames: Optional[int] = None, workspace: Optional[torch.Tensor] = None,
                 ring_frames: Optional[int] = None):
        self._session = ctypes.c_void_p()
        self._dec = decoder                    # (keeps the plan alive)
        self._commit_ws: Optional[torch.Tensor] = None        # the commit state, allocated by the first commit or tail
        self._commit_states: Optional[torch.Tensor] = None    # ``commit`` on a linear session: everything committed so far
        self._commit_dev: Optional[torch.Tensor] = None       # ``commit``: the frontiers on the device ...
        self._first_dev: Optional[torch.Tensor] = None        # ... and (ring sessions) where the committed range starts
        self.B = int(B)
        self._committed = np.zeros(max(self.B, 0), np.int64)  # the frontiers ``commit`` last read back (host)
        self.ring_frames = None if ring_frames is None else int(ring_frames)
        self._append_texts = None if self.ring_frames is None else {     # what an append into a full ring is told
            _lib.VIT_EWORKSPACE: f"vit_stream_append: the frames would overwrite ring rows behind the acknowledged frontier "
                                 f"(ring_frames = {self.ring_frames}): commit() first (or ack() frontiers read from commit_rel_into), "
                                 "or open the stream with a larger ring"}
        # the two session kinds differ in the size query (with its "not served" text), the open call and what counts the rows
        if self.ring_frames is not None:
            self.max_frames = None
            if self.B < 1:
                raise ValueError("a stream needs B >= 1 recordings")
            entry, open_fn, rows = "stream_ring", "vit_stream_open_ring", self.ring_frames
        else:
            if max_frames is None:
                raise ValueError("a stream needs max_frames (or ring_frames)")
            self.max_frames = int(max_frames)
            if self.B < 1 or self.max_frames < 1:
                raise ValueError("a stream needs B >= 1 recordings and max_frames >= 1")
            entry, open_fn, rows = "stream", "vit_stream_open", self.max_frames
        self._ws, ws_ptr, ws_bytes, _ = decoder._call_workspace(decoder._need(entry, True, self.B, rows), workspace)
        _lib.check(getattr(_lib.load(), open_fn)(decoder._plan, self.B, rows, ws_ptr, ws_bytes, ctypes.byref(self._session)), open_fn)

    def _handle(self) -> ctypes.c_void_p:
        if not self._session.value:
            raise _lib.ViterbiHipError("the stream is closed")
        return self._session

    def _enqueue(self, name: str, *args, texts: Optional[dict] = None) -> None:
        """``vit_stream_<name>(session, *args, stream)`` in the decoder's device context, on its current stream; `texts`: status ->
        the session's own wording of a refusal."""
        dev = self._dec.device
        with torch.cuda.device(dev):
            rc = getattr(_lib.load(), "vit_stream_" + name)(self._handle(), *args, torch.cuda.current_stream(dev).cuda_stream)
        if texts and rc in texts:
            raise _lib.ViterbiHipError(texts[rc])
        _lib.check(rc, "vit_stream_" + name)

    # ------------------------------------------------------------------ checks
    def _check_states(self, states: torch.Tensor) -> None:
        if states.dtype != torch.int32 or states.dim() != 2 or states.shape[0] != self.B or not states.is_contiguous() or states.device != self._dec.device:
            raise ValueError("states must be a contiguous int32 [B, stride] tensor on the decoder's device")

    def _check_i64(self, x: torch.Tensor, name: str) -> None:
        if x.dtype != torch.int64 or tuple(x.shape) != (self.B,) or not x.is_contiguous() or x.device != self._dec.device:
            raise ValueError(f"{name} must be an int64 [B] tensor on the decoder's device")

    def _check_loglik(self, loglik: Optional[torch.Tensor]) -> Optional[int]:
        """-> the address of an optional float32 [B] log-likelihood tensor (None for None)."""
        if loglik is None:
            return None
        if loglik.dtype != torch.float32 or tuple(loglik.shape) != (self.B,) or not loglik.is_contiguous() or loglik.device != self._dec.device:
            raise ValueError("loglik must be a float32 [B] tensor on the decoder's device")
        return loglik.data_ptr()

    # ------------------------------------------------------------------ frames in, the whole path out
    def append(self, emissions: torch.Tensor, counts=None) -> None:
        """The next frames: ``emissions`` [B, n, S] (or [n, S] for a one-recording stream), float32 or float16 (the type of the
        first append holds for the session); ``counts``: a host sequence of B ints, recording b takes rows ``[b, :counts[b]]``
        (None: n each).  Raises ``ViterbiHipError`` -- with nothing enqueued and no length changed -- for a count out of range or
        frames beyond ``max_frames``."""
        logE, _, dt = self._dec._check_emissions(emissions)
        if logE.shape[0] != self.B:
            raise ValueError(f"emissions must be [{self.B}, n, {self._dec.S}]")
        cnt = None
        if counts is not None:
            cnt = np.ascontiguousarray(np.asarray(counts, dtype=np.int64))
            if cnt.shape != (self.B,):
                raise ValueError("counts must hold one entry per recording")
        self._enqueue("append", logE.data_ptr(), dt, int(logE.shape[1]), cnt.ctypes.data if cnt is not None else None, texts=self._append_texts)

    @property
    def lengths(self) -> np.ndarray:
        """Frames appended per recording so far (host int64 [B])."""
        out = np.zeros(self.B, np.int64)
        _lib.check(_lib.load().vit_stream_lengths(self._handle(), out.ctypes.data), "vit_stream_lengths")
        return out

    def decode_into(self, states: torch.Tensor, loglik: Optional[torch.Tensor] = None) -> None:
        """Enqueue the back-trace of the recordings as they stand: ``states`` int32 [B, stride], stride >= the longest length (-1
        behind each length), ``loglik`` float32 [B] or None."""
        if self.ring_frames is not None:
            raise _lib.ViterbiHipError("decode() needs every history row: a ring session returns its path by commit() and tail()")
        self._check_states(states)
        self._enqueue("backtrace", states.data_ptr(), int(states.shape[1]), self._check_loglik(loglik))

    def decode(self, out_dtype: torch.dtype = torch.int64) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> ``(states [B, max length so far], loglik [B])`` of the frames appended so far; the session stays open, and a later
        ``decode`` after more appends supersedes this one."""
        states = torch.empty((self.B, int(self.lengths.max())), dtype=torch.int32, device=self._dec.device)
        loglik = torch.empty((self.B,), dtype=torch.float32, device=self._dec.device)
        self.decode_into(states, loglik)
        return (states if out_dtype == torch.int32 else states.to(out_dtype)), loglik

    # ------------------------------------------------------------------ commit point
    # the default lookback of ``commit`` / ``commit_into``: no cap (2^30 frames, the most vit_stream_commit takes)
    MAX_LOOKBACK = 1 << 30

    def _commit_begin(self) -> None:
        """Allocate and bind the commit state on the first call that needs it (a closed session raises first)."""
        self._handle()
        if self._commit_ws is not None:
            return
        ws, ptr, nbytes, _ = self._dec._call_workspace(self._dec._need("stream_commit", True, self.B), None)
        _lib.check(_lib.load().vit_stream_commit_begin(self._handle(), ptr, nbytes), "vit_stream_commit_begin")
        self._commit_ws = ws

    def commit_into(self, states: torch.Tensor, committed: torch.Tensor, max_lookback: Optional[int] = None) -> None:
        """Enqueue ``vit_stream_commit``: for every recording the states of the frames that became final since the last commit are
        written to ``states[b, f_b:f'_b]`` (int32 [B, stride], stride >= the longest length; nothing else of it is touched) and the
        new frontier f'_b to ``committed[b]`` (int64 [B]).  Asynchronous: no host synchronisation.  ``max_lookback``: the most
        frames behind the newest one in which the merge of the survivor paths is looked for (None: no cap).  The commit state is
        allocated on the first call."""
        if self.ring_frames is not None:
            raise _lib.ViterbiHipError("commit_into writes at absolute frames: a ring session commits with commit_rel_into (or commit())")
        self._check_states(states)
        self._check_i64(committed, "committed")
        self._commit_begin()
        self._enqueue("commit", states.data_ptr(), int(states.shape[1]), committed.data_ptr(),
                      self.MAX_LOOKBACK if max_lookback is None else int(max_lookback))

    def commit_rel_into(self, states: torch.Tensor, first: torch.Tensor, committed: torch.Tensor, max_lookback: Optional[int] = None) -> None:
        """Enqueue ``vit_stream_commit_rel``: ``commit_into`` with a window-relative output -- the states of the frames
        ``[f_b, f'_b)`` that became final go to ``states[b, :f'_b - f_b]`` (int32 [B, stride]; on a ring session stride >=
        min(longest length, ring_frames) suffices), ``first[b] = f_b`` and ``committed[b] = f'_b`` (int64 [B] each); nothing else is
        written.  Asynchronous.  On a ring session, report the frontiers you read back with ``ack`` so that appends may go on."""
        self._check_states(states)
        self._check_i64(first, "first")
        self._check_i64(committed, "committed")
        self._commit_begin()
        self._enqueue("commit_rel", states.data_ptr(), int(states.shape[1]), first.data_ptr(), committed.data_ptr(),
                      self.MAX_LOOKBACK if max_lookback is None else int(max_lookback))

    def ack(self, frontiers) -> None:
        """Ring sessions: tell the session the frontiers (host, B ints) READ BACK from a ``committed`` tensor of an earlier commit;
        rows below them may then be overwritten by appends (``vit_stream_commit_ack``: host only).  Values that go down or lie
        beyond the lengths raise.  Acknowledging values that were not read gives wrong states."""
        fr = np.ascontiguousarray(np.asarray(frontiers, dtype=np.int64))
        if fr.shape != (self.B,):
            raise ValueError("frontiers must hold one entry per recording")
        _lib.check(_lib.load().vit_stream_commit_ack(self._handle(), fr.ctypes.data), "vit_stream_commit_ack")

    def tail_into(self, states: torch.Tensor, first: torch.Tensor, loglik: Optional[torch.Tensor] = None) -> None:
        """Enqueue ``vit_stream_tail``: the best path of the frames so far, restricted to the frames behind the frontier:
        ``states[b, :n_b - f_b]`` (int32 [B, stride], stride >= the longest possible tail), ``first[b] = f_b`` (int64 [B]),
        ``loglik`` float32 [B] or None.  The frontier does not move.  Asynchronous; ring and linear sessions alike."""
        self._check_states(states)
        self._check_i64(first, "first")
        ll_ptr = self._check_loglik(loglik)
        self._commit_begin()
        self._enqueue("tail", states.data_ptr(), int(states.shape[1]), first.data_ptr(), ll_ptr)

    def _window(self) -> int:
        n = max(int(self.lengths.max()), 1)
        return n if self.ring_frames is None else min(n, self.ring_frames)

    def _rows(self, stride: int) -> torch.Tensor:
        return torch.empty((self.B, stride), dtype=torch.int32, device=self._dec.device)

    def _frontiers(self) -> torch.Tensor:
        return torch.zeros((self.B,), dtype=torch.int64, device=self._dec.device)

    @staticmethod
    def _ranges(states: torch.Tensor, lo, hi, out_dtype: torch.dtype) -> list:
        """``[states[b, lo_b:hi_b]]`` of every recording as ``out_dtype``."""
        out = [states[b, int(lo[b]):int(hi[b])] for b in range(len(hi))]
        return out if out_dtype == torch.int32 else [x.to(out_dtype) for x in out]

    def tail(self, out_dtype: torch.dtype = torch.int64):
        """-> ``(first (host int64 [B]), [the states of frames [f_b, n_b) of recording b], loglik [B])``: with the commits so far,
        the whole best path of the frames appended.  SYNCHRONISES to read the slice bounds."""
        states, first = self._rows(self._window()), self._frontiers()
        loglik = torch.empty((self.B,), dtype=torch.float32, device=self._dec.device)
        n = self.lengths
        self.tail_into(states, first, loglik)
        f = first.cpu().numpy().astype(np.int64)
        return f, self._ranges(states, np.zeros_like(f), n - f, out_dtype), loglik

    def _commit_ring(self, max_lookback: Optional[int], out_dtype: torch.dtype):
        if self._first_dev is None:
            self._commit_dev, self._first_dev = self._frontiers(), self._frontiers()
        states = self._rows(self._window())
        self.commit_rel_into(states, self._first_dev, self._commit_dev, max_lookback)
        first = self._first_dev.cpu().numpy().astype(np.int64)
        new = self._commit_dev.cpu().numpy().astype(np.int64)
        self.ack(new)
        self._committed = new
        return first, new.copy(), self._ranges(states, np.zeros_like(new), new - first, out_dtype)

    def commit(self, max_lookback: Optional[int] = None, out_dtype: torch.dtype = torch.int64):
        """-> ``(committed lengths (host int64 [B]), [the newly final states of recording b: frames [f_b, f'_b)])``.  The slice
        bounds live on the device, so this call SYNCHRONISES with the stream to read them; ``commit_into`` does not.  The session
        keeps an int32 [B, max_frames] tensor of everything committed so far (``committed_states``).  Use either ``commit`` or
        ``commit_into`` on one session between resets: both advance the same device frontiers, and ``commit`` slices by the ones it read.

        On a RING session the result is ``(first, committed, [states of frames [first_b, committed_b)])`` (``commit_rel_into``), the
        frontiers read are acknowledged so that appends may reuse the rows below them, and no tensor of everything committed is kept."""
        if self.ring_frames is not None:
            return self._commit_ring(max_lookback, out_dtype)
        if self._commit_states is None:
            self._commit_states, self._commit_dev = self._rows(self.max_frames), self._frontiers()
        self.commit_into(self._commit_states, self._commit_dev, max_lookback)
        new = self._commit_dev.cpu().numpy().astype(np.int64)
        old, self._committed = self._committed, new
        return new.copy(), self._ranges(self._commit_states, old, new, out_dtype)

    @property
    def committed_states(self) -> Optional[torch.Tensor]:
        """int32 [B, max_frames]: row b holds the final states of frames [0, committed length) as of the last ``commit`` (None before)."""
        return self._commit_states

    def reset(self) -> None:
        """Every recording back to length 0 and every commit frontier to 0; the workspace is reused."""
        _lib.check(_lib.load().vit_stream_reset(self._handle()), "vit_stream_reset")
        self._committed = np.zeros(self.B, np.int64)

    def close(self) -> None:
        """Free the session (also on garbage collection).  The workspace tensor is released with the object."""
        try:
            if self._session.value:
                _lib.load().vit_stream_close(self._session)
                self._session = ctypes.c_void_p()
        except Exception:
            pass

    def __del__(self):
        self.close()
