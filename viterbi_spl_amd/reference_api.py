"""Signature-compatible adapters for the reference's Viterbi entry points.

Same names, keyword arguments, argument meaning and assertion behaviour as the reference
functions they replace (paths relative to the reference repo); the forward recursion and the
back-trace run on the GPU through ``ViterbiDecoder``.  The prob -> log step stays on the host in
NumPy float32 exactly where the reference does it, because ``np.log`` is the one operation whose
last bit a GPU cannot be trusted to reproduce.

  family A  viterbi_librosa_c_fn / viterbi_numba_fn(*, transition_matrix, prob_init, probs_st)
            dcnet/tf_viterbi_decoding.py:119-207, dcnet/main.py:2417-2468 (+10 copies)
  float64   viterbi_librosa_f64_fn(*, transition_matrix, prob_init, probs_st)    dcnet/tf_viterbi_decoding.py:209-263
            viterbi_librosa_f64_recordings_fn(*, transition_matrix, prob_init, probs_st_list)   the same, many recordings in one call
  family D  viterbi_librosa_fn(*, log_transition_matrix_T, log_prob_init, log_probs_st)
            imm/tf_viterbi.py:75-109
  AOT core  viterbi_numba_core(B, prob_init, probs)   dcnet/aot_viterbi_core.py:8-54
  TF graph  viterbi_tf_fn(transition_matrix, prob_init, probs_st) -> int32        dcnet/tf_viterbi_decoding.py:23-72
  TF eager  tf_viterbi_librosa_fn(*, tf_log_transition_matrix_T, ...) -> int32    imm/tf_viterbi.py:8-72
  family B  Viterbi.viterbi_librosa_fn(self, probs_st)          tonet/for_paper.py:1833-1870
  family C  SoftMaxViterbi.viterbi_librosa_fn(self, probs_ts)   tonet/for_paper.py:1999-2037
  imm       Viterbi(bins_per_semitone, n_bins).__call__(HF0)    imm/tf_imm.py:48-135, call site :692  (ImmViterbi here)
"""
from __future__ import annotations

import numpy as np
import torch

from .decoder import ViterbiDecoder, get_decoder

_TINY = np.finfo(np.float32).tiny


def _run(logA_T: np.ndarray, log_pi: np.ndarray, logE_ts: np.ndarray, decoder: ViterbiDecoder | None = None) -> np.ndarray:
    dec = decoder if decoder is not None else get_decoder(logA_T, log_pi)
    e = torch.from_numpy(np.ascontiguousarray(logE_ts, dtype=np.float32)).to(dec.device)
    states, _ = dec.decode(e, out_dtype=torch.int64)
    return states.cpu().numpy()


# ----------------------------------------------------------------------------- family D
def viterbi_librosa_fn(*, log_transition_matrix_T, log_prob_init, log_probs_st):
    """Log-domain core (imm/tf_viterbi.py:75-109): emissions are [S, T]; returns int64[T]."""
    B = log_transition_matrix_T
    assert B.flags['C_CONTIGUOUS']
    assert B.dtype == np.float32
    S = len(B)
    assert len(log_prob_init) == S
    assert log_probs_st.dtype == np.float32
    assert log_probs_st.shape[0] == S
    logE = np.require(log_probs_st.T, requirements=['C'])
    return _run(B, np.asarray(log_prob_init, np.float32), logE)


# ----------------------------------------------------------------------------- family A
def _check_probs(transition_matrix, prob_init, probs_st):
    # float32 inputs only: with float64 parameters the reference's NumPy code (dcnet/tf_viterbi_decoding.py:183-197) adds a
    # float32 delta to float64 log-probabilities and rounds once, which float32 kernels do not reproduce; the compiled core it
    # replaces takes f4 arrays only ('i8[:](f4[:, ::1], f4[:], f4[:, ::1])', dcnet/aot_viterbi_core.py:8)
    assert transition_matrix.dtype == np.float32 and np.asarray(prob_init).dtype == np.float32 and probs_st.dtype == np.float32
    S = len(transition_matrix)
    assert transition_matrix.shape == (S, S)
    assert probs_st.shape[0] == S and probs_st.ndim == 2
    assert np.allclose(np.sum(transition_matrix, axis=1), 1.)
    assert len(prob_init) == S
    assert np.isclose(np.sum(prob_init), 1.)
    return S


def viterbi_librosa_c_fn(*, transition_matrix, prob_init, probs_st):
    """Probabilities in, [S, T] emissions (dcnet/tf_viterbi_decoding.py:156-207); int64[T] out."""
    _check_probs(transition_matrix, prob_init, probs_st)
    tinyp = np.finfo(probs_st.dtype).tiny
    logA_T = np.require(np.log(transition_matrix.T + tinyp), np.float32, ['C'])
    log_pi = np.log(prob_init + tinyp).astype(np.float32)
    logE = np.require(np.log(probs_st.T + tinyp), np.float32, ['C'])
    return _run(logA_T, log_pi, logE)


def viterbi_librosa_f64_fn(*, transition_matrix, prob_init, probs_st):
    """dcnet's float64 function, ``viterbi_librosa_fn`` at dcnet/tf_viterbi_decoding.py:209-263 (that name is imm's log-domain
    function here, hence the suffix): float32 probabilities in, the log taken on the host, the running score T1 in float64
    (``ViterbiDecoder.decode_f64``); int64[T] out.  float64 parameters stay refused as in the other adapters."""
    S = _check_probs(transition_matrix, prob_init, probs_st)
    assert probs_st.shape == (S, probs_st.shape[1])
    tinyp = np.finfo(probs_st.dtype).tiny
    logA_T = np.require(np.log(transition_matrix.T + tinyp), np.float32, ['C'])
    log_pi = np.log(prob_init + tinyp).astype(np.float32)
    logE = np.require(np.log(probs_st.T + tinyp), np.float32, ['C'])
    dec = get_decoder(logA_T, log_pi)
    states, _ = dec.decode_f64(torch.from_numpy(logE).to(dec.device), out_dtype=torch.int64)
    return states.cpu().numpy()


def viterbi_librosa_f64_recordings_fn(*, transition_matrix, prob_init, probs_st_list, max_workspace_bytes=None):
    """``viterbi_librosa_f64_fn`` over many recordings of different lengths in ONE packed decode
    (``ViterbiDecoder.decode_f64_packed``; the reference calls its function once per recording, as at tonet/for_paper.py:2304-2309):
    ``probs_st_list`` holds one float32 ``[S, T_b]`` array per recording; a list of ``int64[T_b]`` comes back, entry b equal to
    ``viterbi_librosa_f64_fn`` of recording b alone.  The asserts and the host ``np.log`` step are that function's, per recording.
    ``max_workspace_bytes``: a budget for the decode's workspace, met by segments (``ViterbiDecoder.decode_f64_packed_bounded``) --
    the same paths; ``ViterbiHipError`` when nothing fits."""
    probs_st_list = list(probs_st_list)
    if not probs_st_list:
        return []
    parts = []
    for probs_st in probs_st_list:
        S = _check_probs(transition_matrix, prob_init, probs_st)
        assert probs_st.shape == (S, probs_st.shape[1])
        parts.append(np.require(np.log(probs_st.T + np.finfo(probs_st.dtype).tiny), np.float32, ['C']))
    tinyp = np.finfo(np.float32).tiny
    logA_T = np.require(np.log(transition_matrix.T + tinyp), np.float32, ['C'])
    log_pi = np.log(prob_init + tinyp).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int64)
    dec = get_decoder(logA_T, log_pi)
    logE = torch.from_numpy(np.concatenate(parts, axis=0)).to(dec.device)
    if max_workspace_bytes is None:
        states, _ = dec.decode_f64_packed(logE, offsets, out_dtype=torch.int64)
    else:
        states, _ = dec.decode_f64_packed_bounded(logE, offsets, max_workspace_bytes=int(max_workspace_bytes), out_dtype=torch.int64)
    states = states.cpu().numpy()
    return [states[offsets[b]:offsets[b + 1]] for b in range(len(parts))]


def viterbi_numba_fn(*, transition_matrix, prob_init, probs_st):
    """The marshalling wrapper around the AOT core (dcnet/tf_viterbi_decoding.py:119-153)."""
    _check_probs(transition_matrix, prob_init, probs_st)
    B = np.require(transition_matrix.T, requirements=['C']).copy()
    probs = np.require(probs_st.T, requirements=['C']).copy()
    return viterbi_numba_core(B, prob_init.copy(), probs)


def viterbi_numba_core(B, prob_init, probs):
    """Stand-in for ``viterbi_numba.core`` ('i8[:](f4[:, ::1], f4[:], f4[:, ::1])',
    dcnet/aot_viterbi_core.py:8-54).  B is [S,S] "target <- source", probs is [T,S].
    Like the Numba core it log-transforms its arguments IN PLACE (:23-25)."""
    assert B.dtype == np.float32 and prob_init.dtype == np.float32 and probs.dtype == np.float32
    assert B.flags['C_CONTIGUOUS'] and probs.flags['C_CONTIGUOUS']
    S = B.shape[0]
    assert prob_init.shape[0] == S and probs.shape[1] == S
    tinyp = np.float32(1.1754944e-38)
    B[:] = np.log(B + tinyp)
    prob_init[:] = np.log(prob_init + tinyp)
    probs[:] = np.log(probs + tinyp)
    return _run(B, prob_init, probs)


# ----------------------------------------------------------------------------- the TensorFlow variants (rows a3 / a7)
def _to_numpy(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    return x.numpy() if hasattr(x, 'numpy') else np.asarray(x)       # tf.Tensor / tf.Variable expose .numpy() as well


def viterbi_tf_fn(transition_matrix, prob_init, probs_st):
    """Call surface of the TF-graph variant (dcnet/tf_viterbi_decoding.py:23-72): positional probabilities in (tensors or
    arrays, converted to float32 as ``tf.convert_to_tensor(..., tf.float32)`` does), S hard-wired to 321 there, the
    ``tf.debugging.assert_near`` checks on the row sums, ``int32[T]`` states out.  Same float32 recursion as family A; the
    log is NumPy's here (TensorFlow's own log may differ in the last bit: that variant's outputs are parity unpinned)."""
    A = np.asarray(_to_numpy(transition_matrix), np.float32)
    pi = np.asarray(_to_numpy(prob_init), np.float32)
    P = np.asarray(_to_numpy(probs_st), np.float32)
    assert np.allclose(np.sum(A, axis=1), 1., atol=1e-6 * A.shape[1]) and np.isclose(np.sum(pi), 1., atol=1e-5)
    return viterbi_librosa_c_fn(transition_matrix=A, prob_init=pi, probs_st=np.asfortranarray(P)).astype(np.int32)


def tf_viterbi_librosa_fn(*, tf_log_transition_matrix_T, tf_log_prob_init, tf_or_np_log_probs_st):
    """Call surface of the TF-eager log-domain variant (imm/tf_viterbi.py:8-72): ``[S,S]`` target <- source log-matrix,
    ``[S]`` log-prior, ``[S,T]`` log-emissions (tensor or array, taken as float32), ``int32[T]`` states out."""
    B = np.require(_to_numpy(tf_log_transition_matrix_T), np.float32, ['C'])
    prob_init = np.asarray(_to_numpy(tf_log_prob_init), np.float32)
    probs = np.asarray(_to_numpy(tf_or_np_log_probs_st), np.float32)
    S = len(B)
    assert B.shape == (S, S)
    assert len(prob_init) == S
    assert probs.shape == (S, probs.shape[1])
    return viterbi_librosa_fn(log_transition_matrix_T=B, log_prob_init=prob_init, log_probs_st=probs).astype(np.int32)


# ----------------------------------------------------------------------------- families B / C
class _PreparedViterbi:
    """Parameters logged and transposed once (tonet/for_paper.py:1780-1815).

    ``emission_dtype``: storage of the emission tensor the GPU builder writes for ``decode_logits`` / ``decode_logits_batch`` /
    ``decode_recordings`` (and ``RecordingAccumulator``), "float32" or "float16".  With "float16" every float32 emission is rounded to
    nearest even as the builder stores it (``vit_obs_build``): half the tensor, and no float32 tensor on the way.  Float16 rows are a
    DIFFERENT decoder input: the result is the reference decoder's result on the rounded rows (bit for bit), not on the float32 rows
    (on the synthetic logits of scripts/obs_half_time.py the two differ in 3.75e-5 of the frames at [1024 x 30000, 360] and 1.9e-5 at
    [256 x 30000, 722]; on the first shape builder + decode is 1.08x slower with float16 rows than with float32 rows, on the second as
    fast: profiles/obs_half_time.json).
    Logits may be float32 or float16 torch tensors (float16 is widened exactly inside the builder: the result of their
    ``.float()`` copy); NumPy logits are converted to float32 as before.  ``emission_dtype`` is fixed at construction: it is read
    through ``_torch_dtype()`` at every call, so do not assign to it while a ``RecordingAccumulator`` or a stream over this object is open."""

    def __init__(self, transition_matrix, init_probs, num_freq_bins=None, device=None, emission_dtype="float32"):
        if emission_dtype not in ("float32", "float16"):
            raise ValueError('emission_dtype must be "float32" or "float16"')
        self.emission_dtype = emission_dtype
        transition_matrix = np.asarray(transition_matrix)
        init_probs = np.asarray(init_probs)
        U = transition_matrix.shape[0] - 1 if num_freq_bins is None else int(num_freq_bins)
        self.num_freq_bins = U
        assert transition_matrix.shape == (U + 1, U + 1)
        assert np.all(np.isclose(np.sum(transition_matrix, axis=1), 1))
        assert init_probs.shape == (U + 1,)
        assert np.isclose(np.sum(init_probs), 1)
        tiny = np.finfo(np.float32).tiny
        t = np.log(transition_matrix + tiny)
        assert not np.any(np.isneginf(t))
        t = np.require(t.T, np.float32, ['C'])
        t.flags['WRITEABLE'] = False
        self.log_transition_matrix_T = t
        p = np.log(init_probs + tiny)
        assert not np.any(np.isneginf(p))
        p = np.require(p, np.float32)
        p.flags['WRITEABLE'] = False
        self.log_ini_probs = p
        self.ini_probs = init_probs
        self._decoder = ViterbiDecoder(t, p, device)

    @classmethod
    def from_dat_files(cls, transition_file, init_file, **kw):
        from .datfile import load_np_array_from_file_fn
        name, A = load_np_array_from_file_fn(transition_file)
        assert name == 'viterbi_transition_matrix'
        name, pi = load_np_array_from_file_fn(init_file)
        assert name == 'viterbi_init_probs'
        return cls(A, pi, **kw)

    def _torch_dtype(self):
        return torch.float16 if self.emission_dtype == "float16" else torch.float32

    def _post(self, bins):
        n_bins = self.num_freq_bins
        voiced = bins < n_bins
        bins = np.minimum(bins, n_bins - 1)
        return voiced, bins

    # ---- the post-processor on the GPU: logits -> log-emissions -> decode -> (voiced, bins)
    def _log_emissions(self, logits: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """This class's stand-alone emission builder: ``[frames, columns]`` logits (float32 or float16) -> ``[frames, S]`` log-emissions
        in ``emission_dtype`` (into ``out`` when given)."""
        raise NotImplementedError

    def decode_logits(self, logits, note_range=None):
        """Whole post-processor with everything on the GPU.  logits: NumPy or torch, ``[frames, columns]``.
        Returns torch tensors on the decoder's device: ``(voiced bool[T], bins int32[T])``, plus ``notes float32[T]``
        (``note_range[bins]``, 0 where unvoiced: tonet/for_paper.py:2106-2115, :2207) when ``note_range`` is given."""
        lg = logits if isinstance(logits, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(logits, np.float32))
        lg = lg.to(self._decoder.device).contiguous()
        states, _ = self._decoder.decode(self._log_emissions(lg), out_dtype=torch.int32)
        if note_range is None:
            return self._decoder.voicing(states, self.num_freq_bins)
        return self._decoder.voicing_notes(states, note_range, self.num_freq_bins)

    def _obs_params(self) -> dict:
        """This class's emission-builder arguments for ``ViterbiDecoder.decode_logits``, computed as emissions.py computes them."""
        raise NotImplementedError

    def decode_logits_batch(self, logits, lengths=None, note_range=None, fused=False, max_workspace_bytes=None):
        """``decode_logits`` over a batch: logits ``[B, frames, columns]`` (NumPy or torch), ``lengths`` an optional int64 ``[B]``
        tensor (frames past a song's length: voiced False, bins -1).  Returns ``(voiced bool[B, T], bins int32[B, T])`` plus
        ``notes float32[B, T]`` when ``note_range`` is given; row b equals ``decode_logits(logits[b])``.
        ``fused=False``: the emission builder into a ``[B, T, S]`` tensor, then ``decode``.  ``fused=True``: one forward launch that
        builds the emissions where they are consumed (``ViterbiDecoder.decode_logits``; no emission tensor: B * T * S * 4 bytes
        less device memory), the same bits; raises ``ViterbiHipError`` where the plan is not served (the 722-state grids).
        Measured on one MI355X (`[B, 30000, 360]`, profiles/fused_logits_time.json): the fused path is slower at every batch size --
        2.7x at 256 songs, 1.7x at 512, 1.23-1.27x at 1024 and 2048 -- there is no crossover, so it is for batches whose emission
        tensor does not fit, and the default stays unfused.
        ``max_workspace_bytes``: a budget for the decoder's workspace; the same result.  ``fused=True``: ``ViterbiDecoder.decode_logits``
        falls to the checkpointed fused decode (``vit_decode_logits_checkpointed``: neither an emission tensor nor a whole delta
        history); ``fused=False``: ``ViterbiDecoder.decode(max_workspace_bytes=)``, which still needs the emission tensor.
        The fused kernels are float32 only (there is no emission tensor to shrink): ``fused=True`` raises ``ValueError`` with
        ``emission_dtype="float16"`` or float16 logits."""
        dev = self._decoder.device
        lg = logits if isinstance(logits, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(logits, np.float32))
        lg = lg.to(dev).contiguous()
        assert lg.dim() == 3
        if fused and (self.emission_dtype != "float32" or lg.dtype == torch.float16):
            raise ValueError('fused=True decodes float32 logits through float32 emission rows only: use fused=False with '
                             'emission_dtype="float16" or float16 logits')
        if lengths is not None:
            lengths = (lengths if isinstance(lengths, torch.Tensor) else torch.as_tensor(np.asarray(lengths), dtype=torch.int64)).to(dev)
        if fused:
            states, _ = self._decoder.decode_logits(lg, self._obs_params(), lengths=lengths, out_dtype=torch.int32,
                                                    max_workspace_bytes=max_workspace_bytes)
        else:
            states, _ = self._decoder.decode(self._log_emissions(lg), lengths=lengths, out_dtype=torch.int32,
                                             max_workspace_bytes=max_workspace_bytes)
        if note_range is None:
            return self._decoder.voicing(states, self.num_freq_bins)
        return self._decoder.voicing_notes(states, note_range, self.num_freq_bins)

    def decode_recordings(self, logits_list, max_workspace_bytes=None):
        """Many recordings in ONE pass: what the reference does recording by recording (one ``viterbi(logits)`` call each,
        tonet/for_paper.py:2304-2319) as a single emission-builder launch over the concatenated frames, a single packed decode
        (``vit_decode_packed``: no padding, forward slots packed by length) and a single voicing map.  ``logits_list``: NumPy or torch
        ``[T_b, columns]`` per recording.  Returns a list of ``(voiced bool[T_b], bins int32[T_b])`` torch tensors on the GPU;
        every pair equals ``decode_logits`` of that recording alone (the builders work frame by frame, the decode is bit-identical).
        ``max_workspace_bytes``: a budget for the decoder's workspace (``ViterbiDecoder.decode_packed``: the checkpointed packed decode
        where the full delta history does not fit; the same result)."""
        dev = self._decoder.device
        parts = [(lg if isinstance(lg, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(lg, np.float32))).to(dev) for lg in logits_list]
        if not parts:
            return []
        offsets = np.concatenate([[0], np.cumsum([int(x.shape[0]) for x in parts])]).astype(np.int64)
        assert all(x.dim() == 2 and x.shape[1] == parts[0].shape[1] and x.shape[0] >= 1 for x in parts)
        E = self._log_emissions(torch.cat(parts, dim=0).contiguous())
        states, _ = self._decoder.decode_packed(E, offsets, out_dtype=torch.int32, max_workspace_bytes=max_workspace_bytes)
        voiced, bins = self._decoder.voicing(states, self.num_freq_bins)
        return [(voiced[offsets[b]:offsets[b + 1]], bins[offsets[b]:offsets[b + 1]]) for b in range(len(parts))]

    def __call__(self, logits):
        """``viterbi(logits) -> (voiced bool[T], bins int64[T])`` as NumPy arrays, the reference's call surface
        (tonet/for_paper.py:1817-1831, :2309).  The observation probabilities are built on the GPU (``vit_obs_*``: peak
        picking, voicing decision and structural zeros exact; exp / log / sums within a few ulp of NumPy's).  Measured
        against the host-exact pipeline (tests/test_gpu_parity.py::test_postprocessor_agreement_at_full_length): T = 30000,
        five seeds per builder ("shaun", softmax, scaled likelihoods) -- 100 % of the frames of all fifteen songs decode to
        the reference's states; the test's bar is 99.9 % per song with every differing frame on a path whose exact score
        ties the reference's to 1e-6.  Callers that need the reference's bits by construction build the probabilities
        themselves and call :meth:`viterbi_librosa_fn`, which is bit-exact.  All of this is the default, ``emission_dtype="float32"``:
        with ``"float16"`` the call returns the decode of the rounded rows (see the class docstring), which is not the reference's
        result on the float32 rows."""
        voiced, bins = self.decode_logits(logits)
        return voiced.cpu().numpy(), bins.cpu().numpy().astype(np.int64)


class Viterbi(_PreparedViterbi):
    """Family B (tonet/for_paper.py:1683-1870).  ``viterbi_librosa_fn`` takes F-contiguous [S, T]
    probabilities and logs them IN PLACE, as in the reference.  ``__call__(logits)`` is the whole
    post-processor (:1817-1831): emission builder -> decode -> (voiced, bins)."""

    def __init__(self, transition_matrix, init_probs, voicing_threshold=0.32, num_freq_bins=None, device=None, emission_dtype="float32"):
        super().__init__(transition_matrix, init_probs, num_freq_bins, device, emission_dtype)
        assert 0 < voicing_threshold < 1
        self.voicing_threshold = voicing_threshold
        self.threshold = np.log(voicing_threshold / (1. - voicing_threshold))
        self.single_side_peak_width = 5

    def viterbi_librosa_fn(self, probs_st):
        S = self.num_freq_bins + 1
        assert probs_st.shape[0] == S
        assert probs_st.dtype == np.float32
        assert probs_st.flags['F_CONTIGUOUS']
        np.add(probs_st, _TINY, out=probs_st)
        np.log(probs_st, out=probs_st)
        probs = np.require(probs_st.T, np.float32, ['C'])
        return _run(self.log_transition_matrix_T, self.log_ini_probs, probs, self._decoder)

    def _log_emissions(self, logits, out=None):
        from .emissions import shaun_log_emissions
        return shaun_log_emissions(logits, self.voicing_threshold, self.single_side_peak_width, out=out, dtype=self._torch_dtype())

    def _obs_params(self):
        import math
        th, p = self.voicing_threshold, 0.8                 # shaun_log_emissions' defaults: p = 0.8, scale = 2.0
        return ViterbiDecoder.obs_params("shaun", self.num_freq_bins, self.single_side_peak_width, math.log(th / (1.0 - th)),
                                         math.log(p / (1.0 - p)), 2.0)


class SoftMaxViterbi(_PreparedViterbi):
    """Family C (tonet/for_paper.py:1873-2037): C-contiguous [T, S] probabilities (values may
    exceed 1 for scaled likelihoods), logged IN PLACE.  ``__call__(logits)`` as above; logits carry the unvoiced
    column first ([T, n_bins+1])."""

    def __init__(self, transition_matrix, init_probs, num_freq_bins=None, device=None, emission_dtype="float32"):
        super().__init__(transition_matrix, init_probs, num_freq_bins, device, emission_dtype)
        self.single_side_peak_width = 15

    def viterbi_librosa_fn(self, probs_ts):
        S = self.num_freq_bins + 1
        assert probs_ts.ndim == 2
        assert probs_ts.shape[1] == S
        assert probs_ts.dtype == np.float32
        assert probs_ts.flags['C_CONTIGUOUS']
        np.add(probs_ts, _TINY, out=probs_ts)
        np.log(probs_ts, out=probs_ts)
        return _run(self.log_transition_matrix_T, self.log_ini_probs, probs_ts, self._decoder)

    def _log_emissions(self, logits, out=None):
        from .emissions import softmax_log_emissions
        return softmax_log_emissions(logits, self.single_side_peak_width, out=out, dtype=self._torch_dtype())

    def _obs_params(self):
        return ViterbiDecoder.obs_params("softmax", self.num_freq_bins, self.single_side_peak_width)


class ScaledSoftMaxViterbi(SoftMaxViterbi):
    """dcnet's SoftMaxViterbi (dcnet/softmax_viterbi.py:2486-2674; same class in ftanet / jdc / msnet): logits carry
    the n_bins pitch columns only, the unvoiced logit is the voicing-threshold logit, peaks use a +/-5-bin window and --
    with ``scaled=True`` -- every softmax probability is divided by its state prior ("scaled likelihood": values far
    above 1, i.e. positive log-emissions)."""

    def __init__(self, transition_matrix, init_probs, voicing_threshold_prob, scaled, num_freq_bins=None, device=None, emission_dtype="float32"):
        super().__init__(transition_matrix, init_probs, num_freq_bins, device, emission_dtype)
        assert 0 < voicing_threshold_prob < 1
        self.voicing_threshold_prob = float(voicing_threshold_prob)
        self.scaled = bool(scaled)
        self.single_side_peak_width = 5
        if self.scaled:
            assert self.ini_probs.min() > 0.3 / (self.num_freq_bins * 10)       # dcnet/softmax_viterbi.py:2536
        self._prior_dev = torch.from_numpy(np.ascontiguousarray(self.ini_probs, np.float32)).to(self._decoder.device) if self.scaled else None

    def _log_emissions(self, logits, out=None):
        from .emissions import softmax_scaled_log_emissions
        return softmax_scaled_log_emissions(logits, self.voicing_threshold_prob, self._prior_dev, self.single_side_peak_width, out=out, dtype=self._torch_dtype())

    def _obs_params(self):
        vth = np.float32(self.voicing_threshold_prob)       # float32 arithmetic, as softmax_scaled_log_emissions hands it to the kernel
        unvoiced_logit = float(np.log(vth / (np.float32(1) - vth)))
        return ViterbiDecoder.obs_params("softmax_scaled", self.num_freq_bins, self.single_side_peak_width, unvoiced_logit,
                                         prior=self._prior_dev)


# ----------------------------------------------------------------------------- imm's decoder (activations in)
class ImmViterbi:
    """imm's ``Viterbi`` (imm/tf_imm.py:48-135): the dense Durrieu matrix over ``n_bins`` pitch bins plus the unvoiced state,
    a uniform prior, and a front-end that turns NMF source activations ``HF0 [n_bins, T]`` into log-emissions.

    Constructor as in the reference (:51-68): ``log_transition_matrix_T = np.log(A.T)`` with NO ``tiny`` added (the matrix is
    asserted positive), float32 C order; ``log_prob_init`` = the uniform prior logged in float64, then cast to float32.

    * ``process_HF0_fn`` / ``viterbi_librosa_fn`` -- the reference's two steps with its array conventions: the first is host
      NumPy and byte-equal to the reference's, the second decodes on the GPU and is bit-exact.
    * ``__call__(HF0)`` -- the reference's call surface (``int64[T]`` states as NumPy), with the front-end on the GPU as well
      (``vit_obs_activations``): float32 add, the device's ``logf`` (a few ulp from NumPy's; the path can differ from the
      host-exact one only where two paths tie to that precision), the clamp decided exactly as the host decides it.
    * ``decode_activations`` / ``decode_activations_recordings`` -- the same with torch tensors that stay on the GPU, one
      recording or many in one builder launch and one packed decode.

    ``emission_dtype``: storage of the emission tensor the GPU front-end writes, "float32" or "float16" (the float32 value
    rounded to nearest even; the range [-87.4, 89] fits).

    A note on NumPy versions: the reference adds ``np.exp(-87)``, a float64 scalar, in the clamp case.  NumPy 1.x keeps the
    float32 array type there; NumPy >= 2 promotes the sum to float64, and the reference's own ``viterbi_librosa_fn`` then
    rejects the result.  ``process_HF0_fn`` follows whichever NumPy runs, like the reference; the GPU front-end always adds in
    float32 (``clamp_to = float32(exp(-87))``)."""

    def __init__(self, bins_per_semitone, n_bins, device=None, emission_dtype="float32"):
        from .synth import durrieu_transition
        self.b = bins_per_semitone
        self.n_bins = n_bins
        A = durrieu_transition(n_bins=n_bins, bins_per_semitone=bins_per_semitone)
        assert np.all(A > 0)
        t = np.log(A.T)
        assert not np.any(np.isneginf(t))
        self.log_transition_matrix_T = np.require(t, np.float32, ['C'])
        p = np.empty([n_bins + 1])
        p.fill(1. / (n_bins + 1))
        self.log_prob_init = np.log(p).astype(np.float32)
        if emission_dtype not in ("float32", "float16"):
            raise ValueError('emission_dtype must be "float32" or "float16"')
        self.emission_dtype = emission_dtype
        self._device = device
        self._dec = None

    @property
    def _decoder(self) -> ViterbiDecoder:
        """The plan on the GPU, made on first use: the parameters and ``process_HF0_fn`` are host-only."""
        if self._dec is None:
            self._dec = ViterbiDecoder(self.log_transition_matrix_T, self.log_prob_init, self._device)
        return self._dec

    # ---- the reference's two steps
    def process_HF0_fn(self, HF0):
        """Host NumPy, the reference's arithmetic operation by operation (imm/tf_imm.py:70-88): ``[n_bins, T]`` activations ->
        ``[n_bins + 1, T]`` log-emissions, the unvoiced row last."""
        HF0 = _to_numpy(HF0)
        assert isinstance(HF0, np.ndarray)
        assert HF0.shape[0] == self.n_bins
        t = HF0[HF0 > 0].min()                       # (raises on an empty mask, as the reference does)
        if np.log(t) < -87:
            t = np.exp(-87)
        log_HF0 = np.log(HF0 + t)
        return np.pad(log_HF0, [[0, 1], [0, 0]], mode='constant', constant_values=np.min(log_HF0))

    def viterbi_librosa_fn(self, log_HF0):
        """``[n_bins + 1, T]`` float32 log-emissions -> ``int64[T]`` states (imm/tf_imm.py:90-127); bit-exact."""
        S = self.n_bins + 1
        assert isinstance(log_HF0, np.ndarray)
        assert log_HF0.dtype == np.float32
        assert log_HF0.shape[0] == S
        probs = np.require(np.transpose(log_HF0), np.float32, ['C'])
        return _run(self.log_transition_matrix_T, self.log_prob_init, probs, self._decoder)

    # ---- activations in, path out, on the GPU
    def _torch_dtype(self):
        return torch.float16 if self.emission_dtype == "float16" else torch.float32

    def _to_device(self, HF0) -> torch.Tensor:
        x = HF0 if isinstance(HF0, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(_to_numpy(HF0), np.float32))
        x = x.to(device=self._decoder.device, dtype=torch.float32)
        if x.dim() != 2 or x.shape[0] != self.n_bins or x.shape[1] < 1:
            raise ValueError(f"HF0 must be [{self.n_bins}, T] with T >= 1")
        return x if x.stride(1) == 1 and (x.stride(0) >= x.shape[1] or x.shape[0] == 1) else x.contiguous()

    def decode_activations(self, HF0) -> torch.Tensor:
        """``HF0 [n_bins, T]`` (NumPy or torch) -> ``int64[T]`` states as a torch tensor on the decoder's device: the emission
        builder (``emissions.activation_log_emissions``) and the decode, no host visit for GPU-resident activations."""
        from .emissions import activation_log_emissions
        E = activation_log_emissions(self._to_device(HF0), dtype=self._torch_dtype())
        states, _ = self._decoder.decode(E, out_dtype=torch.int64)
        return states

    def decode_activations_recordings(self, hf0_cat, offsets=None, max_workspace_bytes=None):
        """Many recordings in one pass: ``hf0_cat [n_bins, sum T_b]`` holds them side by side along the frame axis, recording b in
        columns ``offsets[b] : offsets[b+1]`` (``offsets``: a host sequence of B + 1 frame offsets from 0).  One emission-builder
        call with per-recording statistics and one packed decode (``vit_decode_packed``; the step-structured plan of the Durrieu
        matrix is served there).  ``hf0_cat`` may also be a list of ``[n_bins, T_b]`` tensors or arrays, which are concatenated
        along frames first -- that is a copy of every recording; callers that can should fill one buffer.  Returns a list of
        ``int64[T_b]`` state tensors on the GPU, each equal to ``decode_activations`` of that recording alone.
        ``max_workspace_bytes``: a budget for the decoder's workspace (``ViterbiDecoder.decode_packed``: the bounded packed decode
        where the full delta history, 2896 bytes per frame at 722 states, does not fit; the same result).  ``None``: the full history."""
        from .emissions import activation_log_emissions
        if isinstance(hf0_cat, (list, tuple)):
            if offsets is not None:
                raise ValueError("offsets come from the list's lengths")
            parts = [self._to_device(x) for x in hf0_cat]
            if not parts:
                return []
            offsets = np.concatenate([[0], np.cumsum([int(x.shape[1]) for x in parts])])
            hf0_cat = torch.cat(parts, dim=1)
        elif offsets is None:
            raise ValueError("offsets are required with a concatenated hf0")
        x = self._to_device(hf0_cat)
        off = np.ascontiguousarray(offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64)
        E = activation_log_emissions(x, offsets=off, dtype=self._torch_dtype())
        states, _ = self._decoder.decode_packed(E, off, out_dtype=torch.int64, max_workspace_bytes=max_workspace_bytes)
        return [states[off[b]:off[b + 1]] for b in range(off.size - 1)]

    def __call__(self, HF0):
        """``viterbi(HF0) -> int64[T]`` states as a NumPy array, the reference's call surface (imm/tf_imm.py:129-135, :692)."""
        return self.decode_activations(HF0).cpu().numpy()


class RecordingAccumulator:
    """Per-recording logits kept on the GPU (replaces tonet/for_paper.py:2282-2309, where every batch of snippets is
    copied to the host, transposed, and the recording concatenated in NumPy before ``viterbi(logits)``).

        acc = RecordingAccumulator(viterbi, max_frames)          # viterbi: Viterbi ("shaun"), SoftMaxViterbi or ScaledSoftMaxViterbi
        for batch in recording: acc.append(pitch_logits, padded_frames)   # [n_snippets, channels, frames] on the GPU
        voiced, bins, notes = acc.finish(note_range)             # torch tensors on the GPU

    ``append`` transposes the snippets into time-major rows directly behind the rows already held (one kernel:
    ``vit_snippets_append``; "shaun" rows are relative to the unvoiced channel, :2296-2297), ``finish`` runs emission
    builder, decoder, voicing map and the bin -> note gather without a host visit.  Channels per snippet: n_bins + 1 with the
    unvoiced channel first for Viterbi (subtracted and dropped) and SoftMaxViterbi (kept); the n_bins pitch channels only for
    ScaledSoftMaxViterbi, whose unvoiced logit is a constant (dcnet/softmax_viterbi.py:2548-2550).

    ``streaming=True`` spends the forward pass beside the acoustic model instead of behind it: ``append`` also builds the emission
    rows of the new frames with the wrapped class's stand-alone builder (the builders work per frame: the rows a whole-recording
    call would build, bit for bit) into a chunk buffer it keeps, and advances a one-recording ``ViterbiDecoder.stream`` by them; ``finish`` is then the
    back-trace, the voicing map and the note gather, with the result of ``streaming=False``.  The default is ``False``, and
    ``logits()`` works in both modes.  ``ring_frames=R`` (with ``streaming=True``) runs the stream as a ring session: R history rows
    whatever ``max_frames`` is; ``partial()`` works as before (call it often enough that R frames never pile up behind the frontier),
    ``finish()`` is the last commit plus the tail behind it and returns what ``streaming=True`` returns.  Only the history is bounded
    by R: the logits rows and the outputs keep ``max_frames``.  The class wraps the three logits decoders only: ``ImmViterbi`` callers stream with
    ``viterbi._decoder.stream(...)`` and ``emissions.activation_log_emissions`` per chunk.

    ``append`` takes float32 or float16 snippets (``vit_snippets_append_f16`` widens exactly; the rows kept are float32 either way), and the
    emission rows of ``finish`` and of the streaming chunk buffer have the wrapped class's ``emission_dtype``: with "float16" the result is
    the decode of the rounded rows (see ``_PreparedViterbi``), the same for ``streaming=False``, ``streaming=True`` and ``ring_frames=``."""

    def __init__(self, viterbi: _PreparedViterbi, max_frames: int, streaming: bool = False, ring_frames: int | None = None):
        self.viterbi = viterbi
        if isinstance(viterbi, Viterbi):
            self.mode, self.channels, self.cols = 0, viterbi.num_freq_bins + 1, viterbi.num_freq_bins
        elif isinstance(viterbi, ScaledSoftMaxViterbi):       # (a SoftMaxViterbi subclass: test it first)
            self.mode, self.channels, self.cols = 1, viterbi.num_freq_bins, viterbi.num_freq_bins
        elif isinstance(viterbi, SoftMaxViterbi):
            self.mode, self.channels, self.cols = 1, viterbi.num_freq_bins + 1, viterbi.num_freq_bins + 1
        else:
            raise TypeError("RecordingAccumulator needs a Viterbi, SoftMaxViterbi or ScaledSoftMaxViterbi")
        dev = viterbi._decoder.device
        self._rows = torch.empty((int(max_frames), self.cols), dtype=torch.float32, device=dev)
        self.n_frames = 0
        self.streaming = bool(streaming)
        if ring_frames is not None and not self.streaming:
            raise ValueError("ring_frames needs streaming=True")
        self._stream = viterbi._decoder.stream(1, int(max_frames), ring_frames=ring_frames) if self.streaming else None
        # (ring) the states committed so far: the ring bounds the history rows only, the outputs keep max_frames
        self._ring_states = torch.empty(int(max_frames), dtype=torch.int32, device=dev) if ring_frames is not None else None
        self._chunk = None                 # (streaming) the emission rows of one append, reused: it grows to the largest append seen
        self._partial = None               # (streaming) partial(): voiced / bins / notes of the committed frames

    def reset(self):
        self.n_frames = 0
        if self._stream is not None:
            self._stream.reset()

    def append(self, pitch_logits: torch.Tensor, padded_frames: int = 0):
        from . import _lib
        if not isinstance(pitch_logits, torch.Tensor) or pitch_logits.device != self._rows.device:
            raise ValueError("pitch_logits must be a torch tensor on the decoder's device")
        if pitch_logits.dtype not in (torch.float32, torch.float16) or pitch_logits.dim() != 3 or pitch_logits.shape[1] != self.channels:
            raise ValueError(f"pitch_logits must be float32 or float16 [snippets, {self.channels}, frames]")
        x = pitch_logits.contiguous()
        n, C, F = x.shape
        rows = n * F - int(padded_frames)
        if rows < 0 or self.n_frames + rows > self._rows.shape[0]:
            raise ValueError("recording longer than max_frames (or padded_frames out of range)")
        # (float16 snippets are widened inside the kernel: the float32 rows of their .float() copy)
        fn = _lib.load().vit_snippets_append_f16 if x.dtype == torch.float16 else _lib.load().vit_snippets_append
        with torch.cuda.device(x.device):
            rc = fn(x.data_ptr(), n, C, F, self.mode, self._rows[self.n_frames:].data_ptr(), rows,
                    torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(rc, "vit_snippets_append")
        if self._stream is not None and rows > 0:      # the new frames' emission rows, then the forward pass over them
            dt = self.viterbi._torch_dtype()             # (read where finish() reads it: the adapter; a session's type is fixed by its first append)
            if self._chunk is not None and self._chunk.dtype != dt:
                raise ValueError("the wrapped decoder's emission_dtype changed while the recording was being accumulated")
            if self._chunk is None or self._chunk.shape[0] < rows:
                self._chunk = torch.empty((rows, self.viterbi.num_freq_bins + 1), dtype=dt, device=self._rows.device)
            self._stream.append(self.viterbi._log_emissions(self._rows[self.n_frames:self.n_frames + rows], out=self._chunk[:rows]))
        self.n_frames += rows

    def logits(self) -> torch.Tensor:
        """The recording so far: ``[n_frames, columns]`` on the GPU (a view)."""
        return self._rows[: self.n_frames]

    def partial(self, note_range=None, max_lookback=None):
        """``(n_final, voiced, bins, notes)`` of frames ``[0, n_final)``: the part of the recording whose path no later frame can
        change (``DecodeStream.commit``), a prefix of what ``finish`` will return.  ``streaming=True`` only.  The voicing map and the
        note gather run over the states committed by this call only; earlier ones are kept.  ``notes`` is None without a
        ``note_range`` (pass the same one every time).  Synchronises, like ``DecodeStream.commit``."""
        if self._stream is None:
            raise ValueError("partial() needs streaming=True")
        dec, dev, cap = self.viterbi._decoder, self._rows.device, self._rows.shape[0]
        if self._partial is None:
            self._partial = (torch.empty(cap, dtype=torch.bool, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
                             torch.empty(cap, dtype=torch.float32, device=dev))
        voiced, bins, notes = self._partial
        if self._ring_states is not None:
            first, lens, fresh = self._stream.commit(max_lookback=max_lookback, out_dtype=torch.int32)
            self._ring_states[int(first[0]):int(lens[0])] = fresh[0]
        else:
            lens, fresh = self._stream.commit(max_lookback=max_lookback, out_dtype=torch.int32)
        n_final, k = int(lens[0]), int(fresh[0].numel())
        if k > 0:
            nb = self.viterbi.num_freq_bins
            out = dec.voicing(fresh[0], nb) if note_range is None else dec.voicing_notes(fresh[0], note_range, nb)
            voiced[n_final - k:n_final], bins[n_final - k:n_final] = out[0], out[1]
            if note_range is not None:
                notes[n_final - k:n_final] = out[2]
        return n_final, voiced[:n_final], bins[:n_final], (notes[:n_final] if note_range is not None else None)

    def finish(self, note_range=None):
        if self._stream is not None:
            dec = self.viterbi._decoder
            if self._ring_states is not None:      # the last commit, then the frames behind the frontier
                first, lens, fresh = self._stream.commit(out_dtype=torch.int32)
                self._ring_states[int(first[0]):int(lens[0])] = fresh[0]
                f, tail, _ = self._stream.tail(out_dtype=torch.int32)
                self._ring_states[int(f[0]):self.n_frames] = tail[0]
                states = self._ring_states[None, :self.n_frames]
            else:
                states, _ = self._stream.decode(out_dtype=torch.int32)
            out = dec.voicing(states[0], self.viterbi.num_freq_bins) if note_range is None else dec.voicing_notes(states[0], note_range, self.viterbi.num_freq_bins)
        else:
            out = self.viterbi.decode_logits(self.logits(), note_range)
        self.reset()
        return out
