"""Song lengths outside [1, T]: include/viterbi_hip.h promises that song b uses clamp(lengths[b], 1, T) frames.

Every kernel and device-side driver takes a song's length through song_length (csrc/device_common.hpp), which clamps in 64 bits
before it narrows to int; the raw reads of a lengths array that remain (the skip_nonpositive tests of the back-trace kernels) read
the library's own segment tables, and the Python wrappers hand the tensor on without host arithmetic -- confirmed by reading before
this file first ran.  The lengths below tell the wrong orders apart: a truncation to int before the clamp turns 2^32 + 3 into 3
and 2^31 + 5 into a negative number, a missing lower clamp leaves 0, -1, -2^62 and INT64_MIN, a missing upper clamp reads past the
song at T + 1, 2^40 and INT64_MAX.

T = 70, twelve songs.  The reference runs with np.clip(lengths, 1, T): states, the -1 fill past each length and the log-likelihood
bits must equal it on every entry point that takes a lengths tensor."""
import math

import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests import f64_ref
from viterbi_spl_amd import ViterbiDecoder, _lib, synth
from viterbi_spl_amd import emissions as em

pytestmark = pytest.mark.gpu

T = 70
K = 64
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
LENGTHS = np.asarray([0, -1, -2 ** 62, INT64_MIN, T, T + 1, 2 ** 31 + 5, 2 ** 32 + 3, 2 ** 40, INT64_MAX, 1, 37], np.int64)
CLAMPED = np.clip(LENGTHS, 1, T)
B = len(LENGTHS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def test_the_lengths_tell_the_wrong_orders_apart():
    assert CLAMPED.tolist() == [1, 1, 1, 1, T, T, T, T, T, T, 1, 37]
    as_int = LENGTHS.astype(np.int32)                       # what a narrowing before the clamp would see
    assert as_int[7] == 3 and as_int[6] < 0 and as_int[8] == 0 and as_int[9] == -1 and as_int[2] == 0 and as_int[3] == 0
    assert not np.array_equal(np.clip(as_int, 1, T), CLAMPED)


def _bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x, np.float32)
    return x.view(np.uint32)


def _params(golden, name):
    return golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]


def _batch(golden, dev, name, kind, f16=False):
    """decoder, emissions [B, T, S] on the device, the lengths tensor, and the oracle's answer for the clamped lengths."""
    from tests.common import GEN
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    E = GEN[kind](B, T, dec.S, seed=len(name) + T, device=dev, dtype=torch.float16 if f16 else torch.float32)
    ref_s, ref_l = vo.decode_c(A, pi, E.float().cpu().numpy(), lengths=CLAMPED)
    for b in range(B):
        assert np.all(ref_s[b, CLAMPED[b]:] == -1) and np.all(ref_s[b, :CLAMPED[b]] >= 0)
    return dec, E, torch.from_numpy(LENGTHS).to(dev), ref_s, ref_l


def check(got, ref_s, ref_l, what):
    st, ll = got
    st = st.cpu().numpy()
    for b in range(B):
        n = int(CLAMPED[b])
        assert np.array_equal(st[b, :n], ref_s[b, :n]), (what, "states of song", b, int(LENGTHS[b]))
        assert np.all(st[b, n:] == -1), (what, "fill past the length of song", b, int(LENGTHS[b]), st[b, n:n + 4])
    assert np.array_equal(_bits(ll), _bits(ref_l)), (what, "log-likelihood bits", ll.cpu().numpy(), ref_l)


def _algos(dec):
    if dec.info["banded_ok"]:
        return ("auto", "dense", "group", "wave") if dec.info["wave_ok"] else ("auto", "dense", "banded")
    return ("auto", "dense")


@pytest.mark.parametrize("name,kind,f16", [("tonet361", "peaks", False), ("tonet361", "dense", True), ("durrieu722", "dense", False),
                                            ("durrieu722", "ties", True), ("dense97", "ties", False)])
def test_decode(golden, dev, name, kind, f16):
    """vit_decode with every algo of the plan: wave, workgroup and dense kernels of the 361-state band, the step kernels (both
    forms) and the dense kernel of the Durrieu matrix, the matrix-resident dense kernel at 97 states, with every back-trace form the
    plan has."""
    dec, E, lens, ref_s, ref_l = _batch(golden, dev, name, kind, f16)
    assert dec.info["step_ok"] == (name == "durrieu722") and dec.info["wave_ok"] == (name == "tonet361")
    try:
        for algo in _algos(dec):
            for btf in ((0, 1, 2) if dec.info["banded_ok"] else (0,)):
                for form in ((0, 3) if dec.info["step_ok"] and algo == "auto" else (0,)):
                    dec.set_option("backtrace_form", btf)
                    dec.set_option("step_form", form)
                    check(dec.decode(E, lengths=lens, algo=algo, out_dtype=torch.int32), ref_s, ref_l, (name, algo, btf, form))
    finally:
        dec.set_option("reset", 0)


@pytest.mark.parametrize("name,kind", [("tonet361", "peaks"), ("durrieu722", "dense")])
def test_decode_checkpointed(golden, dev, name, kind):
    """Segments of 64 frames: pass 1, segment_prep_kernel and the segment back-traces all take the clamped length."""
    dec, E, lens, ref_s, ref_l = _batch(golden, dev, name, kind)
    check(dec.decode_checkpointed(E, segment_frames=K, lengths=lens, out_dtype=torch.int32), ref_s, ref_l, (name, "decode_checkpointed"))


def test_forward_and_backtrace_phases_with_the_half_history(golden, dev):
    """vit_forward then vit_backtrace_checked with the lengths tensor in both, the wave form keeping even rows only."""
    dec, E, lens, ref_s, ref_l = _batch(golden, dev, "tonet361", "dense")
    try:
        dec.set_option("wave_history", 2)
        assert dec.history_mode(B, T, "wave") == "half"
        st = torch.full((B, T), 12345, dtype=torch.int32, device=dev)
        ll = torch.empty((B,), dtype=torch.float32, device=dev)
        dec.decode_into(E, st, ll, lengths=lens, algo="wave", phase="forward")
        dec.decode_into(E, st, None, lengths=lens, algo="wave", phase="backtrace")
        torch.cuda.synchronize()
        check((st, ll), ref_s, ref_l, "forward + backtrace, half history")
    finally:
        dec.set_option("reset", 0)


def test_decode_f64(golden, dev):
    """decode_f64 and decode_f64_checkpointed against the NumPy restatement of the float64 variant (tests/f64_ref.py)."""
    A, pi = _params(golden, "tonet361")
    dec = ViterbiDecoder(A, pi, dev)
    E = synth.emissions_dense(B, T, dec.S, seed=64, device=dev)
    ref_s, ref_l = f64_ref.decode_f64_batch(A, pi, E.cpu().numpy(), CLAMPED)
    lens = torch.from_numpy(LENGTHS).to(dev)
    for what, run in (("decode_f64", lambda: dec.decode_f64(E, lengths=lens)),
                      ("decode_f64_checkpointed", lambda: dec.decode_f64_checkpointed(E, segment_frames=K, lengths=lens))):
        st, ll = run()
        torch.cuda.synchronize()
        st, ll = st.cpu().numpy(), ll.cpu().numpy()
        assert np.array_equal(st, ref_s), (what, np.argwhere(st != ref_s)[:6].tolist())
        assert np.array_equal(f64_ref.bits64(ll), f64_ref.bits64(ref_l)), (what, ll, ref_l)


def test_decode_logits(golden, dev):
    """decode_logits and decode_logits_checkpointed against the stand-alone builder followed by decode of the clamped lengths, and
    that against the oracle on the builder's rows."""
    A, pi = _params(golden, "tonet361")
    dec = ViterbiDecoder(A, pi, dev)
    X = synth.pitch_logits(B, T, 360, seed=3, device=dev)
    obs = ViterbiDecoder.obs_params("shaun", 360, 5, math.log(0.32 / 0.68), math.log(0.8 / 0.2), 2.0)
    Eb = em.shaun_log_emissions(X, 0.32, 5)
    clamped = torch.from_numpy(CLAMPED).to(dev)
    want_s, want_l = dec.decode(Eb, lengths=clamped, algo="wave", out_dtype=torch.int32)
    ref_s, ref_l = vo.decode_c(A, pi, Eb.cpu().numpy(), lengths=CLAMPED)
    check((want_s, want_l), ref_s, ref_l, "builder + decode")
    lens = torch.from_numpy(LENGTHS).to(dev)
    for what, run in (("decode_logits", lambda: dec.decode_logits(X, obs, lengths=lens, out_dtype=torch.int32)),
                      ("decode_logits_checkpointed", lambda: dec.decode_logits_checkpointed(X, obs, segment_frames=K, lengths=lens, out_dtype=torch.int32))):
        st, ll = run()
        torch.cuda.synchronize()
        assert torch.equal(st, want_s), what
        assert torch.equal(ll.view(torch.int32), want_l.view(torch.int32)), what
        check((st, ll), ref_s, ref_l, what)
