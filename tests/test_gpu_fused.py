"""GPU tests of the fused logits -> path decode (``vit_decode_logits``, csrc/fused.hip): emission builder and wave-form forward
recursion in one workgroup, the emission rows handed over through LDS.  Every comparison is exact: states and log-likelihoods
against the two-step path (``vit_obs_*`` into a buffer, then ``decode(algo="wave")``), the optional emission output against the
stand-alone builder byte for byte, and the CPU oracle (``oracle.viterbi_oracle.decode_c``) on the stand-alone builder's rows as the
reference for sampled songs."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests.common import logits_case, range_edge_logits
from viterbi_spl_amd import ViterbiDecoder, _lib, synth
from viterbi_spl_amd import emissions as em
from viterbi_spl_amd import reference_api as ra

pytestmark = pytest.mark.gpu

VIT_EINVAL, VIT_EWORKSPACE, VIT_EUNSUPPORTED = -1, -4, -5
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
VTH2 = 0.32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _decoder(golden, name, dev):
    return ViterbiDecoder(golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"], dev)


def _unvoiced_logit(vth):
    v = np.float32(vth)
    return float(np.log(v / (np.float32(1) - v)))


def _builder(mode, n_bins, prior=None, vth=VTH2):
    """(obs parameters of decode_logits, the stand-alone builder of emissions.py with the same arguments)."""
    import math
    if mode == 0:
        obs = ViterbiDecoder.obs_params("shaun", n_bins, 5, math.log(0.32 / (1.0 - 0.32)), math.log(0.8 / (1.0 - 0.8)), 2.0)
        return obs, lambda x: em.shaun_log_emissions(x, 0.32, 5)
    if mode == 1:
        return ViterbiDecoder.obs_params("softmax", n_bins, 15), lambda x: em.softmax_log_emissions(x, 15)
    obs = ViterbiDecoder.obs_params("softmax_scaled", n_bins, 5, _unvoiced_logit(vth), prior=prior)
    return obs, lambda x: em.softmax_scaled_log_emissions(x, vth, prior, 5)


def _rows(mode, n_bins, n, seed):
    """n logit rows: tests/common.logits_case, with the float32 range-edge rows of range_edge_logits spliced in at the front."""
    cols = n_bins + 1 if mode == 1 else n_bins
    x = logits_case(seed, n, cols)
    edge = range_edge_logits(n_bins, 15 if mode == 1 else 5, unvoiced_column=mode == 1)
    k = min(len(edge), n // 2)
    x[:k] = edge[:k]
    return x


def _lengths(B, T, dev):
    """Lengths that include 1, T, and values inside a phase of the hand-off ring."""
    opts = [T, 1, max(1, T - 1), max(1, T // 2 + 1), max(1, T - 3), min(T, 6), T, min(T, 2), max(1, T - 5)]
    return torch.tensor([opts[b % len(opts)] for b in range(B)], dtype=torch.int64, device=dev)


def _check_case(dec, A, pi, mode, prior, B, T, seed, dev, lengths_on):
    n_bins = dec.S - 1
    obs, build = _builder(mode, n_bins, prior)
    x = torch.from_numpy(_rows(mode, n_bins, B * T, seed)).to(dev).view(B, T, -1).contiguous()
    lengths = _lengths(B, T, dev) if lengths_on else None
    E = build(x)                                                        # the vit_obs_* tensor
    want_s, want_l = dec.decode(E, lengths=lengths, algo="wave", out_dtype=torch.int32)
    eo = torch.full((B, T, dec.S), 7.0, dtype=torch.float32, device=dev)
    got_s, got_l = dec.decode_logits(x, obs, lengths=lengths, out_dtype=torch.int32, emissions_out=eo)
    torch.cuda.synchronize()
    what = f"mode {mode} B {B} T {T} lengths {lengths_on}"
    assert torch.equal(got_s, want_s), f"{what}: states differ from vit_obs + decode(wave)"
    assert torch.equal(got_l.view(torch.int32), want_l.view(torch.int32)), f"{what}: log-likelihood bits differ"
    ln = lengths.cpu().numpy() if lengths_on else np.full(B, T)
    Eh, eoh, sh = E.cpu().numpy(), eo.cpu().numpy(), got_s.cpu().numpy()
    for b in range(B):
        assert np.array_equal(eoh[b, :ln[b]].view(np.uint32), Eh[b, :ln[b]].view(np.uint32)), f"{what}: emissions_out of song {b} differs"
        assert (sh[b, ln[b]:] == -1).all(), f"{what}: states past the length of song {b}"
        assert (sh[b, :ln[b]] >= 0).all()
    # a second call: identical bytes (no state left in the ring, the workspace or the plan)
    again_s, again_l = dec.decode_logits(x, obs, lengths=lengths, out_dtype=torch.int32)
    assert torch.equal(again_s, got_s) and torch.equal(again_l.view(torch.int32), got_l.view(torch.int32)), f"{what}: second call differs"
    # the CPU oracle on the stand-alone builder's rows, three songs
    for b in sorted({0, B // 2, B - 1}):
        ref_s, ref_l = vo.decode_c(A, pi, Eh[b, :ln[b]])
        assert np.array_equal(sh[b, :ln[b]], ref_s), f"{what}: song {b} differs from the oracle"
        assert np.float32(got_l[b].item()).tobytes() == np.float32(ref_l).tobytes(), f"{what}: log-likelihood of song {b} differs from the oracle"


CASES = [("tonet361", 0, False), ("tonet361", 1, False), ("msnet321", 2, False), ("msnet321", 2, True)]


@pytest.mark.parametrize("name,mode,with_prior", CASES)
def test_small_every_builder(golden, dev, name, mode, with_prior):
    """Every builder; B around the four songs of a workgroup, T around the phase length of the ring; with and without lengths."""
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    prior = torch.from_numpy(np.ascontiguousarray(golden["params"]["msnet321_pi"], np.float32)).to(dev) if with_prior else None
    seed = 100 * mode + (50 if with_prior else 0)
    for B in (1, 3, 4, 5, 9):
        for T in (1, 2, 3, 4, 5, 7, 8, 9, 257):
            seed += 1
            _check_case(dec, A, pi, mode, prior, B, T, seed, dev, lengths_on=False)
            _check_case(dec, A, pi, mode, prior, B, T, seed + 1000, dev, lengths_on=True)


def test_wave_uniform_forms(golden, dev):
    """The recursion's last-state form ("wave_uniform" 2) and the three-group form on the 361-state grid (3) decode the same bits."""
    A, pi = golden["params"]["tonet361_logA_T"], golden["params"]["tonet361_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    for opt in (2, 3):
        dec.set_option("wave_uniform", opt)
        _check_case(dec, A, pi, 0, None, 5, 41, 900 + opt, dev, lengths_on=True)
    dec.set_option("reset", 0)


def test_builder_goldens(golden, dev):
    """The cases of tests/golden/obs_goldens.npz: the fused kernel's emission output equals the stand-alone builder's bit for bit,
    so it inherits that builder's recorded 1e-5 bar (tests/test_gpu_parity.py::test_emission_builders_on_gpu)."""
    og = np.load(os.path.join(GOLDEN, "obs_goldens.npz"))
    d361, d321 = _decoder(golden, "tonet361", dev), _decoder(golden, "msnet321", dev)
    prior = torch.from_numpy(np.ascontiguousarray(golden["params"]["msnet321_pi"], np.float32)).to(dev)

    def check(dec, obs, build, x, what):
        x = torch.from_numpy(x).to(dev)
        want = build(x)
        eo = torch.zeros_like(want)
        dec.decode_logits(x, obs, emissions_out=eo)
        torch.cuda.synchronize()
        assert torch.equal(eo.view(torch.int32), want.view(torch.int32)), what

    for k in range(3):
        seed, n = og[f"shaun{k}_seed"]
        obs, build = _builder(0, 360)
        check(d361, obs, build, logits_case(int(seed), int(n), 360), f"shaun{k}")
        seed, n = og[f"softmax{k}_seed"]
        obs, build = _builder(1, 360)
        check(d361, obs, build, logits_case(int(seed), int(n), 361), f"softmax{k}")
    for k in range(4):
        seed, n = og[f"scaled{k}_seed"]
        vth, scaled = float(og[f"scaled{k}_vth"][0]), bool(og[f"scaled{k}_vth"][1])
        obs, build = _builder(2, 320, prior if scaled else None, vth)
        check(d321, obs, build, logits_case(int(seed), int(n), 320), f"scaled{k}")


@pytest.mark.parametrize("voicing", ["toggle", "segments"])
def test_full_size(golden, dev, voicing):
    """[1024, 30000, 360] "shaun" logits, songs repeating with period 32 (bench.py's pipeline block); all songs full length, then
    lengths ragged down to 1.  Fused == unfused on every song (the unfused path in slices of 256 songs: its emission tensor is
    11 GB a slice), repeated songs decode identically wherever they sit, the oracle on three sampled songs."""
    B, T, P = 1024, 30000, 32
    A, pi = golden["params"]["tonet361_logA_T"], golden["params"]["tonet361_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    obs, build = _builder(0, 360)
    X = synth.pitch_logits(P, T, 360, seed=5, device=dev, voicing=voicing).repeat(B // P, 1, 1).contiguous()
    rng = np.random.default_rng(7)
    ragged = rng.integers(1, T + 1, B)
    ragged[:8] = (1, T, 2, T - 1, 4, 5, T - 3, 9)
    for lengths_np in (None, ragged):
        lengths = torch.from_numpy(lengths_np.astype(np.int64)).to(dev) if lengths_np is not None else None
        ws = torch.empty(dec.workspace_bytes_logits(obs, B, T) + 256, dtype=torch.uint8, device=dev)
        got_s, got_l = dec.decode_logits(X, obs, lengths=lengths, out_dtype=torch.int32, workspace=ws)
        torch.cuda.synchronize()
        del ws
        torch.cuda.empty_cache()
        for s0 in range(0, B, 256):
            E = build(X[s0:s0 + 256])
            want_s, want_l = dec.decode(E, lengths=lengths[s0:s0 + 256] if lengths is not None else None, algo="wave", out_dtype=torch.int32)
            assert torch.equal(got_s[s0:s0 + 256], want_s), f"{voicing}: states of songs {s0}.. differ"
            assert torch.equal(got_l[s0:s0 + 256].view(torch.int32), want_l.view(torch.int32)), f"{voicing}: log-likelihoods of songs {s0}.. differ"
            if s0 == 0:
                for b in (0, 17, 31):
                    n = T if lengths_np is None else int(lengths_np[b])
                    ref_s, ref_l = vo.decode_c(A, pi, E[b, :n].cpu().numpy())
                    assert np.array_equal(got_s[b, :n].cpu().numpy(), ref_s), f"{voicing}: song {b} differs from the oracle"
                    assert np.float32(got_l[b].item()).tobytes() == np.float32(ref_l).tobytes()
            del E, want_s, want_l
        dec._ws = None
        torch.cuda.empty_cache()
        if lengths_np is None:          # the same song wherever it sits in the batch
            ref = got_s[:P]
            for r in range(1, B // P):
                assert torch.equal(got_s[r * P:(r + 1) * P], ref), f"{voicing}: repeat {r} decodes differently"
                assert torch.equal(got_l[r * P:(r + 1) * P].view(torch.int32), got_l[:P].view(torch.int32))
        else:
            assert (got_s[0, 1:] == -1).all() and (got_s[0, 0] >= 0)
        del got_s, got_l


def test_refusals(golden, dev):
    """A dense plan and the 722-state jdc band are refused before anything is enqueued; wave_history 2 is ignored (same bits); a
    workspace that is too small and n_bins + 1 != S are loud errors."""
    lib = _lib.load()
    obs, build = _builder(0, 360)
    for name, S in (("dense361", 361), ("jdc722", 722)):
        dec = _decoder(golden, name, dev)
        o = ViterbiDecoder.obs_params("shaun", S - 1, 5, -0.75, 1.386, 2.0)
        assert dec.workspace_bytes_logits(o, 4, 16) == 0
        with pytest.raises(_lib.ViterbiHipError):
            dec.decode_logits(torch.zeros((4, 16, S - 1), device=dev), o)
        # through the C ABI: VIT_EUNSUPPORTED, and the outputs are untouched
        st = torch.full((4, 16), 12345, dtype=torch.int32, device=dev)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        x = torch.zeros((4, 16, S - 1), device=dev)
        op = dec._obs_struct(o)
        rc = lib.vit_decode_logits(dec._plan, x.data_ptr(), ctypes.byref(op), 4, 16, None, (ws.data_ptr() + 255) & ~255, ws.numel() - 256, None,
                                   st.data_ptr(), None, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        assert rc == VIT_EUNSUPPORTED and (st == 12345).all()
    A, pi = golden["params"]["tonet361_logA_T"], golden["params"]["tonet361_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    x = torch.from_numpy(logits_case(3, 4 * 50, 360)).to(dev).view(4, 50, 360)
    want_s, want_l = dec.decode_logits(x, obs, out_dtype=torch.int32)
    dec.set_option("wave_history", 2)
    half_s, half_l = dec.decode_logits(x, obs, out_dtype=torch.int32)
    dec.set_option("reset", 0)
    assert torch.equal(half_s, want_s) and torch.equal(half_l.view(torch.int32), want_l.view(torch.int32))
    need = dec.workspace_bytes_logits(obs, 4, 50)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    st = torch.full((4, 50), 12345, dtype=torch.int32, device=dev)
    op = dec._obs_struct(obs)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.vit_decode_logits(dec._plan, x.data_ptr(), ctypes.byref(op), 4, 50, None, (ws.data_ptr() + 255) & ~255, need - 256, None, st.data_ptr(), None, stream)
    assert rc == VIT_EWORKSPACE
    bad = dec._obs_struct(ViterbiDecoder.obs_params("shaun", 320, 5, -0.75, 1.386, 2.0))
    rc = lib.vit_decode_logits(dec._plan, x.data_ptr(), ctypes.byref(bad), 4, 50, None, (ws.data_ptr() + 255) & ~255, need, None, st.data_ptr(), None, stream)
    assert rc == VIT_EINVAL
    torch.cuda.synchronize()
    assert (st == 12345).all(), "a refused call wrote states"
    with pytest.raises(ValueError):
        dec.decode_logits(x, obs, workspace=torch.empty(need, dtype=torch.uint8, device=dev))


def test_reference_api_surface(golden, dev):
    """decode_logits_batch(fused=True) == decode_logits_batch(fused=False) == decode_logits row by row, for the three classes."""
    p = golden["params"]
    A361, pi361 = synth.tonet_transition(360, 14), synth.floored_prior(361)      # the probabilities behind the tonet361 golden parameters
    note_range = np.linspace(30.0, 90.0, 360).astype(np.float32)
    B, T = 5, 67
    lengths = torch.tensor([67, 1, 30, 66, 5], dtype=torch.int64, device=dev)
    objs = [
        (ra.Viterbi(A361, pi361, device=dev), 360, note_range),
        (ra.SoftMaxViterbi(A361, pi361, device=dev), 361, None),
        (ra.ScaledSoftMaxViterbi(p["msnet321_A"], p["msnet321_pi"], 0.4, True, device=dev), 320, None),
        (ra.ScaledSoftMaxViterbi(p["msnet321_A"], p["msnet321_pi"], 0.4, False, device=dev), 320, np.linspace(30.0, 90.0, 320).astype(np.float32)),
    ]
    for v, cols, nr in objs:
        x = torch.from_numpy(logits_case(cols, B * T, cols)).to(dev).view(B, T, cols).contiguous()
        for ln in (None, lengths):
            fused = v.decode_logits_batch(x, lengths=ln, note_range=nr, fused=True)
            plain = v.decode_logits_batch(x, lengths=ln, note_range=nr, fused=False)
            assert len(fused) == len(plain) == (3 if nr is not None else 2)
            for f, q in zip(fused, plain):
                assert torch.equal(f, q), type(v).__name__
            for b in range(B):
                n = T if ln is None else int(ln[b])
                row = v.decode_logits(x[b, :n], nr)
                for f, q in zip(fused, row):
                    assert torch.equal(f[b, :n], q), (type(v).__name__, b)
    # a grid without the wave form: fused=True is a loud error, fused=False decodes
    dur = ra.ScaledSoftMaxViterbi(np.exp(p["jdc722_logA_T"].T.astype(np.float64)) / np.exp(p["jdc722_logA_T"].T.astype(np.float64)).sum(axis=1, keepdims=True),
                                  np.exp(p["jdc722_log_pi"].astype(np.float64)) / np.exp(p["jdc722_log_pi"].astype(np.float64)).sum(), 0.4, False, device=dev)
    x = torch.from_numpy(logits_case(1, 2 * 20, 721)).to(dev).view(2, 20, 721).contiguous()
    with pytest.raises(_lib.ViterbiHipError):
        dur.decode_logits_batch(x, fused=True)
    assert dur.decode_logits_batch(x, fused=False)[0].shape == (2, 20)
