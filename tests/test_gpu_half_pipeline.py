"""GPU tests of the post-processors with float16 emission rows (``Viterbi`` / ``SoftMaxViterbi`` / ``ScaledSoftMaxViterbi(...,
emission_dtype="float16")``, ``RecordingAccumulator`` over them): logits -> float16 emissions (vit_obs_build) -> decode -> voicing map.

Float16 rows are a different decoder input, so the expected result is the ORACLE's decode (oracle.viterbi_oracle.decode_c) of the
adapter's own float16 rows widened to float32, mapped through the voicing rule -- exactly, for every public way to the decode.  The
rows themselves are pinned to the float32 builder by tests/test_gpu_builders_half.py."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests.common import logits_case
from viterbi_spl_amd import _lib, synth
from viterbi_spl_amd import reference_api as ra

pytestmark = pytest.mark.gpu

B, T = 3, 300
LENS = (300, 1, 157)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _adapter(golden, name, dev, **kw):
    """(adapter, logit columns): the three post-processors on the parameters the issue names."""
    p = golden["params"]
    if name == "Viterbi":
        return ra.Viterbi(synth.tonet_transition(360, 14), synth.floored_prior(361), device=dev, **kw), 360
    if name == "SoftMaxViterbi":
        # the golden jdc722 parameters are stored logged and transposed: exp in float64 (log(tiny) entries are the zeros) gives
        # probabilities whose float64 log(p + tiny) rounds back to the stored float32 values
        L = p["jdc722_logA_T"].T
        A = np.where(L <= np.float32(np.log(np.float64(np.finfo(np.float32).tiny))), 0.0, np.exp(L.astype(np.float64)))
        pi = np.exp(p["jdc722_log_pi"].astype(np.float64))
        v = ra.SoftMaxViterbi(A, pi, device=dev, **kw)
        assert v.log_transition_matrix_T.tobytes() == p["jdc722_logA_T"].tobytes() and v.log_ini_probs.tobytes() == p["jdc722_log_pi"].tobytes()
        return v, 722
    return ra.ScaledSoftMaxViterbi(p["msnet321_A"], p["msnet321_pi"], 0.4, True, device=dev, **kw), 320


def _voicing(states, n_bins):
    """The voicing rule on oracle states (-1 past a recording's end stays voiced False, bin -1)."""
    s = torch.as_tensor(np.asarray(states, np.int32))
    voiced = (s >= 0) & (s < n_bins)
    bins = torch.where(s < 0, torch.full_like(s, -1), torch.clamp(s, max=n_bins - 1))
    return voiced, bins


def _same(got, want, what):
    assert got[0].dtype == torch.bool and got[1].dtype == torch.int32, what
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]), what


@pytest.mark.parametrize("name", ["Viterbi", "SoftMaxViterbi", "ScaledSoftMaxViterbi"])
def test_adapters_decode_the_float16_rows(golden, dev, name):
    """B = 3, T = 300, lengths (300, 1, 157).  decode_logits, decode_logits_batch and decode_recordings (each with and without
    max_workspace_bytes) return the oracle's decode of E16.float(), E16 the adapter's own float16 rows; float16 logits give the result
    of their widened copy; fused=True raises ValueError; a default-constructed adapter is float32 and returns what the float32
    builder + decode return."""
    vit, cols = _adapter(golden, name, dev, emission_dtype="float16")
    assert vit.emission_dtype == "float16"
    dec, nb = vit._decoder, vit.num_freq_bins
    x = logits_case(40 + cols, B * T, cols).reshape(B, T, cols)
    xd = torch.from_numpy(x).to(dev)
    lens = np.asarray(LENS, np.int64)
    lens_d = torch.from_numpy(lens).to(dev)
    E16 = vit._log_emissions(xd)
    assert E16.dtype == torch.float16 and tuple(E16.shape) == (B, T, nb + 1)
    ref_s, _ = vo.decode_c(vit.log_transition_matrix_T, vit.log_ini_probs, E16.float().cpu().numpy(), lengths=lens)
    ref_s = np.array(ref_s, np.int32)
    for b in range(B):
        ref_s[b, lens[b]:] = -1
    want = _voicing(ref_s, nb)

    # one recording at a time
    for b in range(B):
        got = vit.decode_logits(xd[b, :lens[b]])
        _same(got, (want[0][b, :lens[b]], want[1][b, :lens[b]]), f"decode_logits recording {b}")
    # the batch, full history and under a budget that the full history misses by one byte
    _same(vit.decode_logits_batch(xd, lengths=lens_d), want, "decode_logits_batch")
    full = dec.plan_workspace(B, T)["workspace_bytes"]
    assert dec.plan_workspace(B, T, max_workspace_bytes=full - 1)["mode"] != "full"
    _same(vit.decode_logits_batch(xd, lengths=lens_d, max_workspace_bytes=full - 1), want, "decode_logits_batch under a budget")
    # the recordings packed
    recs = [xd[b, :lens[b]] for b in range(B)]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    plan = dec.plan_workspace_packed if dec.info["wave_ok"] else dec.plan_workspace_packed_bounded
    full_p = plan(off)["workspace_bytes"]
    assert plan(off, full_p - 1)["mode"] == "checkpointed"
    for budget in (None, full_p - 1):
        got = vit.decode_recordings(recs, max_workspace_bytes=budget)
        assert len(got) == B
        for b in range(B):
            _same(got[b], (want[0][b, :lens[b]], want[1][b, :lens[b]]), f"decode_recordings budget {budget} recording {b}")

    # float16 logits: the result of their widened float32 copy, and no float32 copy is made on the way
    x16 = xd.half()
    assert vit._log_emissions(x16).dtype == torch.float16
    assert torch.equal(vit._log_emissions(x16).view(torch.int16), vit._log_emissions(x16.float()).view(torch.int16))
    a, b_ = vit.decode_logits_batch(x16, lengths=lens_d), vit.decode_logits_batch(x16.float(), lengths=lens_d)
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])
    a, b_ = vit.decode_recordings([r.half() for r in recs]), vit.decode_recordings([r.half().float() for r in recs])
    assert all(torch.equal(u[0], v[0]) and torch.equal(u[1], v[1]) for u, v in zip(a, b_))
    a, b_ = vit.decode_logits(x16[0]), vit.decode_logits(x16[0].float())
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])

    # the fused kernels are float32 only
    for arg in (xd, x16):
        with pytest.raises(ValueError):
            vit.decode_logits_batch(arg, lengths=lens_d, fused=True)

    # the default: float32 rows, today's result; float16 logits are refused by its fused path as well
    v32, _ = _adapter(golden, name, dev)
    assert v32.emission_dtype == "float32"
    E32 = v32._log_emissions(xd)
    assert E32.dtype == torch.float32
    assert torch.equal(E32.half().view(torch.int16), E16.view(torch.int16))
    st32, _ = v32._decoder.decode(E32, lengths=lens_d, out_dtype=torch.int32)
    w32 = v32._decoder.voicing(st32, nb)
    got32 = v32.decode_logits_batch(xd, lengths=lens_d)
    assert torch.equal(got32[0], w32[0]) and torch.equal(got32[1], w32[1])
    with pytest.raises(ValueError):
        v32.decode_logits_batch(x16, lengths=lens_d, fused=True)
    with pytest.raises(ValueError):
        _adapter(golden, name, dev, emission_dtype="bfloat16")


def test_accumulator_float16(dev):
    """Three recordings of 768 frames as float16 snippets of 32 frames (appends of 96 frames), the wrapped Viterbi with
    emission_dtype="float16": streaming=False, streaming=True and ring_frames=256 return identical finish() results, every partial()
    of the two streaming accumulators is the same prefix of it, and the result is the adapter's decode_logits of the float32 rows held
    (the widened snippets, relative to the unvoiced channel)."""
    U, N = 360, 768
    vit = ra.Viterbi(synth.tonet_transition(U, 14), synth.floored_prior(U + 1), device=dev, emission_dtype="float16")
    note_range = torch.linspace(30.0, 90.0, U, device=dev)
    plain = ra.RecordingAccumulator(vit, N)
    lin = ra.RecordingAccumulator(vit, N, streaming=True)
    ring = ra.RecordingAccumulator(vit, N, streaming=True, ring_frames=256)
    for rec in range(3):
        X = synth.pitch_logits(1, N, U, seed=11 + rec, device=dev)[0]
        snips = torch.cat([torch.zeros((N, 1), device=dev), X], dim=1).view(N // 32, 32, U + 1).permute(0, 2, 1).contiguous().half()
        parts = []
        for k in range(N // 96):
            x = snips[3 * k:3 * k + 3]
            for acc in (plain, lin, ring):
                acc.append(x)
            a, b = ring.partial(note_range), lin.partial(note_range)
            assert a[0] == b[0] and all(torch.equal(u, v) for u, v in zip(a[1:], b[1:]))
            parts.append(tuple(t.clone() for t in a[1:]))
        assert lin._chunk.dtype == torch.float16 and ring._chunk.dtype == torch.float16
        assert plain.n_frames == N and parts[-1][0].numel() > N // 2
        rows = plain.logits().clone()
        assert rows.dtype == torch.float32
        want = vit.decode_logits(rows, note_range)
        fp, fl, fr = plain.finish(note_range), lin.finish(note_range), ring.finish(note_range)
        for got in (fp, fl, fr):
            assert len(got) == 3 and all(u.dtype == v.dtype and torch.equal(u, v) for u, v in zip(got, want))
        for p in parts:                                      # partial() is a prefix of finish()
            assert all(torch.equal(u, v[:u.numel()]) for u, v in zip(p, fp))
