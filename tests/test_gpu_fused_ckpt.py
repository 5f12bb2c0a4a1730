"""GPU tests of the fused logits -> path decode under a workspace budget (``vit_decode_logits_checkpointed``, csrc/fused_ckpt.hip): the
producer / consumer workgroup of the fused decode as the forward launch of the checkpointed scheme -- pass 1 keeps one delta row per
segment, every segment's emission rows are built again from the logits.  Every comparison is exact: states (-1 past a length) and
log-likelihood bits against ``decode_logits`` with the whole history, against the emission builder followed by ``decode(algo="wave")``,
and against the CPU oracle (``oracle.viterbi_oracle.decode_c``) on the stand-alone builder's rows for sampled songs."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests.common import logits_case
from tests.test_gpu_fused import CASES, _builder, _rows
from viterbi_spl_amd import ViterbiDecoder, _lib, synth
from viterbi_spl_amd import reference_api as ra

pytestmark = pytest.mark.gpu

OK, EINVAL, EWORKSPACE, EUNSUPPORTED, ENOTUPLOADED, ENOFORWARD = 0, -1, -4, -5, -6, -7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _lengths(B, T, K):
    """Lengths around the segment boundaries, rotated by B so that every batch size starts elsewhere.  In order: 1; K (ends with a
    segment); 2K; K + 2 (inside a ring phase of four frames behind a segment start); then -- the second workgroup of B = 9 -- K - 1,
    K + 1, 2K + 1 and T: one, two, three and (T > 3K) four segments in one workgroup, three of its songs ending before the last
    segment begins; 3.  Clamped to 1 .. T."""
    opts = [1, K, 2 * K, K + 2, K - 1, K + 1, 2 * K + 1, T, 3]
    return np.asarray([min(T, max(1, opts[(b + B) % len(opts)])) for b in range(B)], np.int64)


def _same(got, want, what):
    assert torch.equal(got[0], want[0]), f"{what}: states differ"
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), f"{what}: log-likelihood bits differ"


def _check(dec, A, pi, mode, prior, B, T, K, seed, dev, lengths_on, oracle=False):
    n_bins = dec.S - 1
    obs, build = _builder(mode, n_bins, prior)
    x = torch.from_numpy(_rows(mode, n_bins, B * T, seed)).to(dev).view(B, T, -1).contiguous()
    ln = _lengths(B, T, K) if lengths_on else np.full(B, T, np.int64)
    lengths = torch.from_numpy(ln).to(dev) if lengths_on else None
    what = f"mode {mode} B {B} T {T} K {K} lengths {ln.tolist() if lengths_on else None}"
    got = dec.decode_logits_checkpointed(x, obs, segment_frames=K, lengths=lengths, out_dtype=torch.int32)
    _same(got, dec.decode_logits(x, obs, lengths=lengths, out_dtype=torch.int32), what + " vs decode_logits")
    E = build(x)
    _same(got, dec.decode(E, lengths=lengths, algo="wave", out_dtype=torch.int32), what + " vs builder + decode(wave)")
    sh = got[0].cpu().numpy()
    for b in range(B):
        assert (sh[b, ln[b]:] == -1).all() and (sh[b, :ln[b]] >= 0).all(), f"{what}: song {b}"
    if oracle:
        Eh = E.cpu().numpy()
        for b in sorted({0, B // 2, B - 1}):
            ref_s, ref_l = vo.decode_c(A, pi, Eh[b, :ln[b]])
            assert np.array_equal(sh[b, :ln[b]], ref_s), f"{what}: song {b} differs from the oracle"
            assert np.float32(got[1][b].item()).tobytes() == np.float32(ref_l).tobytes(), f"{what}: log-likelihood of song {b} differs from the oracle"


def _kt_pairs():
    pairs = [(64, T) for T in (1, 2, 63, 64, 65, 67, 128, 129, 193)]
    for K in (65, 66):                       # not multiples of the ring's four frames
        pairs += [(K, T) for T in (K, K + 1, 2 * K - 1, 2 * K, 2 * K + 1, 3 * K + 2)]
    return pairs + [(4096, 70)]              # one segment of T frames


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. every builder, small shapes
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,with_prior", CASES)
def test_small_every_builder(golden, dev, name, mode, with_prior):
    """B around the four songs of a workgroup; T around one, two, three and four segments of K = 64, of K = 65 and 66 (segment starts
    that are no multiple of the ring phase) and below K = 4096; with and without lengths (see _lengths).  The oracle on three songs
    of the four-segment batches of nine."""
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    prior = torch.from_numpy(np.ascontiguousarray(golden["params"]["msnet321_pi"], np.float32)).to(dev) if with_prior else None
    seed = 100 * mode + (50 if with_prior else 0) + 7000
    for B in (1, 3, 4, 5, 9):
        for K, T in _kt_pairs():
            seed += 1
            oracle = B == 9 and T > 3 * K
            _check(dec, A, pi, mode, prior, B, T, K, seed, dev, lengths_on=False, oracle=oracle)
            _check(dec, A, pi, mode, prior, B, T, K, seed + 1000, dev, lengths_on=True, oracle=oracle)
    ln = _lengths(9, 197, 65)[4:8]
    assert sorted(-(-int(n) // 65) for n in ln) == [1, 2, 3, 4], "premise: one workgroup with four different segment counts"


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. the recursion's uniform-lane forms
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,opt", [("tonet361", 0, 2), ("tonet361", 0, 3), ("msnet321", 2, 3)])
def test_wave_uniform_forms(golden, dev, name, mode, opt):
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    dec.set_option("wave_uniform", opt)
    _check(dec, A, pi, mode, None, 5, 200, 66, 7900 + opt, dev, lengths_on=True, oracle=True)


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. guards
# ----------------------------------------------------------------------------------------------------------------------------------
def _carve(buf, start, nbytes, align=256):
    """-> (byte offset >= start of an `align`-aligned region of nbytes inside the uint8 tensor buf, the offset behind it)."""
    o = start + (-(buf.data_ptr() + start)) % align
    assert o + nbytes <= buf.numel()
    return o, o + nbytes


def test_stays_inside_its_buffers(golden, dev):
    """The workspace is exactly the size function's bytes between two 64 KB guards, `states` and `loglik` sit in the same 0xFF-poisoned
    buffer between guards: the right result and no byte outside the three regions changes; one byte less is VIT_EWORKSPACE and
    nothing at all is written; a workspace that starts as 0xFF, as the leftover of an earlier call on other songs, or as its own
    leftover gives the same bits."""
    lib = _lib.load()
    A, pi = golden["params"]["tonet361_logA_T"], golden["params"]["tonet361_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    obs, _ = _builder(0, 360)
    B, T, K, G = 5, 197, 65, 1 << 16
    ln = _lengths(9, T, K)[4:9].copy()                   # 1, 2, 3, 4 segments and a song of three frames
    x = torch.from_numpy(_rows(0, 360, B * T, 31)).to(dev).view(B, T, 360).contiguous()
    other = torch.from_numpy(_rows(0, 360, B * T, 32)).to(dev).view(B, T, 360).contiguous()
    lengths = torch.from_numpy(ln).to(dev)
    op = dec._obs_struct(obs)
    need = int(lib.vit_workspace_bytes_logits_checkpointed(dec._plan, ctypes.byref(op), B, T, K))
    assert need > 0 and need == dec.workspace_bytes_logits_checkpointed(obs, B, T, K) == dec.workspace_bytes_checkpointed(B, T, K)
    buf = torch.full((4 * G + need + 4 * B * T + 4 * B + 1024,), 0xFF, dtype=torch.uint8, device=dev)
    w0, w1 = _carve(buf, G, need)
    s0, s1 = _carve(buf, w1 + G, 4 * B * T, 4)
    l0, l1 = _carve(buf, s1 + G, 4 * B, 4)
    ws, st, ll = buf[w0:w1], buf[s0:s1], buf[l0:l1]
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(logits, ws_bytes):
        return lib.vit_decode_logits_checkpointed(dec._plan, logits.data_ptr(), ctypes.byref(op), B, T, lengths.data_ptr(), ws.data_ptr(), ws_bytes,
                                                  st.data_ptr(), ll.data_ptr(), K, stream)

    def outside_intact():
        return all(bool((buf[a:b] == 0xFF).all()) for a, b in ((0, w0), (w1, s0), (s1, l0), (l1, buf.numel())))

    assert call(x, need - 1) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool((buf == 0xFF).all()), "a refused call wrote something"
    want = dec.decode_logits(x, obs, lengths=lengths, out_dtype=torch.int32)
    results = []
    for first in (x, other, x, x):         # 0xFF workspace; other songs; the other songs' leftover; its own leftover (a second call)
        assert call(first, need) == OK
        torch.cuda.synchronize()
        assert outside_intact(), "bytes outside the workspace, states and loglik were written"
        results.append((st.view(torch.int32).view(B, T).clone(), ll.view(torch.float32).clone()))
    for k in (0, 2, 3):
        _same(results[k], want, f"guarded call {k}")
    assert not torch.equal(results[1][0], results[0][0]), "premise: the other songs decode differently"
    sh = results[0][0].cpu().numpy()
    for b in range(B):
        assert (sh[b, ln[b]:] == -1).all()


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. refusals and the order of the status codes
# ----------------------------------------------------------------------------------------------------------------------------------
def test_status_order_and_refusals(golden, dev):
    lib = _lib.load()
    p = golden["params"]
    dec = ViterbiDecoder(p["tonet361_logA_T"], p["tonet361_log_pi"], dev)
    obs, _ = _builder(0, 360)
    op = dec._obs_struct(obs)
    B, T, K = 3, 70, 64
    x = torch.from_numpy(logits_case(5, B * T, 360)).to(dev).view(B, T, 360).contiguous()
    need = int(lib.vit_workspace_bytes_logits_checkpointed(dec._plan, ctypes.byref(op), B, T, K))
    wsb = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    ws = (wsb.data_ptr() + 255) & ~255
    st = torch.full((B, T), -7, dtype=torch.int32, device=dev)
    ll = torch.full((B,), -7.0, dtype=torch.float32, device=dev)
    names = ("plan", "logits", "obs", "B", "T", "lengths", "ws", "ws_bytes", "states", "loglik", "K", "stream")
    ok = (dec._plan, x.data_ptr(), ctypes.byref(op), B, T, None, ws, need, st.data_ptr(), ll.data_ptr(), K, None)

    def call(base=ok, **kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.vit_decode_logits_checkpointed(*a)

    def obs_of(mode, n_bins, spw):
        return ctypes.byref(_lib.ObsParams(mode, n_bins, spw, -0.75, 1.386, 2.0, None))

    # a plan that was never uploaded: VIT_ENOTUPLOADED in front of every argument check but the two null checks
    A_, pi_ = np.ascontiguousarray(p["tonet361_logA_T"], np.float32), np.ascontiguousarray(p["tonet361_log_pi"], np.float32)
    raw = ctypes.c_void_p()
    assert lib.vit_plan_create(A_.ctypes.data, pi_.ctypes.data, 361, ctypes.byref(raw)) == 0
    assert call(plan=raw) == ENOTUPLOADED and call(plan=raw, ws=None, T=0, K=63, obs=obs_of(7, 5, 5)) == ENOTUPLOADED
    assert call(plan=raw, obs=None) == EINVAL and call(plan=None) == EINVAL and call(obs=None) == EINVAL
    lib.vit_plan_destroy(raw)
    # the common checks, the builder, the segment length
    assert call(ws=None) == EINVAL and call(ws=ws + 8) == EINVAL and call(T=0) == EINVAL and call(B=-1) == EINVAL
    assert call(obs=obs_of(7, 360, 5)) == EINVAL and call(obs=obs_of(0, 320, 5)) == EINVAL and call(obs=obs_of(0, 1, 5)) == EINVAL
    assert call(K=63) == EINVAL and call(K=(1 << 24) + 1) == EINVAL and call(K=0) == EINVAL
    # VIT_EUNSUPPORTED behind those and in front of the pointers and the workspace size: a builder geometry without an instantiation
    assert call(obs=obs_of(0, 360, 4)) == EUNSUPPORTED
    assert call(obs=obs_of(0, 360, 4), logits=None, states=None, ws_bytes=0) == EUNSUPPORTED
    assert call(obs=obs_of(0, 360, 4), K=63) == EINVAL
    assert call(logits=None) == EINVAL and call(states=None) == EINVAL
    assert call(logits=None, ws_bytes=need - 1) == EINVAL            # the pointers in front of the workspace size
    assert call(ws_bytes=need - 1) == EWORKSPACE and call(ws_bytes=0) == EWORKSPACE
    assert call(B=0) == OK and call(B=0, logits=None, states=None, ws_bytes=0) == OK
    dec.set_option("wave_uniform", 1)
    assert call() == EUNSUPPORTED
    dec.set_option("reset", 0)
    torch.cuda.synchronize()
    assert bool((st == -7).all()) and bool((ll == -7.0).all()), "a refused call wrote its outputs"
    # plans without the fused workgroup: size 0, VIT_EUNSUPPORTED, outputs untouched; n_bins + 1 != S and a bad K come first
    for name in ("jdc722", "dense361"):
        d2 = ViterbiDecoder(p[f"{name}_logA_T"], p[f"{name}_log_pi"], dev)
        S2 = d2.S
        o2 = ViterbiDecoder.obs_params("shaun", S2 - 1, 5, -0.75, 1.386, 2.0)
        assert d2.workspace_bytes_logits_checkpointed(o2, 2, 70, 64) == 0
        x2 = torch.zeros((2, 70, S2 - 1), device=dev)
        with pytest.raises(_lib.ViterbiHipError):
            d2.decode_logits_checkpointed(x2, o2, segment_frames=64)
        with pytest.raises(_lib.ViterbiHipError):
            d2.decode_logits(x2, o2, max_workspace_bytes=1 << 20)
        base = (d2._plan, x2.data_ptr(), obs_of(0, S2 - 1, 5), 2, 70, None, ws, need, st.data_ptr(), ll.data_ptr(), 64, None)
        assert call(base) == EUNSUPPORTED and call(base, logits=None) == EUNSUPPORTED
        assert call(base, K=63) == EINVAL and call(base, obs=obs_of(0, 100, 5)) == EINVAL
    torch.cuda.synchronize()
    assert bool((st == -7).all()) and bool((ll == -7.0).all()), "a refused call wrote its outputs"
    # the decode itself, without the log-likelihood; then: a vit_forward record on the workspace does not survive the call
    assert call(loglik=None) == OK
    torch.cuda.synchronize()
    assert torch.equal(st, dec.decode_logits(x, obs, out_dtype=torch.int32)[0]) and bool((ll == -7.0).all())
    E = synth.emissions_dense(B, T, 361, seed=1, device=dev)
    wsf = torch.empty(max(need, int(lib.vit_workspace_bytes(dec._plan, B, T))) + 256, dtype=torch.uint8, device=dev)
    wf = (wsf.data_ptr() + 255) & ~255
    s2 = torch.empty((B, T), dtype=torch.int32, device=dev)
    assert lib.vit_forward(dec._plan, E.data_ptr(), 0, B, T, None, wf, wsf.numel() - 256, None, 0, None) == OK
    assert lib.vit_backtrace(dec._plan, B, T, None, wf, wsf.numel() - 256, s2.data_ptr(), 0, None) == OK
    assert lib.vit_forward(dec._plan, E.data_ptr(), 0, B, T, None, wf, wsf.numel() - 256, None, 0, None) == OK
    assert call(ws=wf, ws_bytes=wsf.numel() - 256) == OK
    assert lib.vit_backtrace(dec._plan, B, T, None, wf, wsf.numel() - 256, s2.data_ptr(), 0, None) == ENOFORWARD
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. one full-length case
# ----------------------------------------------------------------------------------------------------------------------------------
def test_full_length(golden, dev):
    """Nine songs of up to 30000 frames at K = 1024 (30 segments), lengths ragged down to 1: the same bits as decode_logits; the oracle
    on the shortest and the longest song."""
    B, T, K = 9, 30000, 1024
    A, pi = golden["params"]["tonet361_logA_T"], golden["params"]["tonet361_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    obs, build = _builder(0, 360)
    X = synth.pitch_logits(B, T, 360, seed=5, device=dev)
    ln = np.asarray([T, 1, 1023, 1024, 1025, 29697, 17000, 2, 29999], np.int64)       # (29697 = 29 * 1024 + 1: one frame in the last segment)
    lengths = torch.from_numpy(ln).to(dev)
    got = dec.decode_logits_checkpointed(X, obs, segment_frames=K, lengths=lengths, out_dtype=torch.int32)
    _same(got, dec.decode_logits(X, obs, lengths=lengths, out_dtype=torch.int32), "full length")
    assert dec.workspace_bytes_logits_checkpointed(obs, B, T, K) * 20 < dec.workspace_bytes_logits(obs, B, T)
    for b in (1, 0):
        n = int(ln[b])
        ref_s, ref_l = vo.decode_c(A, pi, build(X[b:b + 1, :n])[0].cpu().numpy())
        assert np.array_equal(got[0][b, :n].cpu().numpy(), ref_s), f"song {b} differs from the oracle"
        assert np.float32(got[1][b].item()).tobytes() == np.float32(ref_l).tobytes()
        assert bool((got[0][b, n:] == -1).all())


# ----------------------------------------------------------------------------------------------------------------------------------
# 6. routing under a budget
# ----------------------------------------------------------------------------------------------------------------------------------
def test_budget_routing(golden, dev):
    """decode_logits(max_workspace_bytes=) and decode_logits_batch(fused=True, max_workspace_bytes=) at [8, 2000, 360] with a tenth of
    the whole history's bytes: the checkpointed form, device memory above inputs and outputs within the budget + 256 bytes, the
    bits of the unbudgeted call; nothing fits below the need at K = 64; emissions_out cannot be served under such a budget."""
    B, T = 8, 2000
    A361, pi361 = synth.tonet_transition(360, 14), synth.floored_prior(361)
    v = ra.Viterbi(A361, pi361, device=dev)                # a decoder of its own: nothing cached
    dec = v._decoder
    obs = v._obs_params()
    x = torch.from_numpy(logits_case(77, B * T, 360)).to(dev).view(B, T, 360).contiguous()
    lengths = torch.tensor([2000, 1, 64, 1999, 129, 1024, 1025, 700], dtype=torch.int64, device=dev)
    full = dec.workspace_bytes_logits(obs, B, T)
    budget = full // 10
    mode = dec.plan_workspace_logits(obs, B, T, budget)
    assert mode["mode"] == "checkpointed" and mode["workspace_bytes"] <= budget and mode["segment_frames"] == 128
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    got = dec.decode_logits(x, obs, lengths=lengths, out_dtype=torch.int32, max_workspace_bytes=budget)
    torch.cuda.synchronize()
    peak, outputs = torch.cuda.max_memory_allocated(dev) - before, torch.cuda.memory_allocated(dev) - before
    print(f"budget {budget} need {mode['workspace_bytes']} peak above the inputs {peak} outputs {outputs} whole history {full}")
    assert outputs <= 4 * B * T + 1024                     # states and loglik, each rounded up to the allocator's 512 bytes
    assert peak - outputs <= budget + 256, (peak, outputs, budget)
    want = dec.decode_logits(x, obs, lengths=lengths, out_dtype=torch.int32)
    _same(got, want, "budgeted decode_logits")
    # the reference's call surface: the same routing, the same voicing and bins as without a budget
    v2 = ra.Viterbi(A361, pi361, device=dev)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fused = v2.decode_logits_batch(x, lengths=lengths, fused=True, max_workspace_bytes=budget)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    outputs = 4 * B * T + 512 + 3 * (B * T + 512) + 4 * B * T + 512      # states, loglik; voiced as uint8 and bool, bins; the lengths copy
    print(f"decode_logits_batch: peak above the inputs {peak}")
    assert peak <= budget + 256 + outputs, (peak, budget, outputs)
    plain = v2.decode_logits_batch(x, lengths=lengths, fused=True)
    unfused = v2.decode_logits_batch(x, lengths=lengths, fused=False, max_workspace_bytes=budget)
    for f, q, u in zip(fused, plain, unfused):
        assert torch.equal(f, q) and torch.equal(f, u)
    # nothing fits below the least need (at this T: K = 64); the error comes before anything is enqueued or allocated
    least = dec.workspace_bytes_logits_checkpointed(obs, B, T, 64)
    assert least == min(dec.workspace_bytes_logits_checkpointed(obs, B, T, k) for k in (64, 128, 256, 512, 1024, 2048, 4096, 8192))
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.max_memory_allocated(dev)
    with pytest.raises(_lib.ViterbiHipError, match=str(least)):
        dec.decode_logits(x, obs, lengths=lengths, max_workspace_bytes=least - 1)
    with pytest.raises(_lib.ViterbiHipError):
        v2.decode_logits_batch(x, lengths=lengths, fused=True, max_workspace_bytes=least - 1)
    assert torch.cuda.max_memory_allocated(dev) == before
    eo = torch.empty((B, T, 361), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        dec.decode_logits(x, obs, emissions_out=eo, max_workspace_bytes=budget)
    s3, _ = dec.decode_logits(x, obs, lengths=lengths, out_dtype=torch.int32, emissions_out=eo, max_workspace_bytes=full)     # fits: the whole history
    assert torch.equal(s3, want[0])
