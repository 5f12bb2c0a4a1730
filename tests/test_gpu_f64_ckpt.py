"""GPU tier of the bounded-workspace float64 decode: vit_decode_f64_checkpointed / ViterbiDecoder.decode_f64_checkpointed and the budget
policy of decode_f64(max_workspace_bytes=), by bit pattern against the reference's float64 outputs (tests/golden), the NumPy
restatement (tests/f64_ref.py) and vit_decode_f64."""
import numpy as np
import pytest
import torch

from tests import common, f64_ref
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _lens(dec, lens):
    return None if lens is None else torch.as_tensor(np.asarray(lens, np.int64), device=dec.device)


def _ckpt(dec, E, K, lens=None, **kw):
    """decode_f64_checkpointed -> (states [B, T] numpy, loglik float64 [B] numpy)"""
    s, l = dec.decode_f64_checkpointed(E, segment_frames=K, lengths=_lens(dec, lens), **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), l.cpu().numpy()


def _full(dec, E, lens=None, **kw):
    s, l = dec.decode_f64(E, lengths=_lens(dec, lens), **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), l.cpu().numpy()


def _assert_same(got_s, got_l, ref_s, ref_l, what, by_value=False):
    assert np.array_equal(got_s, ref_s), (what, "states differ in %d entries" % int(np.sum(got_s != ref_s)))
    if by_value:
        assert np.array_equal(got_l, ref_l), (what, got_l, ref_l)
    else:
        assert np.array_equal(f64_ref.bits64(got_l), f64_ref.bits64(ref_l)), (what, got_l, ref_l)


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. the reference's own outputs
# ----------------------------------------------------------------------------------------------------------------------------------
def test_reference_float64_outputs(golden, dev):
    """The four f64 cases of the golden manifest as one ragged batch [4, 30000, 321] fp32 at K = 1024 (30 segments; songs 0 and 1 end
    inside the first four, so most segments skip them): the states equal the reference's float64 path on every frame, are -1 past
    the lengths and differ from its float32 path in exactly the manifest's frames; states and log-likelihood bits equal decode_f64's."""
    cases = golden["manifest"]["f64_cases"]
    lens = [c["T"] for c in cases]
    assert lens == [500, 4000, 30000, 30000]
    E = torch.zeros((4, 30000, 321), dtype=torch.float32, device=dev)
    for b, c in enumerate(cases):
        logA_T, log_pi, logE = f64_ref.manifest_log_inputs(golden, c)
        E[b, :c["T"]] = torch.from_numpy(logE).to(dev)
    dec = ViterbiDecoder(logA_T, log_pi, dev)
    st, ll = _ckpt(dec, E, 1024, lens)
    for b, c in enumerate(cases):
        k, n = c["index"], c["T"]
        s64 = golden["data"][f"f64_{k}_states64"].astype(np.int64)
        s32 = golden["data"][f"f64_{k}_states32"].astype(np.int64)
        assert np.array_equal(st[b, :n], s64), (c, int(np.sum(st[b, :n] != s64)))
        assert np.all(st[b, n:] == -1)
        assert int(np.sum(st[b, :n] != s32)) == c["differing_frames"], c
    assert [c["differing_frames"] for c in cases] == [0, 0, 1157, 204]
    fs, fl = _full(dec, E, lens)
    _assert_same(st, ll, fs, fl, "against decode_f64")


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. every (window width, wave count) pair a plan can reach, both storage types, against the restatement
# ----------------------------------------------------------------------------------------------------------------------------------
GRID = {16: ((100, 6), (200, 6), (321, 6), (450, 6), (722, 6)),
        32: ((128, 14), (200, 14), (361, 14), (450, 14), (722, 14)),
        64: ((256, 30), (321, 30), (450, 30), (722, 30)),
        84: ((361, 40), (450, 40), (722, 40)),
        96: ((384, 46), (450, 46), (722, 46)),
        128: ((512, 56), (722, 56))}
PLANS = [(W, S, half) for W, v in GRID.items() for S, half in v]
RAGGED = (257, 1, 5, 100, 2)

_plan_cache = {}


def _plan_case(dev, W, S, half):
    """decoder, emissions on the fp16 grid (the same values serve both storage types) and the restatement's results, once per plan"""
    key = (W, S, half)
    if key not in _plan_cache:
        _plan_cache.clear()                          # one plan at a time: the parametrisation walks plan by plan
        logA_T, log_pi = f64_ref.band_params(S, half)
        dec = ViterbiDecoder(logA_T, log_pi, dev)
        assert dec.info["banded_ok"] and dec.info["floor_ok"] and dec.info["group_window"] == W and dec.info["n_dense_rows"] == 0, dec.info
        E16 = synth.emissions_dense(5, 257, S, seed=3 * S + W, dtype=torch.float16)
        ref = f64_ref.decode_f64_batch(logA_T, log_pi, E16.to(torch.float32).numpy(), RAGGED)
        _plan_cache[key] = (dec, E16, ref)
    return _plan_cache[key]


@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("W,S,half", PLANS, ids=[f"W{W}-S{S}" for W, S, _ in PLANS])
def test_every_instantiation_against_the_restatement(dev, W, S, half, f16):
    """A ragged batch of five (lengths 257, 1, 5, 100, 2) at K = 64: four full segments plus a one-frame fifth for song 0, song 3 ends
    inside segment 1, the others inside segment 0; and a single [T, S] song without lengths."""
    dec, E16, ref = _plan_case(dev, W, S, half)
    E = (E16 if f16 else E16.to(torch.float32)).to(dev)
    st, ll = _ckpt(dec, E, 64, RAGGED)
    _assert_same(st, ll, ref[0], ref[1], "ragged batch of five")
    s257, l257 = _ckpt(dec, E[0], 64)
    assert s257.shape == (257,) and l257.shape == ()
    assert np.array_equal(s257, ref[0][0]) and f64_ref.bits64(l257) == f64_ref.bits64(ref[1][0])


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. segment geometry
# ----------------------------------------------------------------------------------------------------------------------------------
GEO_LENS = [200, 1, 2, 63, 64, 65, 66, 128, 129, 130, 193, 199]
GEO_K = (64, 65, 66, 67, 128, 199, 200, 201, 1 << 24)
_geo_cache = {}


def _geo_case(dev, S, half):
    if S not in _geo_cache:
        logA_T, log_pi = f64_ref.band_params(S, half)
        dec = ViterbiDecoder(logA_T, log_pi, dev)
        E16 = synth.emissions_dense(12, 200, S, seed=S + 7, dtype=torch.float16)
        ref = f64_ref.decode_f64_batch(logA_T, log_pi, E16.to(torch.float32).numpy(), GEO_LENS)
        _geo_cache[S] = (dec, E16, ref)
    return _geo_cache[S]


@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("S,half", [(361, 14), (722, 40)], ids=["S361", "S722"])
def test_segment_geometry(dev, S, half, f16):
    """Twelve songs whose lengths sit on, one before and one behind segment boundaries, at K in {64 .. 67} (every residue of the
    four-frame prefetch unroll, both buffer parities at a checkpoint), 128, T - 1, T, T + 1 and 2^24: one restatement per plan,
    every K gives its bits.  Premise: every song of at least 63 frames changes state at least 30 times, so a wrong hand-over between
    segments cannot hide in a constant path."""
    dec, E16, (ref_s, ref_l) = _geo_case(dev, S, half)
    for b, n in enumerate(GEO_LENS):
        if n >= 63:
            assert int(np.sum(ref_s[b, 1:n] != ref_s[b, :n - 1])) >= 30, (S, b, n)
    E = (E16 if f16 else E16.to(torch.float32)).to(dev)
    for K in GEO_K:
        st, ll = _ckpt(dec, E, K, GEO_LENS)
        _assert_same(st, ll, ref_s, ref_l, f"K = {K}")


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. chunking inside segments
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tonet361", "jdc722"])
def test_chunking_inside_segments(golden, dev, name):
    """bt_chunks in {1, 2, 7, 32} x bt_warm in {default, 0} (zero warm-up makes every guess wrong: the verify pass decides) at
    T = 1000, ragged, K = 256: identical bytes throughout and in a second run, equal to decode_f64's."""
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    S = A.shape[0]
    dec = ViterbiDecoder(A, pi, dev)
    lens = [1000, 517, 1, 999]
    E = synth.emissions_peaks(4, 1000, S, seed=S, device=dev)
    base = _full(dec, E, lens, out_dtype=torch.int32)
    try:
        for chunks in (1, 2, 7, 32):
            for warm in (-1, 0):
                dec.set_option("bt_chunks", chunks)
                dec.set_option("bt_warm", warm)
                for run in range(2):
                    st, ll = _ckpt(dec, E, 256, lens, out_dtype=torch.int32)
                    assert st.tobytes() == base[0].tobytes() and ll.tobytes() == base[1].tobytes(), (chunks, warm, run)
    finally:
        dec.set_option("reset", 0)
    for b, n in enumerate(lens):
        assert np.all(base[0][b, n:] == -1) and np.all(base[0][b, :n] >= 0)


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. value edges
# ----------------------------------------------------------------------------------------------------------------------------------
EDGE_PLANS = {"S321-W32-inf": (321, 14, True), "S722-W84": (722, 40, False), "S722-W128-inf": (722, 56, True)}
EDGE_CLASSES = ("sparse_inf", "dead_frame", "starved", "single_survivor", "dead_prior", "overflow_dead", "absorbing", "signed_zeros", "fp16_edges")


def _edge_applies(plan, cls, f16):
    """the combinations for which common.edge_cases yields a case: the classes that need a -inf floor, the float32-only ones, fp16 patterns"""
    if cls in ("starved", "single_survivor"):
        return EDGE_PLANS[plan][2]
    if cls in ("overflow_dead", "absorbing"):
        return not f16
    return f16 if cls == "fp16_edges" else True


EDGE_PARAMS = [pytest.param(plan, cls, f16, id=f"{plan}-{cls}-{'fp16' if f16 else 'fp32'}")
               for plan in EDGE_PLANS for cls in EDGE_CLASSES for f16 in (False, True) if _edge_applies(plan, cls, f16)]


@pytest.mark.parametrize("plan,cls,f16", EDGE_PARAMS)
def test_value_edges(dev, plan, cls, f16):
    """tests/common.py::edge_cases (seed 23, 70 frames) as test_value_edges of tests/test_gpu_f64.py builds them, at K = 64: the dead
    frames and dead songs cross a checkpoint.  Each premise is asserted on the restatement's output."""
    S, half, inf_floor = EDGE_PLANS[plan]
    A, pi = f64_ref.band_params(S, half)
    if inf_floor:
        A = common.inf_floor_sibling(A)
    ran = 0
    for name, A2, pi2, E32, E16, lens, premise, by_value in common.edge_cases(23, A, pi, 70, half=half, f16=f16, only=(cls,)):
        dec = ViterbiDecoder(A2, pi2, dev)
        assert dec.info["floor_ok"] and dec.info["n_dense_rows"] == 0
        ref_s, ref_l = f64_ref.decode_f64_batch(A2, pi2, E32, lens)
        if name == "absorbing":
            lo = np.float64(A2[np.isfinite(A2)].min())
            assert np.all(np.isfinite(ref_l)) and np.all(ref_l + lo == ref_l), ref_l
        else:
            with np.errstate(over="ignore"):
                premise(np.where(ref_s < 0, 0, ref_s), ref_l.astype(np.float32) if name == "overflow_dead" else ref_l)
        if name == "overflow_dead":
            assert np.all(np.isfinite(ref_l)) and np.any(ref_l < -3.5e38), ref_l
        E = torch.from_numpy(E16 if f16 else E32).to(dev)
        assert (E.dtype == torch.float16) == f16 and E.shape[1] > 64
        st, ll = _ckpt(dec, E, 64, lens)
        _assert_same(st, ll, ref_s, ref_l, name, by_value)
        ran += 1
    assert ran >= 1, "the parametrisation lists only combinations that yield a case"


# ----------------------------------------------------------------------------------------------------------------------------------
# 6. workspace fence and status codes, through the C ABI
# ----------------------------------------------------------------------------------------------------------------------------------
def test_stays_inside_its_workspace(golden, dev):
    """A workspace of exactly vit_workspace_bytes_f64_checkpointed bytes between two 64 KB guards, everything filled with 0xFF: the
    right result, the guards intact; one byte less is VIT_EWORKSPACE and `states` stays untouched."""
    lib = _lib.load()
    A, pi = golden["params"]["tonet361_logA_T"], golden["params"]["tonet361_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    B, T, S, K, G = 3, 130, 361, 64, 1 << 16
    lens = np.asarray([130, 64, 1], np.int64)
    E = synth.emissions_dense(B, T, S, seed=9, device=dev)
    need = int(lib.vit_workspace_bytes_f64_checkpointed(dec._plan, B, T, K))
    assert need > 0 and need == dec.workspace_bytes_f64_checkpointed(B, T, K)
    buf = torch.full((G + 256 + need + 256 + G,), 0xFF, dtype=torch.uint8, device=dev)
    o = G + (-(buf.data_ptr() + G)) % 256
    ws = buf[o:o + need]
    assert ws.data_ptr() % 256 == 0
    st = torch.full((B, T), -7, dtype=torch.int32, device=dev)
    ll = torch.zeros(B, dtype=torch.float64, device=dev)
    ln = torch.from_numpy(lens).to(dev)
    args = (dec._plan, E.data_ptr(), _lib.VIT_F32, B, T, ln.data_ptr(), ws.data_ptr())
    assert lib.vit_decode_f64_checkpointed(*args, need - 1, st.data_ptr(), ll.data_ptr(), K, None) == -4        # VIT_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((st == -7).all()) and bool((buf == 0xFF).all())
    assert lib.vit_decode_f64_checkpointed(*args, need, st.data_ptr(), ll.data_ptr(), K, None) == 0
    torch.cuda.synchronize()
    assert bool((buf[:o] == 0xFF).all()), "bytes in front of the workspace were written"
    assert bool((buf[o + need:] == 0xFF).all()), "bytes behind the workspace were written"
    ref_s, ref_l = f64_ref.decode_f64_batch(A, pi, E.cpu().numpy(), lens)
    _assert_same(st.cpu().numpy().astype(np.int64), ll.cpu().numpy(), ref_s, ref_l, "fenced workspace")
    # the same through a caller's workspace tensor, and with the log-likelihood not asked for
    st.fill_(-7)
    assert lib.vit_decode_f64_checkpointed(*args, need, st.data_ptr(), None, K, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), ref_s)
    s2, l2 = dec.decode_f64_checkpointed(E, segment_frames=K, lengths=ln, workspace=torch.empty(need + 256, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    _assert_same(s2.cpu().numpy(), l2.cpu().numpy(), ref_s, ref_l, "caller's workspace")


def test_status_codes(golden, dev):
    """Null pointers, a bad dtype, a misaligned workspace, T = 0, B = -1 and K = 63 are VIT_EINVAL, B = 0 is VIT_OK, refused plans get
    size 0 and VIT_EUNSUPPORTED with `states` untouched, and a vit_forward record on the workspace is gone afterwards."""
    lib = _lib.load()
    p = golden["params"]
    dec = ViterbiDecoder(p["tonet361_logA_T"], p["tonet361_log_pi"], dev)
    B, T, S, K = 2, 70, 361, 64
    E = synth.emissions_dense(B, T, S, seed=1, device=dev)
    need = int(lib.vit_workspace_bytes_f64_checkpointed(dec._plan, B, T, K))
    wsb = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    ws = (wsb.data_ptr() + 255) & ~255
    st = torch.full((B, T), -7, dtype=torch.int32, device=dev)
    ok = (dec._plan, E.data_ptr(), 0, B, T, None, ws, need, st.data_ptr(), None, K, None)

    def call(**kw):
        names = ("plan", "logE", "dtype", "B", "T", "lengths", "ws", "ws_bytes", "states", "loglik", "K", "stream")
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.vit_decode_f64_checkpointed(*a)
    assert call(plan=None) == -1 and call(logE=None) == -1 and call(ws=None) == -1 and call(states=None) == -1
    assert call(dtype=7) == -1 and call(ws=ws + 8) == -1 and call(T=0) == -1 and call(B=-1) == -1
    assert call(K=63) == -1 and call(K=(1 << 24) + 1) == -1
    assert call(B=0) == 0 and call(B=0, ws_bytes=lib.vit_workspace_bytes_f64_checkpointed(dec._plan, 0, T, K)) == 0
    assert call(ws_bytes=need - 1) == -4
    torch.cuda.synchronize()
    assert bool((st == -7).all()), "a refused call wrote states"
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((st >= 0).all())
    # a float32 forward pass on record for the workspace is dropped: vit_backtrace must not walk the float64 rows
    wsf = torch.empty(max(need, int(lib.vit_workspace_bytes(dec._plan, B, T))) + 256, dtype=torch.uint8, device=dev)
    wf = (wsf.data_ptr() + 255) & ~255
    assert lib.vit_forward(dec._plan, E.data_ptr(), 0, B, T, None, wf, wsf.numel() - 256, None, 0, None) == 0
    assert lib.vit_backtrace(dec._plan, B, T, None, wf, wsf.numel() - 256, st.data_ptr(), 0, None) == 0
    assert lib.vit_forward(dec._plan, E.data_ptr(), 0, B, T, None, wf, wsf.numel() - 256, None, 0, None) == 0
    assert lib.vit_decode_f64_checkpointed(dec._plan, E.data_ptr(), 0, B, T, None, wf, wsf.numel() - 256, st.data_ptr(), None, K, None) == 0
    assert lib.vit_backtrace(dec._plan, B, T, None, wf, wsf.numel() - 256, st.data_ptr(), 0, None) == -7     # VIT_ENOFORWARD
    torch.cuda.synchronize()
    # plans the float64 family does not serve: size 0, VIT_EUNSUPPORTED before anything is enqueued
    A = np.array(p["tonet361_logA_T"])
    A[100, :] = -(np.arange(361) % 17).astype(np.float32) - 1                     # one dense row
    for what, A_, pi_ in (("unstructured", p["dense361_logA_T"], p["dense361_log_pi"]), ("Durrieu", p["durrieu722_logA_T"], p["durrieu722_log_pi"]),
                          ("dense row", A, p["tonet361_log_pi"])):
        d2 = ViterbiDecoder(A_, pi_, dev)
        S2 = A_.shape[0]
        assert int(lib.vit_workspace_bytes_f64_checkpointed(d2._plan, B, T, K)) == 0, what
        E2 = synth.emissions_dense(B, T, S2, seed=1, device=dev)
        big = torch.empty(1 << 22, dtype=torch.uint8, device=dev)
        st.fill_(-7)
        rc = lib.vit_decode_f64_checkpointed(d2._plan, E2.data_ptr(), 0, B, T, None, (big.data_ptr() + 255) & ~255, 1 << 21, st.data_ptr(), None, K, None)
        torch.cuda.synchronize()
        assert rc == -5 and bool((st == -7).all()), what
        with pytest.raises(_lib.ViterbiHipError):
            d2.decode_f64_checkpointed(E2, segment_frames=K)
        with pytest.raises(_lib.ViterbiHipError):
            d2.workspace_bytes_f64_checkpointed(B, T, K)


# ----------------------------------------------------------------------------------------------------------------------------------
# 7. budget policy
# ----------------------------------------------------------------------------------------------------------------------------------
def test_budget_policy(golden, dev):
    """decode_f64(max_workspace_bytes=) at tonet361, B = 6, T = 2000, ragged: "full" where the whole history fits, else the largest
    fitting K with the bytes of the unbudgeted call; below size(64) it raises before anything is enqueued; under a budget no tensor
    larger than budget + 256 bytes is decoded in, whatever the decoder kept from an earlier call."""
    A, pi = golden["params"]["tonet361_logA_T"], golden["params"]["tonet361_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    B, T, S = 6, 2000, 361
    lens = [2000, 1, 1999, 700, 64, 1025]
    ln = _lens(dec, lens)
    E = synth.emissions_peaks(B, T, S, seed=41, device=dev)
    full = dec.workspace_bytes_f64(B, T)
    size = {K: dec.workspace_bytes_f64_checkpointed(B, T, K) for K in (64, 128, 256, 512)}
    assert size[64] < size[128] < size[256] < size[512] < full
    base_s, base_l = _full(dec, E, lens)                       # unbudgeted: leaves a full-size buffer in the decoder
    assert dec._ws is not None and dec._ws.numel() >= full + 256
    assert dec.plan_workspace_f64(B, T) == {"mode": "full", "workspace_bytes": full}
    assert dec.plan_workspace_f64(B, T, full) == {"mode": "full", "workspace_bytes": full}
    mid = (size[256] + size[512]) // 2
    assert dec.plan_workspace_f64(B, T, size[64]) == {"mode": "checkpointed", "segment_frames": 64, "workspace_bytes": size[64]}
    assert dec.plan_workspace_f64(B, T, mid) == {"mode": "checkpointed", "segment_frames": 256, "workspace_bytes": size[256]}

    used = []                                                  # every tensor a budgeted call decodes in
    inner = dec._call_workspace

    def spy(need, workspace):
        r = inner(need, workspace)
        used.append(r[0].numel())
        return r
    dec._call_workspace = spy
    try:
        for budget in (size[64], mid, full):
            used.clear()
            st, ll = dec.decode_f64(E, lengths=ln, max_workspace_bytes=budget)
            torch.cuda.synchronize()
            _assert_same(st.cpu().numpy(), ll.cpu().numpy(), base_s, base_l, f"budget {budget}")
            assert len(used) == 1 and used[0] <= budget + 256, (budget, used)
        # a full-mode budget above the need, with a larger buffer left in the decoder: that buffer is not the one decoded in
        dec._ws = torch.empty(2 * full + 256, dtype=torch.uint8, device=dev)
        used.clear()
        st, ll = dec.decode_f64(E, lengths=ln, max_workspace_bytes=full + 1000)
        torch.cuda.synchronize()
        _assert_same(st.cpu().numpy(), ll.cpu().numpy(), base_s, base_l, "full mode under a budget")
        assert len(used) == 1 and used[0] <= full + 1000 + 256, used
        # nothing fits: raised before anything is enqueued, the caller's workspace keeps its bytes
        mine = torch.full((full + 256,), 0xA5, dtype=torch.uint8, device=dev)
        used.clear()
        with pytest.raises(_lib.ViterbiHipError):
            dec.decode_f64(E, lengths=ln, max_workspace_bytes=size[64] - 1, workspace=mine)
        with pytest.raises(_lib.ViterbiHipError):
            dec.plan_workspace_f64(B, T, size[64] - 1)
        torch.cuda.synchronize()
        assert not used and bool((mine == 0xA5).all())
    finally:
        del dec._call_workspace
