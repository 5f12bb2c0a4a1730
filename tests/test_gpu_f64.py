"""GPU tier of the float64-accumulating decode: vit_decode_f64 / ViterbiDecoder.decode_f64 against the reference's own float64
outputs (tests/golden) and against the NumPy restatement of that function (tests/f64_ref.py), by bit pattern."""
import ctypes

import numpy as np
import pytest
import torch

from tests import common, f64_ref
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

PF = 4            # emission rows the forward kernel keeps in flight (kF64Prefetch, csrc/f64.hip)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _decode(dec, E, lens=None, **kw):
    """decode_f64 -> (states int64 [B, T] numpy, loglik float64 [B] numpy)"""
    ln = None if lens is None else torch.as_tensor(np.asarray(lens, np.int64), device=dec.device)
    s, l = dec.decode_f64(E, lengths=ln, **kw)
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
    """The four f64 cases of the golden manifest as one ragged batch [4, 30000, 321] fp32: the states equal the reference's float64
    path on every frame, are -1 past the lengths, and differ from its float32 path in exactly the manifest's frames (the premise
    that the test can tell the two arithmetics apart); the log-likelihoods of the two short cases equal the restatement's by bit
    pattern; the reference-signature adapter returns the same paths."""
    from viterbi_spl_amd import reference_api as ra
    cases = golden["manifest"]["f64_cases"]
    lens = [c["T"] for c in cases]
    assert lens == [500, 4000, 30000, 30000]
    E = torch.zeros((4, 30000, 321), dtype=torch.float32, device=dev)
    logs = []
    for b, c in enumerate(cases):
        logA_T, log_pi, logE = f64_ref.manifest_log_inputs(golden, c)
        logs.append(logE)
        E[b, :c["T"]] = torch.from_numpy(logE).to(dev)
    dec = ViterbiDecoder(logA_T, log_pi, dev)
    st, ll = _decode(dec, E, lens)
    for b, c in enumerate(cases):
        k, n = c["index"], c["T"]
        s64 = golden["data"][f"f64_{k}_states64"].astype(np.int64)
        s32 = golden["data"][f"f64_{k}_states32"].astype(np.int64)
        assert np.array_equal(st[b, :n], s64), (c, int(np.sum(st[b, :n] != s64)))
        assert np.all(st[b, n:] == -1)
        assert int(np.sum(st[b, :n] != s32)) == c["differing_frames"], c
    assert [c["differing_frames"] for c in cases] == [0, 0, 1157, 204]
    for b in (0, 1):
        rs, rd = f64_ref.decode_f64(logA_T, log_pi, logs[b])
        assert f64_ref.bits64(ll[b]) == f64_ref.bits64(rd[rs[-1]]), (b, ll[b], rd[rs[-1]])
    A, pi = golden["params"]["msnet321_A"], golden["params"]["msnet321_pi"]
    for b in (0, 3):
        got = ra.viterbi_librosa_f64_fn(transition_matrix=A, prob_init=pi, probs_st=f64_ref.manifest_case_probs(cases[b]))
        assert got.dtype == np.int64 and np.array_equal(got, st[b, :lens[b]])


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. every (window width, wave count) pair a plan can reach, both storage types, against the restatement
# ----------------------------------------------------------------------------------------------------------------------------------
# (states, half-width of synth's band recipe) -> window width; the plan takes a band only up to a quarter of the states, so the wide
# windows start at the larger grids.  S = 128, 256, 384, 512: no idle lane in the workgroup.
GRID = {16: ((100, 6), (200, 6), (321, 6), (450, 6), (722, 6)),
        32: ((128, 14), (200, 14), (361, 14), (450, 14), (722, 14)),
        64: ((256, 30), (321, 30), (450, 30), (722, 30)),
        84: ((361, 40), (450, 40), (722, 40)),
        96: ((384, 46), (450, 46), (722, 46)),
        128: ((512, 56), (722, 56))}
PLANS = [(W, S, half) for W, v in GRID.items() for S, half in v]
RAGGED = (257, 1, PF + 1, 100, 2)

_plan_cache = {}


def _plan_case(dev, W, S, half):
    """decoder, parameters, emissions on the fp16 grid (the same values serve both storage types) and the restatement's results,
    computed once per plan"""
    key = (W, S, half)
    if key not in _plan_cache:
        _plan_cache.clear()                          # one plan at a time: the parametrisation walks plan by plan
        logA_T, log_pi = f64_ref.band_params(S, half)
        dec = ViterbiDecoder(logA_T, log_pi, dev)
        assert dec.info["banded_ok"] and dec.info["floor_ok"] and dec.info["group_window"] == W and dec.info["n_dense_rows"] == 0, dec.info
        E16 = synth.emissions_dense(5, 257, S, seed=3 * S + W, dtype=torch.float16)
        E32 = E16.to(torch.float32).numpy()
        ref = f64_ref.decode_f64_batch(logA_T, log_pi, E32, RAGGED)
        short = {T: f64_ref.decode_f64_batch(logA_T, log_pi, E32[:1, :T], [T]) for T in (1, 2, 3, PF - 1, PF, PF + 1)}
        _plan_cache[key] = (dec, logA_T, log_pi, E16, ref, short)
    return _plan_cache[key]


@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("W,S,half", PLANS, ids=[f"W{W}-S{S}" for W, S, _ in PLANS])
def test_every_instantiation_against_the_restatement(dev, W, S, half, f16):
    """i.i.d. emissions: a ragged batch of five (lengths 257, 1, prefetch depth + 1, 100, 2) and single songs of 1, 2, 3 frames, of the
    prefetch depth and one on either side of it; all candidates tie (the path is state 0 throughout)."""
    dec, logA_T, log_pi, E16, ref, short = _plan_case(dev, W, S, half)
    E = (E16 if f16 else E16.to(torch.float32)).to(dev)
    st, ll = _decode(dec, E, RAGGED)
    _assert_same(st, ll, ref[0], ref[1], "ragged batch of five")
    s257, l257 = _decode(dec, E[0])                                     # [T, S]: a single song, no lengths
    assert np.array_equal(s257, ref[0][0]) and f64_ref.bits64(l257) == f64_ref.bits64(ref[1][0])
    for T, (rs, rl) in short.items():
        st, ll = _decode(dec, E[:1, :T].contiguous())
        _assert_same(st, ll, rs, rl, f"B = 1, T = {T}")
    # every candidate ties.  fp32: sums of 1e30 absorb every matrix entry, every d row is one value; fp16 (no such magnitude): -inf
    tie = torch.full((1, 20, S), -np.inf if f16 else -1e30, dtype=E.dtype, device=dev)
    rs, rl = f64_ref.decode_f64_batch(logA_T, log_pi, tie.to(torch.float32).cpu().numpy(), [20])
    assert np.all(rs == 0) and (np.isneginf(rl[0]) if f16 else np.isfinite(rl[0]))
    st, ll = _decode(dec, tie)
    _assert_same(st, ll, rs, rl, "all candidates tie")


# one plan per window width: 2, 6, 8 and 12 waves; W = 64 on eight waves keeps its weights as doubles, W = 96 / 128 on twelve waves keep
# part of theirs in LDS
EDGE_PLANS = {"S321-W32": (321, 14, False), "S321-W32-inf": (321, 14, True), "S100-W16-inf": (100, 6, True), "S722-W84": (722, 40, False),
              "S450-W64-inf": (450, 30, True), "S722-W96": (722, 46, False), "S722-W128-inf": (722, 56, True)}
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


def premise_absorbing_f64(ref_l, A):
    """the float64 form of common.premise_absorbing: the running sum absorbs every matrix entry in float64 too"""
    lo = np.float64(A[np.isfinite(A)].min())
    assert np.all(np.isfinite(ref_l)) and np.all(ref_l + lo == ref_l), ref_l


@pytest.mark.parametrize("plan,cls,f16", EDGE_PARAMS)
def test_value_edges(dev, plan, cls, f16):
    """tests/common.py::edge_cases (-inf entries, dead songs, a -inf prior, float32 overflow, fp16 bit patterns) on twelve ragged songs
    of up to 70 frames, each premise asserted on the restatement's output.  Two premises are restated for float64: a frame of
    -3e38 emissions overflows float32 but not float64 -- the song lives on, and its log-likelihood is below what float32 holds (the
    float32 premise sees exactly that: the value cast to float32 is -inf); the absorbing sums are compared in float64."""
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
            premise_absorbing_f64(ref_l, A2)
        else:
            with np.errstate(over="ignore"):
                premise(np.where(ref_s < 0, 0, ref_s), ref_l.astype(np.float32) if name == "overflow_dead" else ref_l)
        if name == "overflow_dead":
            assert np.all(np.isfinite(ref_l)) and np.any(ref_l < -3.5e38), ref_l
        E = torch.from_numpy(E16 if f16 else E32).to(dev)
        assert (E.dtype == torch.float16) == f16
        st, ll = _decode(dec, E, lens)
        _assert_same(st, ll, ref_s, ref_l, name, by_value)
        ran += 1
    assert ran >= 1, "the parametrisation lists only combinations that yield a case"


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. back-trace chunking
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tonet361", "jdc722"])
def test_backtrace_chunking(golden, dev, name):
    """bt_chunks in {1, 2, 7, 32} x bt_warm in {default, 0} (zero warm-up makes every guess wrong: the verify pass decides) at
    T = 1000, ragged: identical bytes throughout, and in a second run."""
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    S = A.shape[0]
    dec = ViterbiDecoder(A, pi, dev)
    lens = [1000, 517, 1, 999]
    E = synth.emissions_peaks(4, 1000, S, seed=S, device=dev)
    base = None
    for chunks in (1, 2, 7, 32):
        for warm in (-1, 0):
            dec.set_option("bt_chunks", chunks)
            dec.set_option("bt_warm", warm)
            for run in range(2):
                st, ll = _decode(dec, E, lens, out_dtype=torch.int32)
                if base is None:
                    base = (st.copy(), ll.copy())
                    rs, rd = f64_ref.decode_f64(A, pi, E[1, :517].cpu().numpy())      # one song against the restatement
                    assert np.array_equal(st[1, :517], rs) and f64_ref.bits64(ll[1]) == f64_ref.bits64(rd[rs[-1]])
                assert st.tobytes() == base[0].tobytes() and ll.tobytes() == base[1].tobytes(), (chunks, warm, run)
    for b, n in enumerate(lens):
        assert np.all(base[0][b, n:] == -1) and np.all(base[0][b, :n] >= 0)
    dec.set_option("reset", 0)


def test_empty_chunks_and_warmups_on_the_terminal_frame(dev):
    """The branches of the chunk scheme (bt_run_chunks) that the chunking tests above, of the packed and of the checkpointed decode do
    not reach with their songs of hundreds of frames: 32 chunks on songs of 1, 2, 65 and 130 frames (most chunks empty, some songs
    with fewer frames than chunks) and no warm-up (every warm-up point of a short song falls on its terminal frame).  The plan is
    f64_ref.band_params(100, 6) as it stands (S = 100, W = 16: the W16-S100 plan of GRID, not the -inf-floor sibling of EDGE_PLANS),
    fp32 emissions.  decode_f64 and decode_f64_checkpointed at K = 64 (three segments,
    the last of two frames) on [4, 130, 100]; decode_f64_packed on recordings of 1, 2, 3 and 65 frames (its chunk counts come from
    its table: one each).  States equal and log-likelihoods bit-equal to the restatement."""
    A, pi = f64_ref.band_params(100, 6)
    dec = ViterbiDecoder(A, pi, dev)
    assert dec.info["group_window"] == 16 and dec.info["floor_ok"]
    lens, plens = [1, 2, 65, 130], [1, 2, 3, 65]
    E = synth.emissions_peaks(4, 130, 100, seed=100, device=dev)
    ref = f64_ref.decode_f64_batch(A, pi, E.cpu().numpy(), lens)
    pref = f64_ref.decode_f64_batch(A, pi, E[:, :65].cpu().numpy(), plens)
    ln = torch.as_tensor(np.asarray(lens, np.int64), device=dev)
    Ep = torch.cat([E[b, :n] for b, n in enumerate(plens)], dim=0).contiguous()
    off = np.concatenate([[0], np.cumsum(plens)]).astype(np.int64)
    dec.set_option("bt_chunks", 32)
    dec.set_option("bt_warm", 0)
    try:
        st, ll = _decode(dec, E, lens)
        _assert_same(st, ll, ref[0], ref[1], "decode_f64")
        s, l = dec.decode_f64_checkpointed(E, segment_frames=64, lengths=ln)
        torch.cuda.synchronize()
        _assert_same(s.cpu().numpy(), l.cpu().numpy(), ref[0], ref[1], "decode_f64_checkpointed")
        s, l = dec.decode_f64_packed(Ep, off)
        torch.cuda.synchronize()
        s, l = s.cpu().numpy(), l.cpu().numpy()
        for b, n in enumerate(plens):
            assert np.array_equal(s[off[b]:off[b + 1]], pref[0][b, :n]), ("decode_f64_packed", b)
        assert np.array_equal(f64_ref.bits64(l), f64_ref.bits64(pref[1])), ("decode_f64_packed", l, pref[1])
    finally:
        dec.set_option("reset", 0)


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. workspace and status codes, through the C ABI
# ----------------------------------------------------------------------------------------------------------------------------------
def test_stays_inside_its_workspace(golden, dev):
    """A workspace of exactly vit_workspace_bytes_f64 bytes between two guards, everything filled with 0xFF: the right result, the
    guards intact; one byte less is VIT_EWORKSPACE."""
    lib = _lib.load()
    A, pi = golden["params"]["tonet361_logA_T"], golden["params"]["tonet361_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    B, T, S, G = 3, 130, 361, 1 << 16
    lens = np.asarray([130, 64, 1], np.int64)
    E = synth.emissions_dense(B, T, S, seed=9, device=dev)
    need = int(lib.vit_workspace_bytes_f64(dec._plan, B, T))
    assert need > 0 and need == dec.workspace_bytes_f64(B, T)
    buf = torch.full((G + 256 + need + 256 + G,), 0xFF, dtype=torch.uint8, device=dev)
    o = G + (-(buf.data_ptr() + G)) % 256
    ws = buf[o:o + need]
    assert ws.data_ptr() % 256 == 0
    st = torch.full((B, T), -7, dtype=torch.int32, device=dev)
    ll = torch.zeros(B, dtype=torch.float64, device=dev)
    ln = torch.from_numpy(lens).to(dev)
    args = (dec._plan, E.data_ptr(), _lib.VIT_F32, B, T, ln.data_ptr(), ws.data_ptr())
    assert lib.vit_decode_f64(*args, need - 1, st.data_ptr(), ll.data_ptr(), None) == -4        # VIT_EWORKSPACE
    assert bool((st == -7).all())
    assert lib.vit_decode_f64(*args, need, st.data_ptr(), ll.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((buf[:o] == 0xFF).all()), "bytes in front of the workspace were written"
    assert bool((buf[o + need:] == 0xFF).all()), "bytes behind the workspace were written"
    ref_s, ref_l = f64_ref.decode_f64_batch(A, pi, E.cpu().numpy(), lens)
    _assert_same(st.cpu().numpy().astype(np.int64), ll.cpu().numpy(), ref_s, ref_l, "fenced workspace")
    # the same through a caller's workspace tensor, log-likelihood not asked for
    assert lib.vit_decode_f64(*args, need, st.data_ptr(), None, None) == 0
    s2, l2 = dec.decode_f64(E, lengths=ln, workspace=torch.empty(need + 256, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    _assert_same(s2.cpu().numpy(), l2.cpu().numpy(), ref_s, ref_l, "caller's workspace")


def test_status_codes(golden, dev):
    """Null pointers and a bad dtype are VIT_EINVAL, refused plans VIT_EUNSUPPORTED with `states` untouched, B = 0 is VIT_OK."""
    lib = _lib.load()
    p = golden["params"]
    dec = ViterbiDecoder(p["tonet361_logA_T"], p["tonet361_log_pi"], dev)
    B, T, S = 2, 10, 361
    E = synth.emissions_dense(B, T, S, seed=1, device=dev)
    need = int(lib.vit_workspace_bytes_f64(dec._plan, B, T))
    wsb = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    ws = (wsb.data_ptr() + 255) & ~255
    st = torch.full((B, T), -7, dtype=torch.int32, device=dev)
    ok = (dec._plan, E.data_ptr(), 0, B, T, None, ws, need, st.data_ptr(), None, None)

    def call(**kw):
        names = ("plan", "logE", "dtype", "B", "T", "lengths", "ws", "ws_bytes", "states", "loglik", "stream")
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.vit_decode_f64(*a)
    assert call(plan=None) == -1 and call(logE=None) == -1 and call(ws=None) == -1 and call(states=None) == -1
    assert call(dtype=7) == -1 and call(ws=ws + 8) == -1 and call(T=0) == -1 and call(B=-1) == -1
    assert call(B=0) == 0 and call(B=0, ws_bytes=lib.vit_workspace_bytes_f64(dec._plan, 0, T)) == 0
    assert call(ws_bytes=need - 1) == -4
    torch.cuda.synchronize()
    assert bool((st == -7).all()), "a refused call wrote states"
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((st >= 0).all())
    # a float32 forward pass on record for the workspace is dropped: vit_backtrace must not walk the float64 history
    wsf = torch.empty(max(need, int(lib.vit_workspace_bytes(dec._plan, B, T))) + 256, dtype=torch.uint8, device=dev)
    wf = (wsf.data_ptr() + 255) & ~255
    assert lib.vit_forward(dec._plan, E.data_ptr(), 0, B, T, None, wf, wsf.numel() - 256, None, 0, None) == 0
    assert lib.vit_backtrace(dec._plan, B, T, None, wf, wsf.numel() - 256, st.data_ptr(), 0, None) == 0
    assert lib.vit_forward(dec._plan, E.data_ptr(), 0, B, T, None, wf, wsf.numel() - 256, None, 0, None) == 0
    assert lib.vit_decode_f64(dec._plan, E.data_ptr(), 0, B, T, None, wf, wsf.numel() - 256, st.data_ptr(), None, None) == 0
    assert lib.vit_backtrace(dec._plan, B, T, None, wf, wsf.numel() - 256, st.data_ptr(), 0, None) == -7     # VIT_ENOFORWARD
    torch.cuda.synchronize()
    # the Python path shares the decoder's buffer between the two decodes: float32, float64, float32 again
    s32, l32 = dec.decode(E)
    s64, _ = dec.decode_f64(E)
    s32b, l32b = dec.decode(E)
    torch.cuda.synchronize()
    assert torch.equal(s32, s32b) and torch.equal(l32.view(torch.int32), l32b.view(torch.int32)) and bool((s64 >= 0).all())
    # plans the float64 family does not serve: size 0, VIT_EUNSUPPORTED before anything is enqueued
    A = np.array(p["tonet361_logA_T"])
    A[100, :] = -(np.arange(361) % 17).astype(np.float32) - 1                     # one dense row
    for what, A_, pi_ in (("unstructured", p["dense361_logA_T"], p["dense361_log_pi"]), ("Durrieu", p["durrieu722_logA_T"], p["durrieu722_log_pi"]),
                          ("dense row", A, p["tonet361_log_pi"])):
        d2 = ViterbiDecoder(A_, pi_, dev)
        S2 = A_.shape[0]
        assert int(lib.vit_workspace_bytes_f64(d2._plan, B, T)) == 0, what
        E2 = synth.emissions_dense(B, T, S2, seed=1, device=dev)
        big = torch.empty(1 << 22, dtype=torch.uint8, device=dev)
        st.fill_(-7)
        rc = lib.vit_decode_f64(d2._plan, E2.data_ptr(), 0, B, T, None, (big.data_ptr() + 255) & ~255, 1 << 21, st.data_ptr(), None, None)
        torch.cuda.synchronize()
        assert rc == -5 and bool((st == -7).all()), what
        with pytest.raises(_lib.ViterbiHipError):
            d2.decode_f64(E2)
