"""GPU tier of the packed float64 decode under a workspace budget: vit_decode_f64_packed_checkpointed /
ViterbiDecoder.decode_f64_packed_checkpointed and the budget policy of decode_f64_packed_bounded, by bit pattern against the reference's
own float64 outputs (tests/golden), the NumPy restatement of that function run per song (tests/f64_ref.py) and the existing
decode_f64_packed.  The new decode is never its own reference.

Geometry the cases are chosen from (include/viterbi_hip.h): recording b has ceil(T_b / K) segments; pass 1 walks min(B, resident
workgroups, max(1, N / tmax)) slots; a pass-2 launch takes at most vit_f64_packed_bounded_units units, at most one per recording."""
import numpy as np
import pytest
import torch

from tests import common, f64_ref
from tests import guarded as gd
from tests.test_gpu_f64 import EDGE_PARAMS, EDGE_PLANS, PLANS, premise_absorbing_f64
from tests.test_gpu_f64_ckpt import GEO_K, GEO_LENS, _geo_case
from tests.test_gpu_f64_packed import POOL_LENS, SET_A, SET_B, _assert_songs, _offsets, _pack, _plan_case
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

OK, EINVAL, EWORKSPACE, EUNSUPPORTED, ENOTUPLOADED, ENOFORWARD = 0, -1, -4, -5, -6, -7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _split(s, off):
    s = s.cpu().numpy().astype(np.int64)
    return [s[off[b]:off[b + 1]] for b in range(len(off) - 1)]


def _decode_pc(dec, Ep, lens, K, **kw):
    """decode_f64_packed_checkpointed -> (list of int64 state arrays per song, loglik float64 [B] numpy)"""
    off = _offsets(lens)
    s, l = dec.decode_f64_packed_checkpointed(Ep, off, segment_frames=K, **kw)
    torch.cuda.synchronize()
    assert s.shape == (int(off[-1]),) and l.shape == (len(lens),) and l.dtype == torch.float64
    return _split(s, off), l.cpu().numpy()


def _decode_full(dec, Ep, lens):
    """the existing decode_f64_packed (full history) -> the same"""
    off = _offsets(lens)
    s, l = dec.decode_f64_packed(Ep, off)
    torch.cuda.synchronize()
    return _split(s, off), l.cpu().numpy()


def _assert_same_songs(got_s, got_l, ref_s, ref_l, what):
    for k, (g, r) in enumerate(zip(got_s, ref_s)):
        assert np.array_equal(g, r), (what, k, len(r), "states differ in %d entries" % int(np.sum(g != r)))
    assert np.array_equal(f64_ref.bits64(got_l), f64_ref.bits64(ref_l)), (what, got_l, ref_l)


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. the reference's own outputs
# ----------------------------------------------------------------------------------------------------------------------------------
def test_reference_float64_outputs(golden, dev):
    """The four f64 cases of the golden manifest (S = 321; 500, 4000, 30000, 30000 frames) as one packed buffer at K = 1024 (1, 4, 30
    and 30 segments): the states equal the reference's float64 path on every frame and differ from its float32 path in exactly the
    manifest's frames; states and log-likelihood bits equal decode_f64_packed's.  The recordings adapter under a budget of the size
    at K = 1024 returns the same paths for cases 0, 1 and 3."""
    from viterbi_spl_amd import reference_api as ra
    cases = golden["manifest"]["f64_cases"]
    lens = [c["T"] for c in cases]
    assert lens == [500, 4000, 30000, 30000]
    logs = []
    for c in cases:
        logA_T, log_pi, logE = f64_ref.manifest_log_inputs(golden, c)
        logs.append(logE)
    Ep = torch.from_numpy(np.concatenate(logs, axis=0)).to(dev)
    dec = ViterbiDecoder(logA_T, log_pi, dev)
    st, ll = _decode_pc(dec, Ep, lens, 1024)
    for b, c in enumerate(cases):
        k = c["index"]
        s64 = golden["data"][f"f64_{k}_states64"].astype(np.int64)
        s32 = golden["data"][f"f64_{k}_states32"].astype(np.int64)
        assert np.array_equal(st[b], s64), (c, int(np.sum(st[b] != s64)))
        assert int(np.sum(st[b] != s32)) == c["differing_frames"], c
    assert [c["differing_frames"] for c in cases] == [0, 0, 1157, 204]
    fs, fl = _decode_full(dec, Ep, lens)
    _assert_same_songs(st, ll, fs, fl, "against decode_f64_packed")
    three = (0, 1, 3)
    off3 = _offsets([lens[b] for b in three])
    budget = dec.workspace_bytes_f64_packed_checkpointed(off3, 1024)
    mode = dec.plan_workspace_f64_packed_bounded(off3, budget)
    assert mode == {"mode": "checkpointed", "segment_frames": 1024, "workspace_bytes": budget}, mode
    A, pi = golden["params"]["msnet321_A"], golden["params"]["msnet321_pi"]
    got = ra.viterbi_librosa_f64_recordings_fn(transition_matrix=A, prob_init=pi, max_workspace_bytes=budget,
                                               probs_st_list=[f64_ref.manifest_case_probs(cases[b]) for b in three])
    assert len(got) == 3
    for g, b in zip(got, three):
        assert g.dtype == np.int64 and np.array_equal(g, golden["data"][f"f64_{cases[b]['index']}_states64"].astype(np.int64)), b


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. every (window width, wave count) pair a plan can reach, both storage types
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("W,S,half", PLANS, ids=[f"W{W}-S{S}" for W, S, _ in PLANS])
def test_every_instantiation(dev, W, S, half, f16):
    """Set A (one slot walks seven songs: 257, 100, 57, 5, 2, 1, 1 -- both hand-over parities in pass 1) and set B (three slots) of
    tests/test_gpu_f64_packed.py at K = 64: the 257-frame songs have five units, the last of one frame; the 100-frame songs end inside
    their second unit; everything shorter is one unit from the prior.  Against the restatement per song."""
    assert [POOL_LENS[r] for r in SET_A] == [257, 100, 57, 5, 2, 1, 1] and [POOL_LENS[r] for r in SET_B] == [257, 1, 5, 100, 2, 257, 57, 100]
    dec, logA_T, log_pi, E16, ref, _ = _plan_case(dev, W, S, half)
    E = (E16 if f16 else E16.to(torch.float32)).to(dev)
    for what, rows in (("set A", SET_A), ("set B", SET_B)):
        lens = [POOL_LENS[r] for r in rows]
        st, ll = _decode_pc(dec, _pack(E, rows, lens), lens, 64)
        _assert_songs(st, ll, rows, lens, ref[0], ref[1], what + " against the restatement")


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. segment geometry
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("S,half", [(361, 14), (722, 40)], ids=["S361", "S722"])
def test_segment_geometry(dev, S, half, f16):
    """The twelve songs of tests/test_gpu_f64_ckpt.py::test_segment_geometry, packed: lengths on, one before and one behind segment
    boundaries at K in {64 .. 67} (every residue of the four-frame prefetch unroll, both buffer parities at a checkpoint), 128,
    199 .. 201 and 2^24.  The lengths K divides (64 and 128 at K = 64, 200 at K = 200) are the ones whose last frame has no checkpoint
    row; at K = 64 the 64-frame song is also placed LAST, where a stray store would land behind the checkpoint area.  Premise: every
    song of at least 63 frames changes state at least 30 times in the restatement, so a wrong hand-over cannot hide in a constant
    path."""
    dec, E16, (ref_s, ref_l) = _geo_case(dev, S, half)
    for b, n in enumerate(GEO_LENS):
        if n >= 63:
            assert int(np.sum(ref_s[b, 1:n] != ref_s[b, :n - 1])) >= 30, (S, b, n)
    E = (E16 if f16 else E16.to(torch.float32)).to(dev)
    rows = tuple(range(len(GEO_LENS)))
    Ep = _pack(E, rows, GEO_LENS)
    for K in GEO_K:
        st, ll = _decode_pc(dec, Ep, GEO_LENS, K)
        _assert_songs(st, ll, rows, GEO_LENS, ref_s, ref_l, f"K = {K}")
    last = tuple(r for r in rows if GEO_LENS[r] != 64) + tuple(r for r in rows if GEO_LENS[r] == 64)
    lens = [GEO_LENS[r] for r in last]
    assert lens[-1] == 64 and sorted(lens) == sorted(GEO_LENS)
    st, ll = _decode_pc(dec, _pack(E, last, lens), lens, 64)
    _assert_songs(st, ll, last, lens, ref_s, ref_l, "the 64-frame song last, K = 64")


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. more songs than units per launch
# ----------------------------------------------------------------------------------------------------------------------------------
def test_more_songs_than_units_per_launch(dev):
    """B = units per launch + 3 at S = 100, W = 16, lengths cycling through (130, 64, 1, 65), K = 64: up to three units per song,
    several launches, launches that are not full.  Against decode_f64_packed of the same buffer (independently tested; the
    restatement would take too long here) and against the restatement on the first eight songs."""
    A, pi = f64_ref.band_params(100, 6)
    dec = ViterbiDecoder(A, pi, dev)
    assert dec.info["group_window"] == 16
    cap = int(_lib.load().vit_f64_packed_bounded_units(dec._plan, 1 << 20))
    assert cap >= 1
    B = cap + 3
    cyc = (130, 64, 1, 65)
    lens = [cyc[b % 4] for b in range(B)]
    pool = synth.emissions_dense(64, 130, 100, seed=5, device=dev)
    rows = [b % 64 for b in range(B)]
    Ep = _pack(pool, rows, lens)
    st, ll = _decode_pc(dec, Ep, lens, 64)
    fs, fl = _decode_full(dec, Ep, lens)
    _assert_same_songs(st, ll, fs, fl, "against decode_f64_packed")
    ref_s, ref_l = f64_ref.decode_f64_batch(A, pi, pool[:8].cpu().numpy(), lens[:8])
    _assert_songs(st[:8], ll[:8], range(8), lens[:8], ref_s, ref_l, "the first eight songs against the restatement")


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. chunking inside units
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tonet361", "jdc722"])
def test_chunking_inside_units(golden, dev, name):
    """bt_chunks in {1, 2, 7, 32} x bt_warm in {default, 0} (zero warm-up makes every guess wrong: the verify pass decides), lengths
    (1000, 517, 1, 999) at K = 256: identical bytes throughout and in a second run, equal to decode_f64_packed's."""
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    S = A.shape[0]
    dec = ViterbiDecoder(A, pi, dev)
    lens = [1000, 517, 1, 999]
    off = _offsets(lens)
    Ep = _pack(synth.emissions_peaks(4, 1000, S, seed=S, device=dev), range(4), lens)
    bs, bl = dec.decode_f64_packed(Ep, off, out_dtype=torch.int32)
    torch.cuda.synchronize()
    base = (bs.cpu().numpy(), bl.cpu().numpy())
    assert np.all(base[0] >= 0)
    try:
        for chunks in (1, 2, 7, 32):
            for warm in (-1, 0):
                dec.set_option("bt_chunks", chunks)
                dec.set_option("bt_warm", warm)
                for run in range(2):
                    s, l = dec.decode_f64_packed_checkpointed(Ep, off, segment_frames=256, out_dtype=torch.int32)
                    torch.cuda.synchronize()
                    assert s.cpu().numpy().tobytes() == base[0].tobytes() and l.cpu().numpy().tobytes() == base[1].tobytes(), (chunks, warm, run)
    finally:
        dec.set_option("reset", 0)


# ----------------------------------------------------------------------------------------------------------------------------------
# 6. value edges
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan,cls,f16", EDGE_PARAMS)
def test_value_edges(dev, plan, cls, f16):
    """tests/common.py::edge_cases on the plans and classes of tests/test_gpu_f64.py::test_value_edges, the twelve ragged songs of up
    to 70 frames packed, at K = 64: dead frames and dead songs cross a checkpoint.  Each premise is asserted on the restatement."""
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
        lens = [int(n) for n in lens]
        assert (E.dtype == torch.float16) == f16 and max(lens) > 64, "a song crosses the checkpoint at frame 63"
        rows = tuple(range(len(lens)))
        st, ll = _decode_pc(dec, _pack(E, rows, lens), lens, 64)
        _assert_songs(st, ll, rows, lens, ref_s, ref_l, name, by_value)
        ran += 1
    assert ran >= 1, "the parametrisation lists only combinations that yield a case"


# ----------------------------------------------------------------------------------------------------------------------------------
# 7. guards
# ----------------------------------------------------------------------------------------------------------------------------------
_guard_cache = {}


def _guard_case(golden, dev):
    """tonet361, four songs at K = 64 (three, one, one and two units): the decoder, the packed emissions one element past a 256-byte
    boundary, the restatement of these songs and, for the neighbour poison, of the same songs under emissions of another seed"""
    if not _guard_cache:
        A, pi = golden["params"]["tonet361_logA_T"], golden["params"]["tonet361_log_pi"]
        lens = [130, 64, 1, 77]
        E = synth.emissions_dense(4, 130, 361, seed=9)
        other = synth.emissions_dense(4, 130, 361, seed=10)
        ref = f64_ref.decode_f64_batch(A, pi, E.numpy(), lens)
        nb_s, _ = f64_ref.decode_f64_batch(A, pi, other.numpy(), lens)
        _guard_cache["case"] = (A, pi, lens, E, ref, nb_s)
    return _guard_cache["case"]


@pytest.mark.parametrize("kind", gd.KINDS)
def test_guarded_buffers(golden, dev, kind):
    """A workspace of exactly the size function's bytes in an arena of 0xFF, `states` and `loglik` between guards over poison, the
    emissions one element past a 256-byte boundary: the right result and every arena intact.  One byte less of workspace is
    VIT_EWORKSPACE with `states`, `loglik` and the workspace still as they were.  Without `loglik` the states are the same."""
    lib = _lib.load()
    A, pi, lens, E, (ref_s, ref_l), nb_s = _guard_case(golden, dev)
    dec = ViterbiDecoder(A, pi, dev)
    off = _offsets(lens)
    B, N, K = len(lens), int(off[-1]), 64
    packed = np.concatenate([E[b, :n].numpy() for b, n in enumerate(lens)], axis=0)
    ea = gd.Arena(packed.nbytes, dev, lead=4)
    ea.store(packed)
    need = int(lib.vit_workspace_bytes_f64_packed_checkpointed(dec._plan, B, off.ctypes.data, K))
    assert need > 0 and need == dec.workspace_bytes_f64_packed_checkpointed(off, K)
    ws = gd.Arena(need, dev)
    poison = gd.poison_states(ref_s.astype(np.int32), 361, kind, nb_s.astype(np.int32) if kind == "neighbour" else None)
    poison = np.concatenate([poison[b, :n] for b, n in enumerate(lens)])
    st = gd.Arena(N * 4, dev, lead=4)
    st.store(poison)
    ll = gd.Arena(B * 8, dev)
    args = (dec._plan, ea.ptr, _lib.VIT_F32, B, off.ctypes.data, ws.ptr)
    assert lib.vit_decode_f64_packed_checkpointed(*args, need - 1, st.ptr, ll.ptr, K, None) == EWORKSPACE
    torch.cuda.synchronize()
    assert np.array_equal(st.view(torch.int32, (N,)).cpu().numpy(), poison), "a refused call wrote into states"
    assert ll.poisoned() and ws.poisoned(), "a refused call wrote into loglik or the workspace"
    assert lib.vit_decode_f64_packed_checkpointed(*args, need, st.ptr, ll.ptr, K, None) == OK
    torch.cuda.synchronize()
    gd.assert_decode_outputs(st, ll, ref_s, ref_l, lens, 0, offsets=off)
    for a, n in ((ws, "workspace"), (ea, "emissions"), (st, "states"), (ll, "loglik")):
        gd.assert_intact(a, n)
    assert np.array_equal(ea.view(torch.float32, packed.shape).cpu().numpy().view(np.uint32), packed.view(np.uint32)), "the emissions changed"
    got = st.view(torch.int32, (N,)).cpu().numpy().copy()
    st.store(poison)
    assert lib.vit_decode_f64_packed_checkpointed(*args, need, st.ptr, None, K, None) == OK
    torch.cuda.synchronize()
    assert np.array_equal(st.view(torch.int32, (N,)).cpu().numpy(), got), "the states depend on whether the log-likelihood is asked for"
    for a, n in ((ws, "workspace"), (st, "states")):
        gd.assert_intact(a, n)


# ----------------------------------------------------------------------------------------------------------------------------------
# 8. status codes and their order
# ----------------------------------------------------------------------------------------------------------------------------------
def test_status_codes(golden, dev):
    """Null pointers, a bad dtype, a misaligned workspace, B = -1, K = 63 and bad offsets are VIT_EINVAL (VIT_ENOTUPLOADED takes its place
    as in vit_decode_f64_packed), B = 0 is VIT_OK, a refused plan gets size 0 and VIT_EUNSUPPORTED with `states` untouched -- ahead of
    the offsets check, behind the K check -- and a vit_forward record on the workspace is gone afterwards."""
    lib = _lib.load()
    p = golden["params"]
    dec = ViterbiDecoder(p["tonet361_logA_T"], p["tonet361_log_pi"], dev)
    S, K = 361, 64
    lens = [70, 3]
    off = _offsets(lens)
    B, N = 2, 73
    E = synth.emissions_dense(B, 70, S, seed=1, device=dev)
    Ep = _pack(E, range(B), lens)
    need = int(lib.vit_workspace_bytes_f64_packed_checkpointed(dec._plan, B, off.ctypes.data, K))
    assert need > 0
    wsb = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    ws = (wsb.data_ptr() + 255) & ~255
    st = torch.full((N,), -7, dtype=torch.int32, device=dev)
    ok = (dec._plan, Ep.data_ptr(), 0, B, off.ctypes.data, ws, need, st.data_ptr(), None, K, None)
    bad0 = np.asarray([1, 70, 73], np.int64)           # offsets[0] != 0
    rep = np.asarray([0, 70, 70], np.int64)            # a repeated offset: an empty song

    def call(fn=lib.vit_decode_f64_packed_checkpointed, **kw):
        names = ("plan", "logE", "dtype", "B", "offsets", "ws", "ws_bytes", "states", "loglik", "K", "stream")
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a)
    assert call(plan=None) == EINVAL and call(offsets=None) == EINVAL and call(ws=None) == EINVAL
    assert call(logE=None) == EINVAL and call(states=None) == EINVAL
    assert call(dtype=7) == EINVAL and call(ws=ws + 8) == EINVAL and call(B=-1) == EINVAL
    assert call(K=63) == EINVAL and call(K=(1 << 24) + 1) == EINVAL
    assert call(offsets=bad0.ctypes.data) == EINVAL and call(offsets=rep.ctypes.data) == EINVAL
    assert call(B=0) == OK and call(B=0, ws_bytes=0) == OK and call(B=0, logE=None, states=None) == OK
    assert call(ws_bytes=need - 1) == EWORKSPACE
    assert call(ws_bytes=need - 1, logE=None) == EINVAL, "null logE is asked before the workspace size"
    torch.cuda.synchronize()
    assert bool((st == -7).all()), "a refused call wrote states"
    assert call() == OK
    torch.cuda.synchronize()
    assert bool((st >= 0).all())
    # a plan that is not uploaded: VIT_ENOTUPLOADED where vit_decode_f64_packed has it -- behind the null and range checks, ahead of
    # the alignment and dtype checks
    A_, pi_ = np.ascontiguousarray(p["tonet361_logA_T"], np.float32), np.ascontiguousarray(p["tonet361_log_pi"], np.float32)
    import ctypes
    host = ctypes.c_void_p()
    assert lib.vit_plan_create(A_.ctypes.data, pi_.ctypes.data, S, ctypes.byref(host)) == 0
    for kw in ({}, {"ws": ws + 8}, {"dtype": 7}, {"K": 63}):
        a = call(plan=host, **kw)
        b = lib.vit_decode_f64_packed(host, Ep.data_ptr(), kw.get("dtype", 0), B, off.ctypes.data, kw.get("ws", ws), need, st.data_ptr(), None, None)
        assert a == ENOTUPLOADED == b, (kw, a, b)
    assert call(plan=host, B=-1) == EINVAL and call(plan=host, ws=None) == EINVAL
    lib.vit_plan_destroy(host)
    # a float32 forward pass on record for the workspace is dropped: vit_backtrace must not walk the float64 rows
    T = 70
    wsf = torch.empty(max(need, int(lib.vit_workspace_bytes(dec._plan, B, T))) + 256, dtype=torch.uint8, device=dev)
    wf = (wsf.data_ptr() + 255) & ~255
    s2 = torch.empty((B, T), dtype=torch.int32, device=dev)
    assert lib.vit_forward(dec._plan, E.data_ptr(), 0, B, T, None, wf, wsf.numel() - 256, None, 0, None) == 0
    assert lib.vit_backtrace(dec._plan, B, T, None, wf, wsf.numel() - 256, s2.data_ptr(), 0, None) == 0
    assert lib.vit_forward(dec._plan, E.data_ptr(), 0, B, T, None, wf, wsf.numel() - 256, None, 0, None) == 0
    assert call(ws=wf, ws_bytes=wsf.numel() - 256) == OK
    assert lib.vit_backtrace(dec._plan, B, T, None, wf, wsf.numel() - 256, s2.data_ptr(), 0, None) == ENOFORWARD
    torch.cuda.synchronize()
    # plans the float64 family does not serve: size 0, no units, VIT_EUNSUPPORTED before anything is enqueued and before the offsets
    # are looked at; a bad K is still VIT_EINVAL
    A = np.array(p["tonet361_logA_T"])
    A[100, :] = -(np.arange(361) % 17).astype(np.float32) - 1                     # one dense row
    for what, A_, pi_ in (("unstructured", p["dense361_logA_T"], p["dense361_log_pi"]), ("Durrieu", p["durrieu722_logA_T"], p["durrieu722_log_pi"]),
                          ("dense row", A, p["tonet361_log_pi"])):
        d2 = ViterbiDecoder(A_, pi_, dev)
        S2 = A_.shape[0]
        assert int(lib.vit_workspace_bytes_f64_packed_checkpointed(d2._plan, B, off.ctypes.data, K)) == 0, what
        assert int(lib.vit_f64_packed_bounded_units(d2._plan, B)) == 0, what
        E2 = _pack(synth.emissions_dense(B, 70, S2, seed=1, device=dev), range(B), lens)
        big = torch.empty(1 << 23, dtype=torch.uint8, device=dev)
        st.fill_(-7)
        a2 = (d2._plan, E2.data_ptr(), 0, B, off.ctypes.data, (big.data_ptr() + 255) & ~255, 1 << 22, st.data_ptr(), None)
        assert lib.vit_decode_f64_packed_checkpointed(*a2, K, None) == EUNSUPPORTED, what
        assert lib.vit_decode_f64_packed_checkpointed(*a2[:4], bad0.ctypes.data, *a2[5:], K, None) == EUNSUPPORTED, what
        assert lib.vit_decode_f64_packed_checkpointed(*a2, 63, None) == EINVAL, what
        torch.cuda.synchronize()
        assert bool((st == -7).all()), what
        with pytest.raises(_lib.ViterbiHipError):
            d2.decode_f64_packed_checkpointed(E2, off, segment_frames=K)
        with pytest.raises(_lib.ViterbiHipError):
            d2.workspace_bytes_f64_packed_checkpointed(off, K)
        with pytest.raises(_lib.ViterbiHipError):
            d2.decode_f64_packed_bounded(E2, off, max_workspace_bytes=1 << 20)


# ----------------------------------------------------------------------------------------------------------------------------------
# 9. budget policy
# ----------------------------------------------------------------------------------------------------------------------------------
def test_budget_policy(golden, dev):
    """tonet361, eight recordings of up to 2000 frames: plan_workspace_f64_packed_bounded picks "full" where the whole history fits,
    else the largest fitting K, and raises below size(64); decode_f64_packed_bounded under each budget gives the bits of the
    unbudgeted call in ONE tensor of at most budget + 256 bytes.  A budget below the longest recording's own full history: the group
    policy of decode_f64_packed(max_workspace_bytes=) still refuses it, the bounded call decodes it."""
    A, pi = golden["params"]["tonet361_logA_T"], golden["params"]["tonet361_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    lens = [2000, 1, 1999, 700, 64, 1025, 513, 130]
    off = _offsets(lens)
    B, N = len(lens), int(off[-1])
    Ep = _pack(synth.emissions_peaks(B, 2000, 361, seed=41, device=dev), range(B), lens)
    full = dec.workspace_bytes_f64_packed(B, N)
    size = {K: dec.workspace_bytes_f64_packed_checkpointed(off, K) for K in (64, 128, 256, 512)}
    assert size[64] < size[128] < size[256] < size[512] < full
    base_s, base_l = dec.decode_f64_packed(Ep, off)
    torch.cuda.synchronize()
    plan = dec.plan_workspace_f64_packed_bounded
    assert plan(off) == {"mode": "full", "workspace_bytes": full} and plan(off, full) == {"mode": "full", "workspace_bytes": full}
    mid = (size[256] + size[512]) // 2
    assert plan(off, size[64]) == {"mode": "checkpointed", "segment_frames": 64, "workspace_bytes": size[64]}
    assert plan(off, mid) == {"mode": "checkpointed", "segment_frames": 256, "workspace_bytes": size[256]}
    one = dec.workspace_bytes_f64_packed(1, 2000)                    # the longest recording's own full history
    assert size[128] < one < size[256], "premise: a budget under the longest recording's own need that a segment length still meets"
    assert plan(off, one - 1) == {"mode": "checkpointed", "segment_frames": 128, "workspace_bytes": size[128]}

    used = []                                                  # every tensor a budgeted call decodes in
    inner = dec._call_workspace

    def spy(need, workspace):
        r = inner(need, workspace)
        used.append(r[0].numel())
        return r
    dec._call_workspace = spy
    try:
        dec._ws = torch.empty(2 * full + 256, dtype=torch.uint8, device=dev)     # a larger buffer kept from an earlier call: not decoded in
        for budget in (size[64], mid, one - 1, full, full + 1000):
            used.clear()
            s, l = dec.decode_f64_packed_bounded(Ep, off, max_workspace_bytes=budget)
            torch.cuda.synchronize()
            assert torch.equal(s, base_s) and torch.equal(l.view(torch.int64), base_l.view(torch.int64)), budget
            assert len(used) == 1 and used[0] <= budget + 256, (budget, used)
        # the group policy refuses what the bounded call just decoded
        with pytest.raises(_lib.ViterbiHipError):
            dec.decode_f64_packed(Ep, off, max_workspace_bytes=one - 1)
        with pytest.raises(_lib.ViterbiHipError):
            dec.plan_workspace_f64_packed(off, one - 1)
        # nothing fits: raised before anything is enqueued, the caller's workspace keeps its bytes
        mine = torch.full((full + 256,), 0xA5, dtype=torch.uint8, device=dev)
        used.clear()
        with pytest.raises(_lib.ViterbiHipError):
            dec.decode_f64_packed_bounded(Ep, off, max_workspace_bytes=size[64] - 1, workspace=mine)
        with pytest.raises(_lib.ViterbiHipError):
            plan(off, size[64] - 1)
        torch.cuda.synchronize()
        assert used == [] and bool((mine == 0xA5).all())
        # a caller's workspace of the planned size serves
        s, l = dec.decode_f64_packed_bounded(Ep, off, max_workspace_bytes=mid, workspace=mine[:size[256] + 256])
        torch.cuda.synchronize()
        assert torch.equal(s, base_s) and torch.equal(l.view(torch.int64), base_l.view(torch.int64))
    finally:
        dec._call_workspace = inner
