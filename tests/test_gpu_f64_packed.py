"""GPU tier of the packed ragged float64 decode: vit_decode_f64_packed / ViterbiDecoder.decode_f64_packed against the reference's own
float64 outputs (tests/golden), the NumPy restatement of that function run per song (tests/f64_ref.py) and the existing padded
decode_f64, by bit pattern.

The chunk rule the lengths are chosen from (include/viterbi_hip.h): cf = max(ceil(N / (8 x compute units)), 1024, ceil(tmax / 32)),
song b gets clamp(T_b / cf, 1, 32) chunks; slots: min(B, resident workgroups, max(1, N / tmax))."""
import numpy as np
import pytest
import torch

from tests import common, f64_ref
from tests.test_gpu_f64 import EDGE_PARAMS, EDGE_PLANS, PF, PLANS, premise_absorbing_f64
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)


def _pack(E, rows, lens):
    """[sum lens, S]: song k of the packed buffer is rows[k] of the padded E, cut to lens[k] frames"""
    return torch.cat([E[r, :n] for r, n in zip(rows, lens)], dim=0).contiguous()


def _decode_packed(dec, Ep, lens, **kw):
    """decode_f64_packed -> (list of int64 state arrays per song, loglik float64 [B] numpy)"""
    off = _offsets(lens)
    s, l = dec.decode_f64_packed(Ep, off, **kw)
    torch.cuda.synchronize()
    assert s.shape == (int(off[-1]),) and l.shape == (len(lens),) and l.dtype == torch.float64
    s = s.cpu().numpy().astype(np.int64)
    return [s[off[b]:off[b + 1]] for b in range(len(lens))], l.cpu().numpy()


def _padded(dec, E, lens):
    """the existing decode_f64 on a padded batch -> (states int64 [B, T], loglik float64 [B])"""
    s, l = dec.decode_f64(E, lengths=torch.as_tensor(np.asarray(lens, np.int64), device=dec.device))
    torch.cuda.synchronize()
    return s.cpu().numpy(), l.cpu().numpy()


def _assert_songs(got_s, got_l, rows, lens, ref_s, ref_l, what, by_value=False):
    """song k of the packed result against row rows[k] of a padded reference"""
    for k, (r, n) in enumerate(zip(rows, lens)):
        assert np.array_equal(got_s[k], ref_s[r, :n]), (what, k, n, "states differ in %d entries" % int(np.sum(got_s[k] != ref_s[r, :n])))
        assert np.all(got_s[k] >= 0), (what, k)
        if by_value:
            assert got_l[k] == ref_l[r], (what, k, got_l[k], ref_l[r])
        else:
            assert f64_ref.bits64(got_l[k]) == f64_ref.bits64(ref_l[r]), (what, k, got_l[k], ref_l[r])


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. the reference's own outputs
# ----------------------------------------------------------------------------------------------------------------------------------
def test_reference_float64_outputs_packed(golden, dev):
    """The four f64 cases of the golden manifest (S = 321; 500, 4000, 30000, 30000 frames) as one packed buffer of 64 500 rows: the
    states equal the reference's float64 path on every frame and differ from its float32 path in exactly the manifest's frames; the
    two short cases' log-likelihoods equal the restatement's.  N / tmax = 2: two slots walk two songs each; the long songs get 29
    chunks.  The recordings adapter returns the same paths for cases 0, 1 and 3."""
    from viterbi_spl_amd import reference_api as ra
    cases = golden["manifest"]["f64_cases"]
    lens = [c["T"] for c in cases]
    assert lens == [500, 4000, 30000, 30000]
    logs = []
    for c in cases:
        logA_T, log_pi, logE = f64_ref.manifest_log_inputs(golden, c)
        logs.append(logE)
    Ep = torch.from_numpy(np.concatenate(logs, axis=0)).to(dev)
    assert Ep.shape == (64500, 321)
    dec = ViterbiDecoder(logA_T, log_pi, dev)
    st, ll = _decode_packed(dec, Ep, lens)
    for b, c in enumerate(cases):
        k = c["index"]
        s64 = golden["data"][f"f64_{k}_states64"].astype(np.int64)
        s32 = golden["data"][f"f64_{k}_states32"].astype(np.int64)
        assert np.array_equal(st[b], s64), (c, int(np.sum(st[b] != s64)))
        assert int(np.sum(st[b] != s32)) == c["differing_frames"], c
    assert [c["differing_frames"] for c in cases] == [0, 0, 1157, 204]
    for b in (0, 1):
        rs, rd = f64_ref.decode_f64(logA_T, log_pi, logs[b])
        assert f64_ref.bits64(ll[b]) == f64_ref.bits64(rd[rs[-1]]), (b, ll[b], rd[rs[-1]])
    A, pi = golden["params"]["msnet321_A"], golden["params"]["msnet321_pi"]
    got = ra.viterbi_librosa_f64_recordings_fn(transition_matrix=A, prob_init=pi,
                                               probs_st_list=[f64_ref.manifest_case_probs(cases[b]) for b in (0, 1, 3)])
    assert len(got) == 3
    for g, b in zip(got, (0, 1, 3)):
        assert g.dtype == np.int64 and np.array_equal(g, st[b])


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. every (window width, wave count) pair a plan can reach, both storage types
# ----------------------------------------------------------------------------------------------------------------------------------
# Nine songs (a row of the 257-frame emission pool, a length) serve both sets.
# Set A: N = 423, tmax = 257 -> one slot walks all seven songs, longest first: 257, 100, 57, 5, 2, 1, 1 -- hand-overs odd -> even,
#   even -> odd, into and out of one-frame songs.
# Set B: N = 779 -> three slots: {257, 5}, {257, 2}, {100, 100, 57, 1}.
POOL_LENS = (257, 100, 57, 5, 2, 1, 1, 257, 100)
SET_A = (0, 1, 2, 3, 4, 5, 6)                 # lengths (257, 100, 57, 5, 2, 1, 1)
SET_B = (0, 5, 3, 1, 4, 7, 2, 8)              # lengths (257, 1, 5, 100, 2, 257, 57, 100)
SHORT = (1, 2, 3, PF - 1, PF, PF + 1)

_plan_cache = {}


def _plan_case(dev, W, S, half):
    """decoder, parameters, emissions on the fp16 grid (the same values serve both storage types) and the restatement's results per
    song, computed once per plan"""
    key = (W, S, half)
    if key not in _plan_cache:
        _plan_cache.clear()                          # one plan at a time: the parametrisation walks plan by plan
        logA_T, log_pi = f64_ref.band_params(S, half)
        dec = ViterbiDecoder(logA_T, log_pi, dev)
        assert dec.info["banded_ok"] and dec.info["floor_ok"] and dec.info["group_window"] == W and dec.info["n_dense_rows"] == 0, dec.info
        E16 = synth.emissions_dense(len(POOL_LENS), 257, S, seed=3 * S + W, dtype=torch.float16)
        E32 = E16.to(torch.float32).numpy()
        ref = f64_ref.decode_f64_batch(logA_T, log_pi, E32, POOL_LENS)
        short = {T: f64_ref.decode_f64_batch(logA_T, log_pi, E32[8:9, :T], [T]) for T in SHORT}
        _plan_cache[key] = (dec, logA_T, log_pi, E16, ref, short)
    return _plan_cache[key]


@pytest.mark.parametrize("f16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("W,S,half", PLANS, ids=[f"W{W}-S{S}" for W, S, _ in PLANS])
def test_every_instantiation_packed(dev, W, S, half, f16):
    """257-frame i.i.d. emissions: set A (one slot, seven songs) and set B (three slots) against the restatement per song and against
    decode_f64 padded; single-song buffers of 1, 2, 3 frames, of the prefetch depth and one on either side; all candidates tie."""
    assert [POOL_LENS[r] for r in SET_A] == [257, 100, 57, 5, 2, 1, 1] and [POOL_LENS[r] for r in SET_B] == [257, 1, 5, 100, 2, 257, 57, 100]
    dec, logA_T, log_pi, E16, ref, short = _plan_case(dev, W, S, half)
    E = (E16 if f16 else E16.to(torch.float32)).to(dev)
    pad_s, pad_l = _padded(dec, E, POOL_LENS)
    for what, rows in (("set A", SET_A), ("set B", SET_B)):
        lens = [POOL_LENS[r] for r in rows]
        st, ll = _decode_packed(dec, _pack(E, rows, lens), lens)
        _assert_songs(st, ll, rows, lens, ref[0], ref[1], what + " against the restatement")
        _assert_songs(st, ll, rows, lens, pad_s, pad_l, what + " against decode_f64 padded")
    for T, (rs, rl) in short.items():
        st, ll = _decode_packed(dec, E[8, :T].contiguous(), [T])
        _assert_songs(st, ll, (0,), (T,), rs, rl, f"one song of {T} frames")
    # every candidate ties.  fp32: sums of 1e30 absorb every matrix entry, every d row is one value; fp16 (no such magnitude): -inf
    tie = torch.full((1, 20, S), -np.inf if f16 else -1e30, dtype=E.dtype, device=dev)
    rs, rl = f64_ref.decode_f64_batch(logA_T, log_pi, tie.to(torch.float32).cpu().numpy(), [20])
    assert np.all(rs == 0) and (np.isneginf(rl[0]) if f16 else np.isfinite(rl[0]))
    lens = (7, 12, 1)
    st, ll = _decode_packed(dec, _pack(tie, (0, 0, 0), lens), lens)
    for k, n in enumerate(lens):
        assert np.all(st[k] == 0) and (np.isneginf(ll[k]) if f16 else np.isfinite(ll[k])), ("all candidates tie", k)
    st, ll = _decode_packed(dec, tie[0], [20])
    _assert_songs(st, ll, (0,), (20,), rs, rl, "all candidates tie")


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. value edges
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan,cls,f16", EDGE_PARAMS)
def test_value_edges_packed(dev, plan, cls, f16):
    """tests/common.py::edge_cases on the plans and classes of tests/test_gpu_f64.py::test_value_edges, the twelve ragged songs packed
    from the padded arrays; the premises are that test's, its float64 restatements of overflow_dead and absorbing included."""
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
        lens = [int(n) for n in lens]
        rows = tuple(range(len(lens)))
        st, ll = _decode_packed(dec, _pack(E, rows, lens), lens)
        _assert_songs(st, ll, rows, lens, ref_s, ref_l, name, by_value)
        ran += 1
    assert ran >= 1, "the parametrisation lists only combinations that yield a case"


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. back-trace chunking
# ----------------------------------------------------------------------------------------------------------------------------------
CHUNK_LENS = (5000, 1, 2047, 2048, 3100, 1023, 4097, 1024)      # cf = 1024: 4, 1, 1, 2, 3, 1, 4 and 1 chunks


@pytest.mark.parametrize("name", ["S100-W16", "tonet361"])
def test_backtrace_chunking_packed(golden, dev, name):
    """Songs of 1 to 4 chunks in one call, bt_warm in {default, 0} (zero warm-up makes every guess wrong: the verify pass decides),
    each setting twice: identical bytes throughout, equal to decode_f64 padded, and to the restatement for the 3100- and the
    1023-frame song; bt_chunks = 7 afterwards changes nothing (it is ignored)."""
    if name == "tonet361":
        A, pi = golden["params"]["tonet361_logA_T"], golden["params"]["tonet361_log_pi"]
    else:
        A, pi = f64_ref.band_params(100, 6)
    S = A.shape[0]
    dec = ViterbiDecoder(A, pi, dev)
    if name != "tonet361":
        assert dec.info["group_window"] == 16
    lens = list(CHUNK_LENS)
    assert sum(lens) // (8 * 256) < 1024 and max(lens) <= 32 * 1024, "cf = 1024 on any device of up to 256 compute units"
    assert [max(1, n // 1024) for n in lens] == [4, 1, 1, 2, 3, 1, 4, 1]
    B, T = len(lens), max(lens)
    E = synth.emissions_peaks(B, T, S, seed=S, device=dev)
    rows = tuple(range(B))
    Ep = _pack(E, rows, lens)
    pad_s, pad_l = _padded(dec, E, lens)
    off = _offsets(lens)
    base = None
    for warm in (-1, 0, "bt_chunks"):
        if warm == "bt_chunks":
            dec.set_option("bt_warm", -1)
            dec.set_option("bt_chunks", 7)
        else:
            dec.set_option("bt_warm", warm)
        for run in range(2):
            s, l = dec.decode_f64_packed(Ep, off, out_dtype=torch.int32)
            torch.cuda.synchronize()
            s, l = s.cpu().numpy(), l.cpu().numpy()
            if base is None:
                base = (s.copy(), l.copy())
            assert s.tobytes() == base[0].tobytes() and l.tobytes() == base[1].tobytes(), (warm, run)
    dec.set_option("reset", 0)
    st = [base[0][off[b]:off[b + 1]].astype(np.int64) for b in range(B)]
    _assert_songs(st, base[1], rows, lens, pad_s, pad_l, "against decode_f64 padded")
    for b in (4, 5):
        rs, rd = f64_ref.decode_f64(A, pi, E[b, :lens[b]].cpu().numpy())
        assert np.array_equal(st[b], rs) and f64_ref.bits64(base[1][b]) == f64_ref.bits64(rd[rs[-1]]), b


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. workspace and status codes, through the C ABI
# ----------------------------------------------------------------------------------------------------------------------------------
def test_stays_inside_its_workspace_packed(golden, dev):
    """A workspace of exactly vit_workspace_bytes_f64_packed bytes between two 64 KB guards, everything filled with 0xFF: the right
    result, the guards intact, no negative state; one byte less is VIT_EWORKSPACE with `states` untouched."""
    lib = _lib.load()
    A, pi = golden["params"]["tonet361_logA_T"], golden["params"]["tonet361_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    S, G = 361, 1 << 16
    lens = [130, 64, 1, 77]
    off = _offsets(lens)
    B, N = len(lens), int(off[-1])
    E = synth.emissions_dense(B, 130, S, seed=9, device=dev)
    Ep = _pack(E, range(B), lens)
    need = int(lib.vit_workspace_bytes_f64_packed(dec._plan, B, N))
    assert need > 0 and need == dec.workspace_bytes_f64_packed(B, N)
    buf = torch.full((G + 256 + need + 256 + G,), 0xFF, dtype=torch.uint8, device=dev)
    o = G + (-(buf.data_ptr() + G)) % 256
    ws = buf[o:o + need]
    assert ws.data_ptr() % 256 == 0
    st = torch.full((N,), -7, dtype=torch.int32, device=dev)
    ll = torch.zeros(B, dtype=torch.float64, device=dev)
    args = (dec._plan, Ep.data_ptr(), _lib.VIT_F32, B, off.ctypes.data, ws.data_ptr())
    assert lib.vit_decode_f64_packed(*args, need - 1, st.data_ptr(), ll.data_ptr(), None) == -4        # VIT_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((st == -7).all())
    assert lib.vit_decode_f64_packed(*args, need, st.data_ptr(), ll.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((buf[:o] == 0xFF).all()), "bytes in front of the workspace were written"
    assert bool((buf[o + need:] == 0xFF).all()), "bytes behind the workspace were written"
    assert bool((st >= 0).all())
    ref_s, ref_l = f64_ref.decode_f64_batch(A, pi, E.cpu().numpy(), lens)
    s = st.cpu().numpy().astype(np.int64)
    _assert_songs([s[off[b]:off[b + 1]] for b in range(B)], ll.cpu().numpy(), range(B), lens, ref_s, ref_l, "fenced workspace")
    # the same through a caller's workspace tensor; the log-likelihood not asked for
    assert lib.vit_decode_f64_packed(*args, need, st.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    s2, l2 = _decode_packed(dec, Ep, lens, workspace=torch.empty(need + 256, dtype=torch.uint8, device=dev))
    _assert_songs(s2, l2, range(B), lens, ref_s, ref_l, "caller's workspace")


def test_status_codes_packed(golden, dev):
    """Null pointers, a bad dtype, a misaligned workspace and bad offsets are VIT_EINVAL, B = 0 is VIT_OK, refused plans get size 0 and
    VIT_EUNSUPPORTED with `states` untouched; the workspace's vit_forward record is dropped; the float32 packed decode on the same
    decoder is undisturbed."""
    lib = _lib.load()
    p = golden["params"]
    dec = ViterbiDecoder(p["tonet361_logA_T"], p["tonet361_log_pi"], dev)
    S = 361
    lens = [10, 3]
    off = _offsets(lens)
    B, N = 2, 13
    E = synth.emissions_dense(B, 10, S, seed=1, device=dev)
    Ep = _pack(E, range(B), lens)
    need = int(lib.vit_workspace_bytes_f64_packed(dec._plan, B, N))
    wsb = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    ws = (wsb.data_ptr() + 255) & ~255
    st = torch.full((N,), -7, dtype=torch.int32, device=dev)
    ok = (dec._plan, Ep.data_ptr(), 0, B, off.ctypes.data, ws, need, st.data_ptr(), None, None)
    bad0 = np.asarray([1, 10, 13], np.int64)           # offsets[0] != 0
    rep = np.asarray([0, 10, 10], np.int64)            # a repeated offset: an empty song

    def call(**kw):
        names = ("plan", "logE", "dtype", "B", "offsets", "ws", "ws_bytes", "states", "loglik", "stream")
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.vit_decode_f64_packed(*a)
    assert call(plan=None) == -1 and call(offsets=None) == -1 and call(ws=None) == -1
    assert call(logE=None) == -1 and call(states=None) == -1
    assert call(dtype=7) == -1 and call(ws=ws + 8) == -1 and call(B=-1) == -1
    assert call(offsets=bad0.ctypes.data) == -1 and call(offsets=rep.ctypes.data) == -1
    assert call(B=0) == 0 and call(B=0, ws_bytes=0) == 0
    assert call(ws_bytes=need - 1) == -4
    torch.cuda.synchronize()
    assert bool((st == -7).all()), "a refused call wrote states"
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((st >= 0).all())
    # a float32 forward pass on record for the workspace is dropped: vit_backtrace must not walk the float64 history
    T = 10
    wsf = torch.empty(max(need, int(lib.vit_workspace_bytes(dec._plan, B, T))) + 256, dtype=torch.uint8, device=dev)
    wf = (wsf.data_ptr() + 255) & ~255
    s2 = torch.empty((B, T), dtype=torch.int32, device=dev)
    assert lib.vit_forward(dec._plan, E.data_ptr(), 0, B, T, None, wf, wsf.numel() - 256, None, 0, None) == 0
    assert lib.vit_backtrace(dec._plan, B, T, None, wf, wsf.numel() - 256, s2.data_ptr(), 0, None) == 0
    assert lib.vit_forward(dec._plan, E.data_ptr(), 0, B, T, None, wf, wsf.numel() - 256, None, 0, None) == 0
    assert lib.vit_decode_f64_packed(dec._plan, Ep.data_ptr(), 0, B, off.ctypes.data, wf, wsf.numel() - 256, st.data_ptr(), None, None) == 0
    assert lib.vit_backtrace(dec._plan, B, T, None, wf, wsf.numel() - 256, s2.data_ptr(), 0, None) == -7     # VIT_ENOFORWARD
    torch.cuda.synchronize()
    # the float32 packed decode before and after on the same decoder (the same staging buffer)
    s32, l32 = dec.decode_packed(Ep, off)
    s64, _ = dec.decode_f64_packed(Ep, off)
    s32b, l32b = dec.decode_packed(Ep, off)
    torch.cuda.synchronize()
    assert torch.equal(s32, s32b) and torch.equal(l32.view(torch.int32), l32b.view(torch.int32)) and bool((s64 >= 0).all())
    # plans the float64 family does not serve: size 0, VIT_EUNSUPPORTED before anything is enqueued
    A = np.array(p["tonet361_logA_T"])
    A[100, :] = -(np.arange(361) % 17).astype(np.float32) - 1                     # one dense row
    for what, A_, pi_ in (("unstructured", p["dense361_logA_T"], p["dense361_log_pi"]), ("Durrieu", p["durrieu722_logA_T"], p["durrieu722_log_pi"]),
                          ("dense row", A, p["tonet361_log_pi"])):
        d2 = ViterbiDecoder(A_, pi_, dev)
        S2 = A_.shape[0]
        assert int(lib.vit_workspace_bytes_f64_packed(d2._plan, B, N)) == 0, what
        E2 = _pack(synth.emissions_dense(B, 10, S2, seed=1, device=dev), range(B), lens)
        big = torch.empty(1 << 22, dtype=torch.uint8, device=dev)
        st.fill_(-7)
        rc = lib.vit_decode_f64_packed(d2._plan, E2.data_ptr(), 0, B, off.ctypes.data, (big.data_ptr() + 255) & ~255, 1 << 21, st.data_ptr(), None, None)
        torch.cuda.synchronize()
        assert rc == -5 and bool((st == -7).all()), what
        with pytest.raises(_lib.ViterbiHipError):
            d2.decode_f64_packed(E2, off)
        with pytest.raises(_lib.ViterbiHipError):
            d2.workspace_bytes_f64_packed(B, N)


# ----------------------------------------------------------------------------------------------------------------------------------
# 6. the workspace budget: consecutive groups of recordings
# ----------------------------------------------------------------------------------------------------------------------------------
def test_budget_groups(golden, dev):
    """Set B at S = 361 under a budget that yields at least three groups: the bytes of the unbudgeted call; a budget below the
    longest song's need raises before anything is written."""
    A, pi = golden["params"]["tonet361_logA_T"], golden["params"]["tonet361_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    lens = [POOL_LENS[r] for r in SET_B]
    off = _offsets(lens)
    E = synth.emissions_dense(len(POOL_LENS), 257, 361, seed=77, device=dev)
    Ep = _pack(E, SET_B, lens)
    s0, l0 = dec.decode_f64_packed(Ep, off)
    torch.cuda.synchronize()
    one = dec.workspace_bytes_f64_packed(1, 257)                  # the longest song alone
    # room for three recordings of 362 frames together: (257, 1, 5) fit and a fourth recording does not, (100, 2, 257) = 359 frames fit
    # and (57, 100) are left
    budget = dec.workspace_bytes_f64_packed(3, 362)
    mode = dec.plan_workspace_f64_packed(off, budget)
    groups = mode["groups"]
    assert groups == [(0, 3), (3, 6), (6, 8)], groups
    assert len(groups) >= 3 and groups[0][0] == 0 and groups[-1][1] == len(lens), groups
    assert all(a[1] == b[0] for a, b in zip(groups, groups[1:])) and mode["bytes"] <= budget
    for b0, b1 in groups:
        assert dec.workspace_bytes_f64_packed(b1 - b0, int(off[b1] - off[b0])) <= budget
    ws = torch.empty(mode["bytes"] + 256, dtype=torch.uint8, device=dev)
    for kw in ({}, {"workspace": ws}):
        s1, l1 = dec.decode_f64_packed(Ep, off, max_workspace_bytes=budget, **kw)
        torch.cuda.synchronize()
        assert torch.equal(s0, s1) and torch.equal(l0.view(torch.int64), l1.view(torch.int64)), kw
    assert dec.plan_workspace_f64_packed(off, None)["groups"] == [(0, len(lens))]
    # one recording alone does not fit: raised before anything is enqueued (the caller's workspace keeps its bytes)
    ws.fill_(0xA5)
    with pytest.raises(_lib.ViterbiHipError):
        dec.decode_f64_packed(Ep, off, max_workspace_bytes=one - 1, workspace=ws)
    with pytest.raises(_lib.ViterbiHipError):
        dec.plan_workspace_f64_packed(off, one - 1)
    torch.cuda.synchronize()
    assert bool((ws == 0xA5).all())
