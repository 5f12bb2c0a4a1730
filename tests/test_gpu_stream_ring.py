"""GPU tests of ring sessions (vit_stream_open_ring, vit_stream_commit_ack / _commit_rel / _tail; DecodeStream(ring_frames=),
RecordingAccumulator(ring_frames=)): recordings longer than the ring, decoded in R history rows with the bits of ``decode``.

Every parity test first asserts ON THE REFERENCE ALONE (tests/ring_ref.py over tests/commit_ref.py) that its schedule is accepted
(residency never violated), wraps the ring at least three times and exercises the ring's edges: a committed range and a merge walk
that straddle slot R - 1 -> 0, and an append that starts exactly at a slot 0.  All comparisons are exact."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests import commit_ref as cr
from tests import common, guarded
from tests import ring_ref as rr
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

PLANS = ["tonet361", "msnet321", "jdc722", "imm722w"]
POISON = -77
NO_CAP = 1 << 20
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -4, -5

# test 1: R = 64, T = 300.  (Only the first schedule can start an append at a slot 0: 26 + 40 k and 37 k are no multiple of 64 below 300.)
T1, R1 = 300, 64
SCHEDULES_1 = ([64, 1, 1, 3, 61, 1, 5, 59, 7, 1, 57, 9, 31], [1] * 9 + [2, 3, 5, 7] + [40] * 6 + [34], [37] * 8 + [4])
# test 2: dense emissions merge late: rings of 128 .. 256 rows, so 800 frames for three wraps; 32 divides every candidate R
T2, SCHEDULE_2, SEED_2 = 800, [32] * 25, 5
# the smallest ring of (128, 192, 256) the reference replay fits, per plan and (no cap, lookback 32) -- recorded from the reference
RING_2 = {"tonet361": (192, 192), "msnet321": (128, 128), "jdc722": (128, 256), "imm722w": (128, 256)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


_DECODERS = {}


def _decoder(golden, dev, name):
    if name not in _DECODERS:
        _DECODERS[name] = ViterbiDecoder(golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"], dev)
    return _DECODERS[name]


def _params(golden, name):
    return golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]


def _steps(E, counts_per_step, dev):
    """(chunk, counts or None) per append; counts_per_step: ints (every recording) or per-recording tuples"""
    B = E.shape[0]
    pos = np.zeros(B, np.int64)
    for c in counts_per_step:
        if np.isscalar(c):
            yield E[:, int(pos[0]):int(pos[0]) + int(c)].contiguous(), None
            pos += int(c)
        else:
            cnt = np.asarray(c, np.int64)
            buf = torch.full((B, max(int(cnt.max()), 1), E.shape[2]), float("nan"), device=dev, dtype=E.dtype)
            for b in range(B):
                buf[b, :cnt[b]] = E[b, pos[b]:pos[b] + cnt[b]]
            pos += cnt
            yield buf, cnt


def _per_recording(counts_per_step, B):
    return [[int(c) if np.isscalar(c) else int(c[b]) for c in counts_per_step] for b in range(B)]


def _drive(st, E, counts_per_step, replays, L, dev, rel_stride=None):
    """Append, commit_rel and ack step by step against the replays; then the tail.  -> (paths [B] of int32 arrays, loglik tensor)."""
    B = st.B
    R = st.ring_frames
    parts = [[] for _ in range(B)]
    f = np.zeros(B, np.int64)
    for k, (chunk, counts) in enumerate(_steps(E, counts_per_step, dev)):
        st.append(chunk, counts=counts)
        n = st.lengths
        stride = rel_stride or max(1, int(n.max()) if R is None else min(int(n.max()), R))
        states = torch.full((B, stride), POISON, dtype=torch.int32, device=dev)
        first = torch.full((B,), -9, dtype=torch.int64, device=dev)
        committed = torch.full((B,), -9, dtype=torch.int64, device=dev)
        st.commit_rel_into(states, first, committed, max_lookback=L)
        torch.cuda.synchronize()
        gf, gc, gs = first.cpu().numpy(), committed.cpu().numpy(), states.cpu().numpy()
        for b in range(B):
            want = replays[b][k]
            assert n[b] == want["n"]
            assert gf[b] == want["f0"] and gc[b] == want["f"], ("frontier", k, b, int(gf[b]), int(gc[b]), want["f0"], want["f"])
            m = want["f"] - want["f0"]
            assert np.array_equal(gs[b, :m], want["states"]), ("states", k, b, want["f0"], want["f"])
            assert (gs[b, m:] == POISON).all(), ("written outside the committed range", k, b)
            parts[b].append(gs[b, :m].copy())
        if R is not None:
            st.ack(gc)
        f = gc
    n = st.lengths
    stride = max(1, int((n - 0).max()) if R is None else min(int(n.max()), R))
    states = torch.full((B, stride), POISON, dtype=torch.int32, device=dev)
    first = torch.full((B,), -9, dtype=torch.int64, device=dev)
    loglik = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    st.tail_into(states, first, loglik)
    torch.cuda.synchronize()
    gs = states.cpu().numpy()
    assert np.array_equal(first.cpu().numpy(), f)
    for b in range(B):
        m = int(n[b] - f[b])
        assert (gs[b, m:] == POISON).all(), ("tail wrote outside [0, n - f)", b)
        parts[b].append(gs[b, :m].copy())
    return [np.concatenate(p) for p in parts], loglik


def _premise(replays, need_slot0=True, need_walk=True, moving=None):
    """The conditions of a parity test on its schedule, from the reference replay alone."""
    sums = [rr.summary(r) for r in replays]
    moving = range(len(replays)) if moving is None else moving
    for b in moving:
        assert sums[b]["resident"], ("the schedule violates residency on the reference", b)
        assert sums[b]["wraps"] >= 3, ("fewer than three wraps", b, sums[b])
        assert sums[b]["range_straddle"] >= 1, ("no committed range straddles slot R - 1 -> 0", b, sums[b])
    assert not need_walk or sum(sums[b]["walk_straddle"] for b in moving) >= 1, "no merge walk straddles slot R - 1 -> 0"
    assert not need_slot0 or sum(sums[b]["slot0"] for b in moving) >= 1, "no append starts at a slot 0"
    return sums


def _check_whole(dec, A, pi, E, lens, paths, loglik):
    En = E.float().cpu().numpy()
    ref_s, ref_l = vo.decode_c(A, pi, En, lengths=lens)
    ds, dl = dec.decode(E, lengths=torch.from_numpy(lens).to(E.device), out_dtype=torch.int32)
    for b in range(E.shape[0]):
        k = int(lens[b])
        assert np.array_equal(paths[b], ref_s[b, :k]), ("commits + tail differ from the oracle", b)
        assert np.array_equal(paths[b], ds[b, :k].cpu().numpy()), ("commits + tail differ from decode", b)
    assert np.array_equal(loglik.cpu().numpy().view(np.uint32), np.ascontiguousarray(ref_l, np.float32).view(np.uint32))
    assert torch.equal(loglik.view(torch.int32), dl.view(torch.int32))


@pytest.mark.parametrize("name", PLANS)
def test_peaks_three_schedules(golden, dev, name):
    """Test 1: peaks emissions, B = 2, R = 64, T = 300, float32 and float16, three schedules: after every append commit_rel's first,
    committed and states are the reference's, and the concatenated commits plus the tail are ``decode`` and the oracle."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    st = dec.stream(2, ring_frames=R1)
    lens = np.array([T1, T1], np.int64)
    for dt in (torch.float32, torch.float16):
        E = synth.emissions_peaks(2, T1, dec.S, seed=21, device=dev, dtype=dt)
        En = E.float().cpu().numpy()
        psis = [cr.back_pointers(A, pi, En[b]) for b in range(2)]
        slot0 = 0
        for sizes in SCHEDULES_1:
            assert sum(sizes) == T1
            replays = [rr.replay(psis[b], sizes, R1, NO_CAP) for b in range(2)]
            sums = _premise(replays, need_slot0=False)
            slot0 += sum(s["slot0"] for s in sums)
            st.reset()
            paths, loglik = _drive(st, E, sizes, replays, NO_CAP, dev)
            _check_whole(dec, A, pi, E, lens, paths, loglik)
        assert slot0 >= 1, "no append of the three schedules starts at a slot 0"
    st.close()


@pytest.mark.parametrize("name", PLANS)
def test_dense_smallest_ring(golden, dev, name):
    """Test 2: dense emissions (late merges), 800 frames in appends of 32, in the smallest ring of 128 / 192 / 256 rows the
    reference replay fits (RING_2 records which), uncapped and with a lookback of 32, whose run must stall and then commit."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    lens = np.array([T2, T2], np.int64)
    for dt in (torch.float32, torch.float16):
        E = synth.emissions_dense(2, T2, dec.S, seed=SEED_2, device=dev, dtype=dt)
        En = E.float().cpu().numpy()
        psis = [cr.back_pointers(A, pi, En[b]) for b in range(2)]
        for L, R_want in zip((NO_CAP, 32), RING_2[name]):
            R = rr.smallest_ring(psis, [SCHEDULE_2] * 2, L)
            assert R == R_want, (name, dt, L, R)
            replays = [rr.replay(psis[b], SCHEDULE_2, R, L) for b in range(2)]
            sums = _premise(replays)
            if L == 32:
                assert all(s["stall_then_commit"] for s in sums), "lookback 32: no stall followed by a commit"
            st = dec.stream(2, ring_frames=R)
            paths, loglik = _drive(st, E, SCHEDULE_2, replays, L, dev)
            _check_whole(dec, A, pi, E, lens, paths, loglik)
            st.close()


ACC_SEEDS = (3, 4)         # test 9: the two recordings' logits

RAGGED = [(1, 30, 40), (0, 20, 40), (0, 40, 0), (0, 38, 48), (0, 40, 40), (0, 0, 37), (0, 26, 20), (0, 45, 33), (0, 47, 32)]


@pytest.mark.parametrize("name", PLANS)
def test_ragged(golden, dev, name):
    """Test 3: counts with zeros through the per-launch tables: recording 0 stays at one frame, recordings 1 and 2 wrap in different
    appends (step 1: only recording 2; step 2: only recording 1) and both start step 4 at slot 0.  (The uniform path: tests 1, 2, 5.)"""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    per = _per_recording(RAGGED, 3)
    lens = np.array([sum(p) for p in per], np.int64)
    assert lens.tolist() == [1, 286, 290]
    st = dec.stream(3, ring_frames=64)
    for gen, dt in ((synth.emissions_peaks, torch.float32), (synth.emissions_peaks, torch.float16)):
        E = gen(3, int(lens.max()), dec.S, seed=21, device=dev, dtype=dt)
        En = E.float().cpu().numpy()
        psis = [cr.back_pointers(A, pi, En[b, :lens[b]]) for b in range(3)]
        replays = [rr.replay(psis[b], per[b], 64, NO_CAP) for b in range(3)]
        assert rr.summary(replays[0])["resident"]
        _premise(replays, moving=(1, 2))
        assert replays[2][1]["wraps"] == 1 and replays[1][1]["wraps"] == 0 and replays[1][2]["wraps"] == 1 and replays[2][2]["wraps"] == 0
        assert replays[1][4]["slot0"] and replays[2][4]["slot0"]
        st.reset()
        paths, loglik = _drive(st, E, RAGGED, replays, NO_CAP, dev)
        assert replays[0][-1]["f"] == 0 and len(paths[0]) == 1
        _check_whole(dec, A, pi, E, lens, paths, loglik)
    st.close()


@pytest.mark.parametrize("name", ["tonet361", "jdc722"])
def test_edge_values(golden, dev, name):
    """Test 4: a stretch of -inf rows across the wrap at frame 64 (recording 1), a recording that dies exactly in slot 0 of the second
    lap (recording 0, frame 64) and one dead from frame 0: state 0 and log-likelihood -inf, as everywhere else."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    T = 203
    rng = np.random.default_rng(3)
    En = common.dead_frame(rng, 4, T, dec.S, {0: 64, 2: 0})
    En[1, 62:67, :] = -np.inf
    E = torch.from_numpy(En).to(dev)
    sizes = [63, 1, 1, 1] + [17] * 8 + [1]          # (recording 3's sparse -inf entries merge up to 33 frames back: short appends)
    psis = [cr.back_pointers(A, pi, En[b]) for b in range(4)]
    replays = [rr.replay(psis[b], sizes, 64, NO_CAP) for b in range(4)]
    for b in range(4):
        s = rr.summary(replays[b])
        assert s["resident"] and s["wraps"] >= 3 and s["range_straddle"] >= 1, (b, s)
    st = dec.stream(4, ring_frames=64)
    paths, loglik = _drive(st, E, sizes, replays, NO_CAP, dev)
    lens = np.full(4, T, np.int64)
    _check_whole(dec, A, pi, E, lens, paths, loglik)
    ll = loglik.cpu().numpy()
    assert np.isneginf(ll[[0, 1, 2]]).all() and np.isfinite(ll[3])
    assert (paths[0][65:] == 0).all() and (paths[2][1:] == 0).all() and (paths[1][67:] == 0).all()
    st.close()


@pytest.mark.parametrize("name", ["tonet361", "msnet321", "jdc722"])
def test_long_run(golden, dev, name):
    """Test 5: 5000 frames in a ring of 256 rows, appends of 100, through DecodeStream.commit() / tail(): nineteen wraps.  The
    session accepting every append IS the residency premise here (an append past it raises); the straddles are read off the
    frontiers the commits return, which tests 1 to 4 hold against the reference."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    T, R, step = 5000, 256, 100
    E = synth.emissions_peaks(1, T, dec.S, seed=9, device=dev)
    st = dec.stream(1, ring_frames=R)
    parts, straddles, f = [], 0, 0
    for t in range(0, T, step):
        st.append(E[:, t:t + step].contiguous())
        first, committed, fresh = st.commit(out_dtype=torch.int32)
        assert first[0] == f and committed[0] >= f and fresh[0].numel() == committed[0] - first[0]
        straddles += int(committed[0] > f and f // R != (committed[0] - 1) // R)
        f = int(committed[0])
        parts.append(fresh[0].clone())
    assert (T - 1) // R >= 3 and straddles >= 3 and f > T - R
    tf, tail, loglik = st.tail(out_dtype=torch.int32)
    assert tf[0] == f and tail[0].numel() == T - f
    path = torch.cat(parts + [tail[0]])
    ds, dl = dec.decode(E, out_dtype=torch.int32)
    assert torch.equal(path, ds[0]) and torch.equal(loglik.view(torch.int32), dl.view(torch.int32))
    ref_s, ref_l = vo.decode_c(A, pi, E.cpu().numpy())
    assert np.array_equal(path.cpu().numpy(), ref_s[0]) and loglik.cpu().numpy()[0] == ref_l[0]
    with pytest.raises(_lib.ViterbiHipError):
        st.decode()
    st.close()


@pytest.mark.parametrize("name", ["tonet361", "imm722w"])
def test_tail_and_commit_rel_on_a_linear_session(golden, dev, name):
    """Test 6: on a session of vit_stream_open: tail == decode(frames so far)[f:n] after 0, 1 and several commits, and commit_rel's
    writes are commit's shifted by first."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    T = 203
    E = synth.emissions_peaks(2, T, dec.S, seed=21, device=dev)
    lin, rel = dec.stream(2, T), dec.stream(2, T)
    abs_states = torch.full((2, T), POISON, dtype=torch.int32, device=dev)
    abs_comm = torch.zeros((2,), dtype=torch.int64, device=dev)
    f = np.zeros(2, np.int64)
    t = 0
    for k, n in enumerate([40, 33, 1, 64, 65]):
        lin.append(E[:, t:t + n].contiguous())
        rel.append(E[:, t:t + n].contiguous())
        t += n
        ds, dl = dec.decode(E[:, :t].contiguous(), out_dtype=torch.int32)
        tf, tail, ll = rel.tail(out_dtype=torch.int32)                 # k = 0: before any commit: f = 0
        assert np.array_equal(tf, f)
        for b in range(2):
            assert torch.equal(tail[b], ds[b, int(f[b]):t])
        assert torch.equal(ll.view(torch.int32), dl.view(torch.int32))
        lin.commit_into(abs_states, abs_comm)
        rs = torch.full((2, t), POISON, dtype=torch.int32, device=dev)
        rf = torch.full((2,), -9, dtype=torch.int64, device=dev)
        rc = torch.full((2,), -9, dtype=torch.int64, device=dev)
        rel.commit_rel_into(rs, rf, rc)
        torch.cuda.synchronize()
        new = abs_comm.cpu().numpy()
        assert np.array_equal(rf.cpu().numpy(), f) and np.array_equal(rc.cpu().numpy(), new)
        for b in range(2):
            m = int(new[b] - f[b])
            assert torch.equal(rs[b, :m], abs_states[b, int(f[b]):int(new[b])]) and (rs[b, m:] == POISON).all()
        f = new.copy()
    assert f.min() >= 190
    with pytest.raises(_lib.ViterbiHipError):
        lin.ack([0, 0])
    lin.close()
    rel.close()


@pytest.mark.parametrize("name", ["tonet361", "imm722w"])
def test_guards(golden, dev, name):
    """Test 7: states of exactly [B, min(n, R)], first, committed, the ring workspace of exactly vit_workspace_bytes_stream_ring
    bytes and the commit buffer between guards over poisoned memory: nothing is written outside them, and inside `states` nothing
    outside [0, f' - f)."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    lib = _lib.load()
    B, R, T = 2, 64, 200
    E = synth.emissions_peaks(B, T, dec.S, seed=21, device=dev)
    En = E.cpu().numpy()
    psis = [cr.back_pointers(A, pi, En[b]) for b in range(B)]
    sizes = [64, 40, 40, 56]
    replays = [rr.replay(psis[b], sizes, R, NO_CAP) for b in range(B)]
    assert all(rr.summary(r)["resident"] and rr.summary(r)["wraps"] >= 3 for r in replays)
    need, cneed = int(lib.vit_workspace_bytes_stream_ring(dec._plan, B, R)), int(lib.vit_workspace_bytes_stream_commit(dec._plan, B))
    assert need > 0 and cneed > 0
    w_ar, c_ar = guarded.Arena(need, dev), guarded.Arena(cneed, dev)
    s_ar = guarded.Arena(B * R * 4, dev, fill=0xB3)
    f_ar, k_ar, l_ar = (guarded.Arena(B * 8, dev, fill=0xB3), guarded.Arena(B * 8, dev, fill=0xB3), guarded.Arena(B * 4, dev, fill=0xB3))
    poison = int(np.frombuffer(bytes([0xB3] * 4), np.int32)[0])
    h = ctypes.c_void_p()
    assert lib.vit_stream_open_ring(dec._plan, B, R, w_ar.ptr, need - 1, ctypes.byref(h)) == EWORKSPACE
    assert lib.vit_stream_open_ring(dec._plan, B, R, w_ar.ptr + 64, need, ctypes.byref(h)) == EINVAL
    assert lib.vit_stream_open_ring(dec._plan, B, R, w_ar.ptr, need, ctypes.byref(h)) == 0
    assert lib.vit_stream_commit_begin(h, c_ar.ptr, cneed) == 0
    stream = torch.cuda.current_stream(dev).cuda_stream
    arenas = ((w_ar, "ring workspace"), (c_ar, "commit state"), (s_ar, "states"), (f_ar, "first"), (k_ar, "committed"), (l_ar, "loglik"))
    t = 0
    for k, n in enumerate(sizes):
        chunk = E[:, t:t + n].contiguous()
        t += n
        assert lib.vit_stream_append(h, chunk.data_ptr(), 0, n, None, stream) == 0
        s_ar.payload.fill_(0xB3)
        assert lib.vit_stream_commit_rel(h, s_ar.ptr, R, f_ar.ptr, k_ar.ptr, NO_CAP, stream) == 0
        torch.cuda.synchronize()
        gs = s_ar.view(torch.int32, (B, R)).cpu().numpy()
        gc = k_ar.view(torch.int64, (B,)).cpu().numpy().copy()
        for b in range(B):
            want = replays[b][k]
            m = want["f"] - want["f0"]
            assert gc[b] == want["f"] and f_ar.view(torch.int64, (B,))[b].item() == want["f0"]
            assert np.array_equal(gs[b, :m], want["states"]) and (gs[b, m:] == poison).all()
        for ar, what in arenas:
            guarded.assert_intact(ar, what)
        assert lib.vit_stream_commit_ack(h, gc.ctypes.data) == 0
    s_ar.payload.fill_(0xB3)
    assert lib.vit_stream_tail(h, s_ar.ptr, R, f_ar.ptr, l_ar.ptr, stream) == 0
    torch.cuda.synchronize()
    gs = s_ar.view(torch.int32, (B, R)).cpu().numpy()
    ref_s, ref_l = vo.decode_c(A, pi, En)
    for b in range(B):
        assert np.array_equal(gs[b, :T - gc[b]], ref_s[b, gc[b]:]) and (gs[b, T - gc[b]:] == poison).all()
    assert np.array_equal(l_ar.view(torch.float32, (B,)).cpu().numpy(), ref_l)
    for ar, what in arenas:
        guarded.assert_intact(ar, what)
    lib.vit_stream_close(h)


def test_refusals(golden, dev):
    """Test 8: every refusal is a status, nothing is enqueued (outputs keep their poison) and no position moves."""
    dec = _decoder(golden, dev, "tonet361")
    lib = _lib.load()
    B, R = 2, 64
    E = synth.emissions_peaks(B, 300, dec.S, seed=21, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    # sizes
    for bad in (63, (1 << 30) + 1, 0, -5):
        assert int(lib.vit_workspace_bytes_stream_ring(dec._plan, B, bad)) == 0
    need = int(lib.vit_workspace_bytes_stream_ring(dec._plan, B, R))
    assert need > 0 and need == int(lib.vit_workspace_bytes_stream(dec._plan, B, R))
    ws = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device=dev)
    ptr = (ws.data_ptr() + 255) & ~255
    h = ctypes.c_void_p()
    assert lib.vit_stream_open_ring(dec._plan, B, 63, ptr, need, ctypes.byref(h)) == EINVAL
    assert lib.vit_stream_open_ring(dec._plan, B, (1 << 30) + 1, ptr, need, ctypes.byref(h)) == EINVAL
    assert not h.value
    for other in ("durrieu722", "dense64"):
        if f"{other}_logA_T" not in golden["params"]:
            continue
        od = _decoder(golden, dev, other)
        assert int(lib.vit_workspace_bytes_stream_ring(od._plan, B, R)) == 0
        assert lib.vit_stream_open_ring(od._plan, B, R, ptr, need, ctypes.byref(h)) == EUNSUPPORTED and not h.value
        with pytest.raises(_lib.ViterbiHipError):
            od.stream(B, ring_frames=R)
    un = ViterbiDecoder(synth.dense_random_log_transition(96, seed=1), np.log(synth.uniform_prior(96)), dev)
    assert int(lib.vit_workspace_bytes_stream_ring(un._plan, B, R)) == 0
    assert lib.vit_stream_open_ring(un._plan, B, R, ptr, need, ctypes.byref(h)) == EUNSUPPORTED and not h.value
    torch.cuda.synchronize()
    assert (ws == 0x5A).all()

    st = dec.stream(B, ring_frames=R)
    hs = st._handle()
    states = torch.full((B, R), POISON, dtype=torch.int32, device=dev)
    first = torch.full((B,), -9, dtype=torch.int64, device=dev)
    committed = torch.full((B,), -9, dtype=torch.int64, device=dev)
    cneed = int(lib.vit_workspace_bytes_stream_commit(dec._plan, B))
    cws = torch.full((cneed + 256,), 0x5A, dtype=torch.uint8, device=dev)
    cptr = (cws.data_ptr() + 255) & ~255
    sp, fp, kp = states.data_ptr(), first.data_ptr(), committed.data_ptr()
    # tail before commit_begin, commit_rel before commit_begin, tail with a 0-frame recording
    assert lib.vit_stream_tail(hs, sp, R, fp, None, stream) == EINVAL
    assert lib.vit_stream_commit_rel(hs, sp, R, fp, kp, 8, stream) == EINVAL
    assert lib.vit_stream_commit_begin(hs, cptr, cneed) == 0
    assert lib.vit_stream_tail(hs, sp, R, fp, None, stream) == EINVAL                       # no frame yet
    cnt = np.array([40, 0], np.int64)
    assert lib.vit_stream_append(hs, E[:, :40].contiguous().data_ptr(), 0, 40, cnt.ctypes.data, stream) == 0
    assert lib.vit_stream_tail(hs, sp, R, fp, None, stream) == EINVAL                       # recording 1 has none
    cnt = np.array([0, 40], np.int64)
    assert lib.vit_stream_append(hs, E[:, :40].contiguous().data_ptr(), 0, 40, cnt.ctypes.data, stream) == 0
    assert lib.vit_stream_tail(hs, sp, 39, fp, None, stream) == EINVAL                      # stride below the longest possible tail
    assert lib.vit_stream_tail(hs, None, R, fp, None, stream) == EINVAL and lib.vit_stream_tail(hs, sp, R, None, None, stream) == EINVAL
    assert lib.vit_stream_commit_rel(hs, sp, 39, fp, kp, 8, stream) == EINVAL
    assert lib.vit_stream_commit_rel(hs, sp, R, None, kp, 8, stream) == EINVAL
    assert lib.vit_stream_commit_rel(hs, sp, R, fp, kp, 0, stream) == EINVAL
    # the absolute calls on a ring
    big = torch.full((B, 300), POISON, dtype=torch.int32, device=dev)
    assert lib.vit_stream_backtrace(hs, big.data_ptr(), 300, None, stream) == EUNSUPPORTED
    assert lib.vit_stream_commit(hs, big.data_ptr(), 300, kp, 8, stream) == EUNSUPPORTED
    with pytest.raises(_lib.ViterbiHipError):
        st.decode()
    with pytest.raises(_lib.ViterbiHipError):
        st.commit_into(big, committed)
    torch.cuda.synchronize()
    assert (states == POISON).all() and (big == POISON).all() and (first == -9).all() and (committed == -9).all() and (cws == 0x5A).all()
    # residency: never acknowledge.  40 + 24 = 64 = R fits, one more frame does not
    assert lib.vit_stream_append(hs, E[:, 40:64].contiguous().data_ptr(), 0, 24, None, stream) == 0
    assert lib.vit_stream_commit_rel(hs, sp, R, fp, kp, NO_CAP, stream) == 0
    torch.cuda.synchronize()
    front = committed.cpu().numpy().copy()
    assert front.min() > 40                                                                # the device frontier moved; unacknowledged
    assert lib.vit_stream_append(hs, E[:, 64:65].contiguous().data_ptr(), 0, 1, None, stream) == EWORKSPACE
    cnt = np.array([0, 1], np.int64)
    assert lib.vit_stream_append(hs, E[:, 64:65].contiguous().data_ptr(), 0, 1, cnt.ctypes.data, stream) == EWORKSPACE
    assert st.lengths.tolist() == [64, 64]
    with pytest.raises(_lib.ViterbiHipError, match="ring"):
        st.append(E[:, 64:65].contiguous())
    # ack: a value above pos, then a good one, then one that goes down; NULL; nothing changes on a refusal
    bad = np.array([65, front[1]], np.int64)
    assert lib.vit_stream_commit_ack(hs, bad.ctypes.data) == EINVAL
    assert lib.vit_stream_append(hs, E[:, 64:65].contiguous().data_ptr(), 0, 1, None, stream) == EWORKSPACE    # (the good half was not taken)
    assert lib.vit_stream_commit_ack(hs, None) == EINVAL
    assert lib.vit_stream_commit_ack(hs, front.ctypes.data) == 0
    down = front - np.array([1, 0], np.int64)
    assert lib.vit_stream_commit_ack(hs, down.ctypes.data) == EINVAL
    assert lib.vit_stream_append(hs, E[:, 64:65].contiguous().data_ptr(), 0, 1, None, stream) == 0
    assert st.lengths.tolist() == [65, 65]
    # reset, then a full replay: the same bits as a fresh session
    A, pi = _params(golden, "tonet361")
    En = E.cpu().numpy()
    psis = [cr.back_pointers(A, pi, En[b]) for b in range(B)]
    sizes = SCHEDULES_1[2]
    replays = [rr.replay(psis[b], sizes, R, NO_CAP) for b in range(B)]
    st.reset()
    assert st.lengths.tolist() == [0, 0]
    p1, l1 = _drive(st, E, sizes, replays, NO_CAP, dev)
    st.reset()
    p2, l2 = _drive(st, E, sizes, replays, NO_CAP, dev)
    assert all(np.array_equal(a, b) for a, b in zip(p1, p2)) and torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    _check_whole(dec, A, pi, E, np.array([300, 300], np.int64), p2, l2)
    st.close()


def test_recording_accumulator_ring(dev):
    """Test 9: RecordingAccumulator(streaming=True, ring_frames=128) over 704 frames in appends of 96 (the last one 32): every
    partial() and finish() equal the linear streaming accumulator's."""
    from viterbi_spl_amd import reference_api as ra
    U = 360
    vit = ra.Viterbi(synth.tonet_transition(U, 14), synth.floored_prior(U + 1), device=dev)
    note_range = torch.linspace(30.0, 90.0, U, device=dev)
    ring = ra.RecordingAccumulator(vit, 704, streaming=True, ring_frames=128)
    lin = ra.RecordingAccumulator(vit, 704, streaming=True)
    with pytest.raises(ValueError):
        ra.RecordingAccumulator(vit, 704, streaming=False, ring_frames=128)
    for rec in range(2):                                    # (the second recording: finish() resets the session)
        # melody-like logits (synth.pitch_logits: survivors merge within a few frames, so 96 new frames fit a ring of 128 rows behind the
        # frontier), the unvoiced channel first, cut into snippets of 32 frames
        X = synth.pitch_logits(1, 704, U, seed=ACC_SEEDS[rec], device=dev)[0]
        snips = torch.cat([torch.zeros((704, 1), device=dev), X], dim=1).view(22, 32, U + 1).permute(0, 2, 1).contiguous()
        for k in range(8):
            x = snips[3 * k:3 * k + 3]
            ring.append(x)
            lin.append(x)
            a, b = ring.partial(note_range), lin.partial(note_range)
            assert a[0] == b[0] and all(torch.equal(u, v) for u, v in zip(a[1:], b[1:]))
        assert ring.n_frames == 704 and a[0] > 576
        fa, fb = ring.finish(note_range), lin.finish(note_range)
        assert len(fa) == len(fb) and all(u.dtype == v.dtype and torch.equal(u, v) for u, v in zip(fa, fb))
