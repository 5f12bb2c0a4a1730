"""GPU tests of the commit point of a streaming session (vit_stream_commit*, DecodeStream.commit / commit_into,
RecordingAccumulator.partial): after every append the frontier and the newly written states of the NumPy reference of the
definition (tests/commit_ref.py), exactly; nothing written outside the committed range; the committed prefix is the prefix of
``decode`` and of the CPU oracle."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests import commit_ref as cr
from tests import common, guarded
from tests import floor_grid as fg
from tests import stream_grid as sg
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

PLANS = ["tonet361", "msnet321", "jdc722", "imm722w"]
T = 203
POISON = -77
NO_CAP = 1 << 20
SCHEDULES = ([203], [1] * 9 + [2, 3, 4, 5, 7, 8] + [40, 40, 40, 45], [64, 64, 75])


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


def _uniform(E, sizes):
    """appends of `sizes` frames for every recording: (chunk, counts=None)"""
    t = 0
    for n in sizes:
        yield E[:, t:t + n].contiguous(), None
        t += n


def _drive(st, steps, psis, L, stride, dev, f0=None):
    """Append and commit, step by step, against the reference.  -> (frontiers, states tensor, log of (b, n, f, f') per call)."""
    B = st.B
    states = torch.full((B, stride), POISON, dtype=torch.int32, device=dev)
    exp = np.full((B, stride), POISON, np.int32)
    f = np.zeros(B, np.int64) if f0 is None else f0.copy()
    log = []
    for chunk, counts in steps:
        st.append(chunk, counts=counts)
        n = st.lengths
        committed = torch.full((B,), -9, dtype=torch.int64, device=dev)
        st.commit_into(states, committed, max_lookback=L)
        torch.cuda.synchronize()
        want = f.copy()
        for b in range(B):
            f2, s = cr.commit(psis[b], n[b], f[b], L)
            exp[b, f[b]:f2] = s
            want[b] = f2
            log.append((b, int(n[b]), int(f[b]), int(f2)))
        got = committed.cpu().numpy()
        assert np.array_equal(got, want), ("frontier", n.tolist(), f.tolist(), got.tolist(), want.tolist())
        gs = states.cpu().numpy()
        bad = np.argwhere(gs != exp)
        assert bad.size == 0, ("states", n.tolist(), f.tolist(), want.tolist(), bad[:4].tolist(), gs[tuple(bad[0])], exp[tuple(bad[0])])
        f = want
    return f, states, log


@pytest.mark.parametrize("name", PLANS)
def test_frontier_and_states(golden, dev, name):
    """Test 1: commit after every append; three schedules; no cap and a 32-frame lookback; peaks and dense, float32 and float16."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    st = dec.stream(2, T)
    for kind, gen in (("peaks", synth.emissions_peaks), ("dense", synth.emissions_dense)):
        for dt in (torch.float32, torch.float16):
            E = gen(2, T, dec.S, seed=21, device=dev, dtype=dt)
            En = E.float().cpu().numpy()
            psis = [cr.back_pointers(A, pi, En[b]) for b in range(2)]
            ref_s, _ = vo.decode_c(A, pi, En)
            ds, _ = dec.decode(E, out_dtype=torch.int32)
            stall_then_commit = False
            for L in (NO_CAP, 32):
                for sizes in SCHEDULES:
                    st.reset()
                    f, states, log = _drive(st, _uniform(E, sizes), psis, L, T, dev)
                    for b in range(2):
                        k = int(f[b])
                        assert torch.equal(states[b, :k], ds[b, :k]) and np.array_equal(states[b, :k].cpu().numpy(), ref_s[b, :k])
                        if L == NO_CAP:           # on the reference: the test is not vacuous
                            assert k >= 150 and (kind != "peaks" or k >= 190), (name, kind, dt, b, k)
                        else:
                            mine = [(n, f1, f2) for bb, n, f1, f2 in log if bb == b]
                            stalls = [i for i, (n, f1, f2) in enumerate(mine) if n > 33 and f2 == f1]
                            stall_then_commit |= bool(stalls) and any(f2 > f1 for n, f1, f2 in mine[stalls[0] + 1:])
            if kind == "dense":
                assert stall_then_commit, (name, dt, "L = 32: no call that commits nothing followed by one that commits")
    st.close()


@pytest.mark.parametrize("name", PLANS)
def test_ragged(golden, dev, name):
    """Test 2: final lengths 1, 130, 203, counts with zeros.  The one-frame recording never commits, a recording without a new
    frame commits nothing new, `committed` is written for every recording (it is poisoned before every call)."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    lens = np.array([1, 130, 203], np.int64)
    plan = [(0, 0, 40), (1, 30, 40), (0, 33, 33), (0, 67, 67), (0, 0, 23)]
    st = dec.stream(3, T)
    for gen, dt in ((synth.emissions_peaks, torch.float32), (synth.emissions_dense, torch.float16)):
        E = gen(3, T, dec.S, seed=5, device=dev, dtype=dt)
        En = E.float().cpu().numpy()
        psis = [cr.back_pointers(A, pi, En[b, :lens[b]]) for b in range(3)]
        ref_s, _ = vo.decode_c(A, pi, En, lengths=lens)

        def steps():
            pos = np.zeros(3, np.int64)
            for cnt in plan:
                cnt = np.asarray(cnt, np.int64)
                buf = torch.full((3, int(cnt.max()), dec.S), float("nan"), device=dev, dtype=dt)
                for b in range(3):
                    buf[b, :cnt[b]] = E[b, pos[b]:pos[b] + cnt[b]]
                pos += cnt
                yield buf, cnt

        st.reset()
        f, states, log = _drive(st, steps(), psis, NO_CAP, T + 5, dev)
        assert np.array_equal(st.lengths, lens)
        assert f[0] == 0 and f[1] > 0 and f[2] > 0
        for k, cnt in enumerate(plan):
            for b in range(3):
                bb, n, f1, f2 = log[3 * k + b]
                assert bb == b and (cnt[b] > 0 or f2 == f1), (k, b, log[3 * k + b])
        for b in range(3):
            assert np.array_equal(states[b, :f[b]].cpu().numpy(), ref_s[b, :f[b]])
    st.close()


@pytest.mark.parametrize("name", ["tonet361", "jdc722"])
def test_edge_values(golden, dev, name):
    """Test 3: -inf entries, a stretch of -inf rows across chunk boundaries and songs that die (the inputs of
    tests/test_gpu_stream.py::test_edge_values): every back-pointer of a dead frame resolves to 0."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    rng = np.random.default_rng(3)
    En = common.dead_frame(rng, 4, T, dec.S, {0: 64, 2: 0})
    En[1, 62:67, :] = -np.inf
    E = torch.from_numpy(En).to(dev)
    psis = [cr.back_pointers(A, pi, En[b]) for b in range(4)]
    assert (psis[0][66:] == 0).all() and (psis[2][2:] == 0).all()
    ds, _ = dec.decode(E, out_dtype=torch.int32)
    st = dec.stream(4, T)
    for L in (NO_CAP, 32):
        st.reset()
        f, states, _ = _drive(st, _uniform(E, [63, 1, 1, 1, T - 66]), psis, L, T, dev)
        assert f[0] == T - 1 and f[2] == T - 1                # a dead song's survivors are the one state 0
        for b in range(4):
            assert torch.equal(states[b, :f[b]], ds[b, :f[b]])
    st.close()


GRID_SERVED = [e for e in fg.GRID if (e[0], e[1]) in sg.STREAM_SERVED]


@pytest.mark.parametrize("entry", GRID_SERVED, ids=fg.plan_id)
def test_forced_hops_every_geometry(dev, entry):
    """Test 4: every served (window, waves) pair on the hop batch (the path leaves the window at frames 64 / 128 / 192, and in an
    eighth of all steps), 64 frames an append: the many-lane full evaluation, the candidate table in LDS and in global memory."""
    dec, batches, keep = sg.plan_case(dev, entry)
    name, E, lens, ref_s, _ = batches[2]
    assert name == "hops" and len(GRID_SERVED) == len(sg.STREAM_SERVED)
    A, pi = keep["A"], keep["pi"]
    B = len(lens)
    psis = [cr.back_pointers(A, pi, E[b, :max(int(lens[b]), 1)]) for b in range(B)]
    sched = sg.schedule("segments", lens, fg.T)
    En = sg.nan_rows(torch.from_numpy(E.copy()).to(dev), lens)
    rows = torch.arange(B, device=dev)[:, None]

    def steps():
        pos = np.zeros(B, np.int64)
        for n, cnt in sched:
            k = np.arange(n)[None, :]
            idx = np.where(k < cnt[:, None], pos[:, None] + k, fg.T)
            pos += cnt
            yield En[rows, torch.from_numpy(idx).to(dev)].contiguous(), cnt

    st = dec.stream(B, sg.T_CAP)
    f, states, _ = _drive(st, steps(), psis, NO_CAP, fg.T, dev)
    assert f.max() >= 150
    for b in range(B):
        assert np.array_equal(states[b, :f[b]].cpu().numpy(), ref_s[b, :f[b]])
    st.close()


def test_reset_and_reuse(golden, dev):
    """Test 5: commit, reset(), other emissions, commit: the frontiers start from 0 again."""
    A, pi = _params(golden, "tonet361")
    dec = _decoder(golden, dev, "tonet361")
    st = dec.stream(2, T)
    for seed, gen in ((21, synth.emissions_dense), (22, synth.emissions_peaks)):
        E = gen(2, T, dec.S, seed=seed, device=dev)
        En = E.cpu().numpy()
        psis = [cr.back_pointers(A, pi, En[b]) for b in range(2)]
        st.reset()
        f, states, log = _drive(st, _uniform(E, [64, 64, 75]), psis, NO_CAP, T, dev)
        assert log[0][2] == 0 and log[1][2] == 0 and f.min() >= 150
    # the Python layer's own bookkeeping: commit() returns the fresh slices, reset() starts them over
    st.reset()
    st.append(E[:, :100].contiguous())
    lens1, fresh1 = st.commit(out_dtype=torch.int32)
    st.append(E[:, 100:].contiguous())
    lens2, fresh2 = st.commit(out_dtype=torch.int32)
    ds, _ = dec.decode(E, out_dtype=torch.int32)
    for b in range(2):
        assert 0 < lens1[b] <= lens2[b] and fresh1[b].numel() == lens1[b] and fresh2[b].numel() == lens2[b] - lens1[b]
        assert torch.equal(torch.cat([fresh1[b], fresh2[b]]), ds[b, :lens2[b]])
        assert torch.equal(st.committed_states[b, :lens2[b]], ds[b, :lens2[b]])
    st.close()


@pytest.mark.parametrize("name", ["tonet361", "imm722w"])
def test_buffers_and_second_session(golden, dev, name):
    """Test 6: states, committed and the commit state of exactly the asked size between guards over poisoned memory; a second
    session of the same plan on a second stream commits independently."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    lib = _lib.load()
    B, stride = 2, T + 9
    E = [synth.emissions_peaks(B, T, dec.S, seed=14 + k, device=dev) for k in range(2)]
    psis = [[cr.back_pointers(A, pi, e.cpu().numpy()[b]) for b in range(B)] for e in E]
    need = int(lib.vit_workspace_bytes_stream_commit(dec._plan, B))
    assert need > 0
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    sess = [dec.stream(B, T) for _ in range(2)]
    arenas = []
    for k in range(2):
        s_ar = guarded.Arena(B * stride * 4, dev, fill=0xB3)
        c_ar = guarded.Arena(B * 8, dev, fill=0xB3)
        w_ar = guarded.Arena(need, dev)
        assert lib.vit_stream_commit_begin(sess[k]._handle(), w_ar.ptr, need - 1) == -4
        assert lib.vit_stream_commit_begin(sess[k]._handle(), w_ar.ptr + 64, need) == -1
        assert lib.vit_stream_commit_begin(sess[k]._handle(), w_ar.ptr, need) == 0
        arenas.append((s_ar, c_ar, w_ar))
    poison = int(np.frombuffer(bytes([0xB3] * 4), np.int32)[0])
    f = [np.zeros(B, np.int64) for _ in range(2)]
    exp = [np.full((B, stride), poison, np.int32) for _ in range(2)]
    t = 0
    for n in (50, 80, 73):
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                sess[k].append(E[k][:, t:t + n].contiguous())
                rc = lib.vit_stream_commit(sess[k]._handle(), arenas[k][0].ptr, stride, arenas[k][1].ptr, NO_CAP, streams[k].cuda_stream)
                assert rc == 0
        torch.cuda.synchronize()
        t += n
        for k in range(2):
            s_ar, c_ar, w_ar = arenas[k]
            got_f = c_ar.view(torch.int64, (B,)).cpu().numpy()
            for b in range(B):
                f2, s = cr.commit(psis[k][b], t, f[k][b], NO_CAP)
                exp[k][b, f[k][b]:f2] = s
                f[k][b] = f2
            assert np.array_equal(got_f, f[k]), (k, t)
            assert np.array_equal(s_ar.view(torch.int32, (B, stride)).cpu().numpy(), exp[k]), (k, t)
            for ar, what in zip(arenas[k], ("states", "committed", "commit state")):
                guarded.assert_intact(ar, what)
    assert min(x.min() for x in f) >= 190
    for s in sess:
        s.close()


def test_refusals_write_nothing(golden, dev):
    """Test 7: max_lookback = 0 (and above 2^30), a stride below the lengths, a commit before commit_begin, NULL outputs; a
    durrieu722 session has no commit point.  Nothing is enqueued: outputs and commit state keep their poison."""
    dec = _decoder(golden, dev, "tonet361")
    lib = _lib.load()
    E = synth.emissions_peaks(2, T, dec.S, seed=2, device=dev)
    st = dec.stream(2, T)
    st.append(E[:, :150].contiguous())
    stream = torch.cuda.current_stream(dev).cuda_stream
    states = torch.full((2, T), POISON, dtype=torch.int32, device=dev)
    committed = torch.full((2,), -9, dtype=torch.int64, device=dev)
    need = int(lib.vit_workspace_bytes_stream_commit(dec._plan, 2))
    cws = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device=dev)
    ptr = (cws.data_ptr() + 255) & ~255
    h = st._handle()
    assert lib.vit_stream_commit(h, states.data_ptr(), T, committed.data_ptr(), 8, stream) == -1          # no commit_begin yet
    assert lib.vit_stream_commit_begin(h, None, need) == -1
    assert lib.vit_stream_commit_begin(h, ptr, need) == 0
    assert lib.vit_stream_commit(h, states.data_ptr(), T, committed.data_ptr(), 0, stream) == -1
    assert lib.vit_stream_commit(h, states.data_ptr(), T, committed.data_ptr(), (1 << 30) + 1, stream) == -1
    assert lib.vit_stream_commit(h, states.data_ptr(), 149, committed.data_ptr(), 8, stream) == -1
    assert lib.vit_stream_commit(h, None, T, committed.data_ptr(), 8, stream) == -1
    assert lib.vit_stream_commit(h, states.data_ptr(), T, None, 8, stream) == -1
    torch.cuda.synchronize()
    assert (states == POISON).all() and (committed == -9).all() and (cws == 0x5A).all()
    with pytest.raises(ValueError):
        st.commit_into(states.to(torch.int64), committed)
    with pytest.raises(ValueError):
        st.commit_into(states, committed.to(torch.int32))
    st.close()
    dur = _decoder(golden, dev, "durrieu722")
    assert int(lib.vit_workspace_bytes_stream_commit(dur._plan, 2)) == 0
    sd = dur.stream(2, T)
    assert lib.vit_stream_commit_begin(sd._handle(), ptr, need) == -5
    assert lib.vit_stream_commit(sd._handle(), states.data_ptr(), T, committed.data_ptr(), 8, stream) == -1
    with pytest.raises(_lib.ViterbiHipError):
        sd.commit()
    torch.cuda.synchronize()
    assert (states == POISON).all() and (committed == -9).all() and (cws == 0x5A).all()
    sd.close()


@pytest.mark.parametrize("cls", ["Viterbi", "SoftMaxViterbi", "ScaledSoftMaxViterbi"])
def test_recording_accumulator_partial(dev, cls):
    """Test 8: a recording of 3 x 768 frames: partial() after each append is a prefix of finish(), n_final never decreases."""
    from viterbi_spl_amd import reference_api as ra
    U = 360
    Atr, p0 = synth.tonet_transition(U, 14), synth.floored_prior(U + 1)
    if cls == "Viterbi":
        vit = ra.Viterbi(Atr, p0, device=dev)
    elif cls == "SoftMaxViterbi":
        vit = ra.SoftMaxViterbi(Atr, p0, device=dev)
    else:
        vit = ra.ScaledSoftMaxViterbi(Atr, p0, 0.5, True, device=dev)
    note_range = torch.linspace(30.0, 90.0, U, device=dev)
    acc = ra.RecordingAccumulator(vit, 3 * 768, streaming=True)
    with pytest.raises(ValueError):
        ra.RecordingAccumulator(vit, 16, streaming=False).partial()
    for rec in range(2):                                    # (the second recording: finish() resets the frontier)
        g = torch.Generator(device="cpu").manual_seed(300 + rec)
        parts, last = [], 0
        for _ in range(3):
            acc.append((torch.randn((24, acc.channels, 32), generator=g) * 3.0).to(dev))
            n_final, voiced, bins, notes = acc.partial(note_range)
            assert last <= n_final < acc.n_frames and voiced.shape[0] == bins.shape[0] == notes.shape[0] == n_final
            parts.append((n_final, voiced.clone(), bins.clone(), notes.clone()))
            last = n_final
        assert parts[0][0] > 0 and last > 2 * 768
        fv, fb, fn = acc.finish(note_range)
        assert fv.shape[0] == 3 * 768
        for n_final, voiced, bins, notes in parts:
            assert torch.equal(voiced, fv[:n_final]) and torch.equal(bins, fb[:n_final]) and torch.equal(notes, fn[:n_final])
