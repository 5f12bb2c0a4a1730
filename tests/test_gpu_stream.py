"""GPU tests of the streaming decode (vit_stream_*, ViterbiDecoder.stream, RecordingAccumulator(streaming=True)): whatever the
chunking, the states and the log-likelihood of ``decode`` on the same frames and of the CPU oracle, bit for bit; the history rows of
``vit_forward``; refusals that write nothing.  Every other (window width, target waves) pair, the edges of the step range, launch
boundaries on forced hops and the chunked back-trace forms of a session: tests/test_gpu_stream_grid.py."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests import common
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

PLANS = ["tonet361", "msnet321", "jdc722", "imm722w", "durrieu722"]
T = 203
POISON = -77


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


def _chunkings(T, every_frame):
    out = [[T], [1] * 9 + [2, 3, 4, 5, 7, 8], [63, 64, 65]]
    if every_frame:
        out.append([1] * T)
    for c in out:
        if sum(c) < T:
            c.append(T - sum(c))
        assert sum(c) == T and min(c) >= 1
    return out


def _feed(st, E, chunks):
    t = 0
    for n in chunks:
        st.append(E[:, t:t + n].contiguous())
        t += n


def _bits(x):
    return x.detach().cpu().numpy().view(np.int32)


@pytest.mark.parametrize("name", PLANS)
def test_any_chunking_same_bits(golden, dev, name):
    """Test 1: one chunk; 9 x 1 frame then 2, 3, 4, 5, 7, 8 and the rest (below, at and above the prefetch depths 2, 4 and 12, every
    remainder of the unrolled loops); 63 / 64 / 65 / rest; for the 361-state plan also T chunks of one frame.  Every chunking with
    peak-like and dense emissions, float32 and float16."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    for kind, gen in (("peaks", synth.emissions_peaks), ("dense", synth.emissions_dense)):
        for dt in (torch.float32, torch.float16):
            E = gen(2, T, dec.S, seed=21, device=dev, dtype=dt)
            ref_s, ref_l = vo.decode_c(A, pi, E.float().cpu().numpy())
            ds, dl = dec.decode(E, out_dtype=torch.int32)
            assert np.array_equal(ds.cpu().numpy(), ref_s) and np.array_equal(dl.cpu().numpy(), ref_l)
            st = dec.stream(2, T)
            for chunks in _chunkings(T, name == "tonet361"):
                st.reset()
                _feed(st, E, chunks)
                assert st.lengths.tolist() == [T, T]
                s, l = st.decode(out_dtype=torch.int32)
                assert torch.equal(s, ds), (name, kind, dt, chunks[:4])
                assert np.array_equal(_bits(l), _bits(dl)), (name, kind, dt, chunks[:4])
            st.close()


@pytest.mark.parametrize("name", PLANS)
def test_ragged_counts(golden, dev, name):
    """Test 2: final lengths 1, 130, 203 through shared [3, n, S] chunks; counts with zeros; one song stops early, the one-frame song
    never sees a second frame.  A back-trace while a song is at length 0 is VIT_EINVAL and leaves the poisoned outputs alone."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    lens = np.array([1, 130, 203], np.int64)
    st = dec.stream(3, T)
    for gen, dt in ((synth.emissions_peaks, torch.float32), (synth.emissions_dense, torch.float32),
                    (synth.emissions_peaks, torch.float16), (synth.emissions_dense, torch.float16)):
        E = gen(3, T, dec.S, seed=5, device=dev, dtype=dt)
        ref_s, ref_l = vo.decode_c(A, pi, E.float().cpu().numpy(), lengths=lens)
        ds, dl = dec.decode(E, lengths=torch.from_numpy(lens).to(dev), out_dtype=torch.int32)
        st.reset()
        pos = np.zeros(3, np.int64)
        plan = [(0, 0, 40), (1, 30, 40), (0, 33, 33), (0, 67, 67), (0, 0, 23)]     # counts per append; song 0 starts late, song 1 ends early
        states = torch.full((3, T), POISON, dtype=torch.int32, device=dev)
        ll = torch.full((3,), 7.0, device=dev)
        for k, cnt in enumerate(plan):
            cnt = np.asarray(cnt, np.int64)
            n = int(cnt.max())
            buf = torch.full((3, n, dec.S), float("nan"), device=dev, dtype=dt)
            for b in range(3):
                buf[b, :cnt[b]] = E[b, pos[b]:pos[b] + cnt[b]]
            st.append(buf, counts=cnt)
            pos += cnt
            if k == 0:
                with pytest.raises(_lib.ViterbiHipError, match="invalid argument"):
                    st.decode_into(states, ll)
                torch.cuda.synchronize()
                assert (states == POISON).all() and (ll == 7.0).all()
        assert np.array_equal(pos, lens) and np.array_equal(st.lengths, lens)
        s, l = st.decode(out_dtype=torch.int32)
        assert np.array_equal(s.cpu().numpy(), ref_s) and np.array_equal(l.cpu().numpy(), ref_l), dt
        assert torch.equal(s, ds) and np.array_equal(_bits(l), _bits(dl)), dt
    st.close()


@pytest.mark.parametrize("name", ["tonet361", "durrieu722"])
def test_one_recording_and_uneven_positions(golden, dev, name):
    """The [n, S] form of ``append`` on a one-recording session; and ``counts=None`` on a session whose recordings stand at different
    positions (n frames for every recording, through the per-launch tables), float16."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    E = synth.emissions_dense(2, T, dec.S, seed=17, device=dev, dtype=torch.float16)
    ds, dl = dec.decode(E[:1].contiguous(), out_dtype=torch.int32)
    st = dec.stream(1, T)
    t = 0
    for n in (1, 12, 13, 77, T - 103):
        st.append(E[0, t:t + n].contiguous())
        t += n
    s, l = st.decode(out_dtype=torch.int32)
    assert torch.equal(s, ds) and np.array_equal(_bits(l), _bits(dl))
    st.close()
    lens = np.array([150, 120], np.int64)
    ref_s, ref_l = vo.decode_c(A, pi, E.float().cpu().numpy(), lengths=lens)
    st = dec.stream(2, T)
    first = torch.zeros((2, 50, dec.S), device=dev, dtype=torch.float16)
    first[0], first[1, :20] = E[0, :50], E[1, :20]
    st.append(first, counts=[50, 20])
    st.append(torch.stack([E[0, 50:150], E[1, 20:120]]).contiguous())         # counts=None: 100 frames each, from positions 50 and 20
    assert st.lengths.tolist() == [150, 120]
    s, l = st.decode(out_dtype=torch.int32)
    assert np.array_equal(s.cpu().numpy(), ref_s[:, :150]) and np.array_equal(l.cpu().numpy(), ref_l)
    st.close()


@pytest.mark.parametrize("name", ["tonet361", "jdc722", "durrieu722"])
def test_same_history(golden, dev, name):
    """Test 3: the session's rows against vit_forward (forward_form 1: one target per lane) on the whole tensor: columns [0, S) of
    every row and, for the banded plans, pad column S of rows 0 .. T - 2, as bytes."""
    dec = ViterbiDecoder(*_params(golden, name), dev)
    S, SD = dec.S, (dec.S + 5) // 4 * 4
    for gen, dt in ((synth.emissions_peaks, torch.float32), (synth.emissions_dense, torch.float16)):
        E = gen(2, T, S, seed=33, device=dev, dtype=dt)
        if name != "durrieu722":
            dec.set_option("forward_form", 1)
        states = torch.empty((2, T), dtype=torch.int32, device=dev)
        dec.decode_into(E, states, algo="auto" if name == "durrieu722" else "group", phase="forward", slot=3)
        torch.cuda.synchronize()
        ws = dec._ws_slots[3]
        off = ((ws.data_ptr() + 255) & ~255) - ws.data_ptr()
        ref = ws[off:off + 2 * T * SD * 4].view(torch.int32).view(2, T, SD).clone()
        dec.set_option("reset", 0)
        need = dec.workspace_bytes_stream(2, T)
        buf = torch.zeros(need + 256, dtype=torch.uint8, device=dev)
        st = dec.stream(2, T, workspace=buf)
        _feed(st, E, [1, 2, 5, 64, 13, T - 85])
        torch.cuda.synchronize()
        o2 = ((buf.data_ptr() + 255) & ~255) - buf.data_ptr()
        got = buf[o2:o2 + 2 * T * SD * 4].view(torch.int32).view(2, T, SD)
        assert torch.equal(got[:, :, :S], ref[:, :, :S]), dt
        if name != "durrieu722":
            assert torch.equal(got[:, :T - 1, S], ref[:, :T - 1, S]), dt
        st.close()


@pytest.mark.parametrize("name", PLANS)
def test_backtrace_is_not_final(golden, dev, name):
    """Test 4: decode after 100 frames = decode of the first 100 frames; append the rest, decode again = the whole."""
    dec = _decoder(golden, dev, name)
    E = synth.emissions_dense(2, T, dec.S, seed=8, device=dev, dtype=torch.float16)
    st = dec.stream(2, T)
    st.append(E[:, :100].contiguous())
    s, l = st.decode(out_dtype=torch.int32)
    ds, dl = dec.decode(E[:, :100].contiguous(), out_dtype=torch.int32)
    assert torch.equal(s, ds) and np.array_equal(_bits(l), _bits(dl))
    st.append(E[:, 100:].contiguous())
    s, l = st.decode(out_dtype=torch.int32)
    ds, dl = dec.decode(E, out_dtype=torch.int32)
    assert torch.equal(s, ds) and np.array_equal(_bits(l), _bits(dl))
    st.close()


@pytest.mark.parametrize("name", ["tonet361", "jdc722", "durrieu722"])
def test_edge_values(golden, dev, name):
    """Test 5: -inf entries, a whole -inf stretch across a chunk boundary and songs that die (the dead_frame class of the value-edge
    tests, plus frames 62 .. 66 of song 1 all -inf with chunk boundaries at 63, 64 and 65): the result of ``decode``."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    rng = np.random.default_rng(3)
    En = common.dead_frame(rng, 4, T, dec.S, {0: 64, 2: 0})
    En[1, 62:67, :] = -np.inf
    E = torch.from_numpy(En).to(dev)
    ref_s, ref_l = vo.decode_c(A, pi, En)
    assert common.f32_bits(ref_l)[0] == common.NINF_BITS and np.isfinite(ref_l[3])
    ds, dl = dec.decode(E, out_dtype=torch.int32)
    st = dec.stream(4, T)
    _feed(st, E, [63, 1, 1, 1, T - 66])
    s, l = st.decode(out_dtype=torch.int32)
    assert torch.equal(s, ds) and np.array_equal(_bits(l), _bits(dl))
    assert np.array_equal(s.cpu().numpy(), ref_s) and np.array_equal(common.f32_bits(l.cpu().numpy()), common.f32_bits(ref_l))
    st.close()


@pytest.mark.parametrize("name", ["tonet361", "imm722w", "durrieu722"])
def test_buffers(golden, dev, name):
    """Test 6: a workspace of exactly the asked size, NaN-filled, between guards; poisoned states and loglik between guards; chunk
    tensors at odd element offsets of a larger buffer; states_stride > the longest length."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    lib = _lib.load()
    B, S, G = 2, dec.S, 4096
    lens = np.array([150, T], np.int64)
    E = synth.emissions_peaks(B, T, S, seed=14, device=dev)
    ref_s, ref_l = vo.decode_c(A, pi, E.cpu().numpy(), lengths=lens)
    need = dec.workspace_bytes_stream(B, T)
    raw = torch.full((need + 2 * G + 256,), 0xA5, dtype=torch.uint8, device=dev)
    base = ((raw.data_ptr() + G + 255) & ~255) - raw.data_ptr()
    raw[base:base + need].view(torch.float32).fill_(float("nan"))
    stride = T + 9
    sraw = torch.full((G + B * stride + G,), POISON, dtype=torch.int32, device=dev)
    lraw = torch.full((64 + B + 64,), -5.0, device=dev)
    sess = ctypes.c_void_p()
    stream = torch.cuda.current_stream(dev).cuda_stream
    assert lib.vit_stream_open(dec._plan, B, T, raw.data_ptr() + base, need - 1, ctypes.byref(sess)) == -4
    assert lib.vit_stream_open(dec._plan, B, T, raw.data_ptr() + base, need, ctypes.byref(sess)) == 0
    big = torch.full((3 + B * 80 * S + 8,), float("nan"), device=dev)
    pos = np.zeros(B, np.int64)
    while (pos < lens).any():
        cnt = np.minimum(lens - pos, [50, 80])
        n = int(cnt.max())
        chunk = big[3:3 + B * n * S].view(B, n, S)
        assert (chunk.data_ptr() - big.data_ptr()) // 4 == 3
        for b in range(B):
            chunk[b, :cnt[b]] = E[b, pos[b]:pos[b] + cnt[b]]
        assert lib.vit_stream_append(sess, chunk.data_ptr(), 0, n, cnt.ctypes.data, stream) == 0
        torch.cuda.synchronize()
        big.fill_(float("nan"))                                   # the chunk is the caller's again once the kernel has run
        pos += cnt
    states = sraw[G:G + B * stride].view(B, stride)
    assert lib.vit_stream_backtrace(sess, states.data_ptr(), stride, lraw[64:].data_ptr(), stream) == 0
    torch.cuda.synchronize()
    lib.vit_stream_close(sess)
    got = states.cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b, :lens[b]], ref_s[b, :lens[b]]) and (got[b, lens[b]:] == -1).all()
    assert np.array_equal(lraw[64:64 + B].cpu().numpy(), ref_l)
    assert (sraw[:G] == POISON).all() and (sraw[G + B * stride:] == POISON).all()
    assert (lraw[:64] == -5.0).all() and (lraw[64 + B:] == -5.0).all()
    assert (raw[:base] == 0xA5).all() and (raw[base + need:] == 0xA5).all()


def test_refusals_write_nothing(golden, dev):
    """Test 7: append past T_cap (a following legal append still decodes right), counts[b] > n, n = 0, a dtype switch, a misaligned
    workspace, states_stride too small, unsupported plans."""
    A, pi = _params(golden, "tonet361")
    dec = _decoder(golden, dev, "tonet361")
    lib = _lib.load()
    S = dec.S
    E = synth.emissions_peaks(2, T, S, seed=2, device=dev)
    ds, dl = dec.decode(E, out_dtype=torch.int32)
    need = dec.workspace_bytes_stream(2, T)
    ws = torch.empty(need + 512, dtype=torch.uint8, device=dev)
    ptr = (ws.data_ptr() + 255) & ~255
    sess = ctypes.c_void_p()
    assert lib.vit_stream_open(dec._plan, 2, T, ptr + 16, need, ctypes.byref(sess)) == -1 and not sess.value
    assert lib.vit_stream_open(dec._plan, 2, T, ptr, need, ctypes.byref(sess)) == 0
    stream = torch.cuda.current_stream(dev).cuda_stream
    head = E[:, :150].contiguous()
    assert lib.vit_stream_append(sess, head.data_ptr(), 0, 150, None, stream) == 0
    torch.cuda.synchronize()
    snap = ws.clone()
    tail = E[:, 150:].contiguous()
    over = torch.zeros((2, 54, S), device=dev)
    bad = np.array([54, 10], np.int64)
    assert lib.vit_stream_append(sess, over.data_ptr(), 0, 54, None, stream) == -1                 # 150 + 54 > T_cap
    assert lib.vit_stream_append(sess, over.data_ptr(), 0, 54, bad.ctypes.data, stream) == -1      # ... for one song
    assert lib.vit_stream_append(sess, over.data_ptr(), 0, 5, bad.ctypes.data, stream) == -1       # counts[b] > n
    assert lib.vit_stream_append(sess, over.data_ptr(), 0, 5, np.array([-1, 2], np.int64).ctypes.data, stream) == -1
    assert lib.vit_stream_append(sess, over.data_ptr(), 0, 0, None, stream) == -1                  # n = 0
    assert lib.vit_stream_append(sess, over.data_ptr(), 1, 5, None, stream) == -1                  # float16 after float32
    assert lib.vit_stream_append(sess, over.data_ptr(), 2, 5, None, stream) == -1
    states = torch.full((2, T), POISON, dtype=torch.int32, device=dev)
    assert lib.vit_stream_backtrace(sess, states.data_ptr(), 149, None, stream) == -1              # stride below the lengths
    torch.cuda.synchronize()
    assert torch.equal(ws, snap) and (states == POISON).all()
    ln = np.zeros(2, np.int64)
    assert lib.vit_stream_lengths(sess, ln.ctypes.data) == 0 and ln.tolist() == [150, 150]
    assert lib.vit_stream_append(sess, tail.data_ptr(), 0, T - 150, None, stream) == 0
    ll = torch.empty(2, device=dev)
    assert lib.vit_stream_backtrace(sess, states.data_ptr(), T, ll.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(states, ds) and np.array_equal(_bits(ll), _bits(dl))
    lib.vit_stream_close(sess)
    for name in ("dense361", "dense97"):
        d2 = ViterbiDecoder(*_params(golden, name), dev)
        assert d2.workspace_bytes_stream(2, T) == 0
        assert lib.vit_stream_open(d2._plan, 2, T, ptr, need, ctypes.byref(sess)) == -5
        with pytest.raises(_lib.ViterbiHipError):
            d2.stream(2, T)


@pytest.mark.parametrize("name", ["tonet361", "jdc722"])
def test_two_sessions_two_streams(golden, dev, name):
    """Test 8: two sessions of one plan on two streams, ragged counts (so every append goes through the plan's one pinned staging
    buffer), appends interleaved from one thread: both equal the oracle."""
    A, pi = _params(golden, name)
    dec = _decoder(golden, dev, name)
    E = [synth.emissions_peaks(2, T, dec.S, seed=40 + k, device=dev) for k in range(2)]
    refs = [vo.decode_c(A, pi, e.cpu().numpy()) for e in E]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    sess = [dec.stream(2, T) for _ in range(2)]
    pos = [np.zeros(2, np.int64) for _ in range(2)]
    keep = []
    step = 0
    while any((p < T).any() for p in pos):
        for k in range(2):
            cnt = np.minimum(T - pos[k], [17 + 3 * k + step % 5, 29 - 2 * k])
            if cnt.max() == 0:
                continue
            n = int(cnt.max())
            with torch.cuda.stream(streams[k]):
                buf = torch.zeros((2, n, dec.S), device=dev)
                for b in range(2):
                    buf[b, :cnt[b]] = E[k][b, pos[k][b]:pos[k][b] + cnt[b]]
                sess[k].append(buf, counts=cnt)
            keep.append(buf)
            pos[k] += cnt
        step += 1
    out = []
    for k in range(2):
        with torch.cuda.stream(streams[k]):
            out.append(sess[k].decode(out_dtype=torch.int32))
    torch.cuda.synchronize()
    for k in range(2):
        assert np.array_equal(out[k][0].cpu().numpy(), refs[k][0]) and np.array_equal(out[k][1].cpu().numpy(), refs[k][1]), k
        sess[k].close()


@pytest.mark.parametrize("cls", ["Viterbi", "SoftMaxViterbi", "ScaledSoftMaxViterbi"])
def test_recording_accumulator_streaming(dev, cls):
    """Test 9: snippets with a padded last batch through RecordingAccumulator(streaming=True): the (voiced, bins, notes) of
    streaming=False exactly; reset() (inside finish) and a second recording."""
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
    accs = [ra.RecordingAccumulator(vit, 600, streaming=s) for s in (False, True)]
    F = 32
    for rec in range(2):
        g = torch.Generator(device="cpu").manual_seed(100 + rec)
        batches = [(6, 0), (6, 0), (4 + rec, 19)]                  # (snippets, padded frames): the last batch is padded
        outs = []
        for acc in accs:
            g.manual_seed(100 + rec)
            for n, pad in batches:
                x = (torch.randn((n, acc.channels, F), generator=g) * 3.0).to(dev)
                acc.append(x, pad)
            if acc.streaming:
                assert acc.logits().shape[0] == sum(n * F - pad for n, pad in batches)
            outs.append(acc.finish(note_range))
        for a, b in zip(*outs):
            assert torch.equal(a, b)
        assert outs[0][0].shape[0] == sum(n * F - pad for n, pad in batches)
