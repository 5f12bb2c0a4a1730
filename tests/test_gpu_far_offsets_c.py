"""Construction C of tests/far_offsets.py on the GPU: ONE recording whose own frame offsets t * S and t * SD pass element 2^31 and
byte 2^32 (5.95 M frames of 361 float32 states, 2.97 M frames of 722 float16 states).  Stretches with a single live state, islands
of ordinary emissions at the first frames, around the row of every mark of every buffer, around the row a wrapped byte offset
would land in, and at the last frames; the expected path and score are chained island by island (tests/test_far_offsets_host.py
proves the chain equal to one oracle run at a scaled-down mark).  Bit for bit."""
import numpy as np
import pytest
import torch

from tests import f64_ref, far_offsets as fo
from tests.common import f32_bits
from viterbi_spl_amd import ViterbiDecoder, _lib

pytestmark = pytest.mark.gpu

CASES = [("tonet361", False, "peaks"), ("jdc722", True, "dense")]
IDS = ["tonet361-f32", "jdc722-f16"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


_EXPECTED = {}


def _case(golden, dev, name, f16, kind, f64=False):
    """-> (decoder, the construction (computed once per module and left unchanged), E [N, S] on the device)."""
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    S, isz = dec.S, 2 if f16 else 4
    key = (name, f16, f64)
    if key not in _EXPECTED:
        rows = fo.history_rows(_lib.load(), dec._plan)
        layouts = ("f64",) if f64 else ("group", "wave", "dense", "packed", "stream")
        buffers = [(S, isz)] + sorted({rows[k] for k in layouts if k in rows})
        _EXPECTED[key] = fo.recording_c(A, pi, f16, buffers, kind, seed=17 + f16, f64=f64), buffers
    c, buffers = _EXPECTED[key]
    widest = max(buffers[1:], key=lambda ri: ri[0] * ri[1])
    fo.need_free(c["N"] * (S * isz + widest[0] * widest[1] + 8))
    E = torch.empty((c["N"], S), dtype=torch.float16 if f16 else torch.float32, device=dev)
    fo.fill_recording(E, c["k"], c["v"], c["spans"], c["islands"])
    return dec, c, E


def _check(st, ll, c, what, bits=f32_bits):
    got = st.reshape(-1).cpu().numpy()
    bad = np.flatnonzero(got != c["states"])
    assert bad.size == 0, (what, "frames", bad[:8].tolist(), got[bad[:8]].tolist(), c["states"][bad[:8]].tolist(), c["spans"])
    assert bits(ll.reshape(-1).cpu().numpy())[0] == bits(c["loglik"]), (what, ll, c["loglik"])


def _tag(name, f16):
    return f"{name}/{'f16' if f16 else 'f32'}"


GROUP = [c + (btf,) for c in CASES for btf in (0, 2)] + [("durrieu722", True, "dense", 0)]     # (the step plans have one back-trace form)


@pytest.mark.parametrize("name,f16,kind,btf", GROUP, ids=[f"{n}-{'f16' if h else 'f32'}-{('sparse', '', 'rows')[b]}" for n, h, _, b in GROUP])
def test_decode_group(golden, dev, name, f16, kind, btf):
    """decode() with one workgroup walking the whole recording: the split floor kernel at 361 states (algo "group"), the 722-state
    workgroup kernel ("banded") and the step kernel of the Durrieu matrix ("auto"); the sparse and the whole-row back-trace."""
    dec, c, E = _case(golden, dev, name, f16, kind)
    algo = "group" if dec.info["wave_ok"] else "banded" if dec.info["banded_ok"] else "auto"
    assert dec.forward_family(1, algo) == ("group" if dec.info["banded_ok"] else "dense")
    dec.set_option("backtrace_form", btf)
    with fo.measured(f"c/decode_{algo}/bt{btf}/{_tag(name, f16)}", E.shape):
        st, ll = dec.decode(E, algo=algo, out_dtype=torch.int32)
    dec.set_option("reset", 0)
    _check(st, ll, c, (name, algo, btf))
    del dec, E, st, ll
    fo.release()


@pytest.mark.parametrize("hist", [1, 2], ids=["full", "half"])
def test_decode_wave(golden, dev, hist):
    """decode(algo="wave") of the 361-state recording: one wavefront walks it, with every history row (element 2^31 at frame 5.59 M of
    the 384-float rows) and with the rows of even frames only (byte 2^32 at frame 5.59 M; the back-trace rebuilds the odd ones from
    emission rows past the marks)."""
    name, f16, kind = CASES[0]
    dec, c, E = _case(golden, dev, name, f16, kind)
    dec.set_option("wave_history", hist)
    assert dec.history_mode(1, c["N"], "wave") == ("full", "half")[hist - 1]
    with fo.measured(f"c/decode_wave/{('full', 'half')[hist - 1]}/{_tag(name, f16)}", E.shape):
        st, ll = dec.decode(E, algo="wave", out_dtype=torch.int32)
    dec.set_option("reset", 0)
    _check(st, ll, c, (name, "wave", hist))
    del dec, E, st, ll
    fo.release()


@pytest.mark.parametrize("name,f16,kind", CASES, ids=IDS)
def test_decode_checkpointed(golden, dev, name, f16, kind):
    """decode_checkpointed with the default 1024-frame segments (5800 of them): far emission rows and far states.  Both passes walk
    the recording: the slowest call of these files (8 s at 361 states, where one wavefront runs it), at the shortest length that
    reaches the marks."""
    dec, c, E = _case(golden, dev, name, f16, kind)
    with fo.measured(f"c/decode_checkpointed/K1024/{_tag(name, f16)}", E.shape):
        st, ll = dec.decode_checkpointed(E, segment_frames=1024, out_dtype=torch.int32)
    _check(st, ll, c, (name, "checkpointed"))
    del dec, E, st, ll
    fo.release()


def test_decode_f64(golden, dev):
    """decode_f64 on the 361-state recording: rows of doubles, byte 2^32 at frame 1.47 M, element 2^31 at frame 5.9 M.  (One workgroup
    walks 2.5 us per frame at 722 states: that recording would take 7 s; constructions A and B cover the 722-state float64 kernels.)"""
    name, f16, kind = CASES[0]
    dec, c, E = _case(golden, dev, name, f16, kind, f64=True)
    with fo.measured(f"c/decode_f64/{_tag(name, f16)}", E.shape):
        st, ll = dec.decode_f64(E, out_dtype=torch.int32)
    _check(st, ll, c, (name, "f64"), f64_ref.bits64)
    del dec, E, st, ll
    fo.release()


@pytest.mark.parametrize("name,f16,kind", CASES, ids=IDS)
def test_linear_stream_session(golden, dev, name, f16, kind):
    """A linear session of one recording: two appends (the first runs past byte 2^32 of a float32 chunk, the second starts in a far
    row of the history), decode(), then commit(): with a single survivor on every stretch the frontier reaches the stretch in front
    of the last island, so the committed states cross every mark."""
    dec, c, E = _case(golden, dev, name, f16, kind)
    N = c["N"]
    with fo.measured(f"c/stream/{_tag(name, f16)}", E.shape):
        sess = dec.stream(1, max_frames=N)
        cut = N // 2 + 7
        sess.append(E[:cut])
        sess.append(E[cut:])
        assert sess.lengths.tolist() == [N]
        st, ll = sess.decode(out_dtype=torch.int32)
        _check(st, ll, c, (name, "stream decode"))
        done, fresh = sess.commit(out_dtype=torch.int32)
        assert N - 1 >= done[0] >= c["spans"][-1][0] - 8, (done, c["spans"][-1])
        assert np.array_equal(fresh[0].cpu().numpy(), c["states"][:done[0]]), (name, "committed states")
        sess.close()
    del dec, E, sess, st, ll, fresh
    fo.release()


@pytest.mark.parametrize("name,f16,kind", CASES, ids=IDS)
def test_decode_packed_between_short_ones(golden, dev, name, f16, kind):
    """decode_packed of three recordings: 301 frames, the long one, 257 frames -- the long one's rows start at a small offset, the
    last one's offset times the strides lies past every mark."""
    dec, c, E = _case(golden, dev, name, f16, kind)
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    N, S = c["N"], dec.S
    short = fo.live_songs("peaks", [301, 257], S, seed=23, f16=f16)
    ref_s, ref_l = fo.expected_a(A, pi, short, [301, 257])
    off = np.asarray([0, 301, 301 + N, 301 + N + 257], np.int64)
    Ep = torch.empty((int(off[-1]), S), dtype=E.dtype, device=dev)
    Ep[:301] = torch.from_numpy(short[0, :301]).to(dev)
    Ep[301:301 + N] = E
    Ep[301 + N:] = torch.from_numpy(short[1, :257]).to(dev)
    del E
    fo.release()
    with fo.measured(f"c/decode_packed/{_tag(name, f16)}", Ep.shape):
        st, ll = dec.decode_packed(Ep, off, out_dtype=torch.int32)
    got_l = f32_bits(ll.cpu().numpy())
    assert np.array_equal(st[:301].cpu().numpy(), ref_s[0, :301]) and got_l[0] == f32_bits(ref_l)[0]
    assert np.array_equal(st[301 + N:].cpu().numpy(), ref_s[1, :257]) and got_l[2] == f32_bits(ref_l)[1]
    _check(st[301:301 + N], ll[1:2], c, (name, "packed"))
    del dec, Ep, st, ll
    fo.release()
