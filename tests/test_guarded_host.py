"""CPU tier of tests/guarded.py: the harness must be able to fail.  Fake "decodes" written in NumPy over CPU arenas, one per defect
class tests/test_gpu_bounds.py is after -- each is flagged with the message that names the defect, and the correct fake passes.
Then the premises of poison_states on one oracle decode."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests import guarded as gd
from viterbi_spl_amd import synth

B, T, S = 3, 40, 97
LENS = np.asarray([40, 17, 1], np.int64)
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def oracle(golden):
    A, pi = golden["params"]["dense97_logA_T"], golden["params"]["dense97_log_pi"]
    out = {}
    for seed in (5, 6):
        E = synth.emissions_peaks(B, T, S, seed=seed).numpy()
        out[seed] = vo.decode_c(A, pi, E, lengths=LENS)
    return out


def _arenas(ref_s, kind="shifted", neighbour=None):
    st = gd.Arena(B * T * 4, CPU)
    ll = gd.Arena(B * 4, CPU)
    ws = gd.Arena(1000, CPU)
    st.store(gd.poison_states(ref_s, S, kind, neighbour))
    return st, ll, ws


def _fake_decode(st, ll, ws, ref_s, ref_l, defect=None):
    """Writes the oracle's result the way a decode does (path, -1 tail, log-likelihoods, scratch in the workspace), with one defect."""
    states = st.view(torch.int32, (B, T)).numpy()
    for b, n in enumerate(LENS):
        states[b, :n] = ref_s[b, :n]
        if defect != "tail":
            states[b, n:] = -1
    if defect == "last_frame":
        states[1, LENS[1] - 1] = gd.poison_states(ref_s, S, "shifted")[1, LENS[1] - 1]      # (what the buffer held: never written)
    ll.view(torch.float32, (B,)).numpy()[:] = ref_l
    ws.payload.numpy()[:] = 0
    if defect == "behind_states":
        st.buf.numpy()[st.offset + st.nbytes:st.offset + st.nbytes + 4] = np.frombuffer(np.int32(5).tobytes(), np.uint8)
    if defect == "front_of_workspace":
        ws.buf.numpy()[ws.offset - 1] = 0
    if defect == "loglik_B":
        ll.buf.numpy()[ll.offset + ll.nbytes:ll.offset + ll.nbytes + 4] = np.frombuffer(np.float32(-1.5).tobytes(), np.uint8)


def _check(st, ll, ws, ref_s, ref_l):
    gd.assert_decode_outputs(st, ll, ref_s, ref_l, LENS, T)
    gd.assert_intact(ws, "workspace")


def test_arena_layout():
    for lead, align in ((0, 256), (4, 256), (2, 256), (0, 64)):
        a = gd.Arena(1001, CPU, lead=lead, align=align)
        assert a.payload.numel() == 1001 and a.ptr == a.payload.data_ptr()
        assert (a.ptr - lead) % align == 0 and a.offset >= a.guard + lead
        assert a.buf.numel() - a.offset - a.nbytes >= a.guard
        assert a.poisoned() and a.intact() == (True, True, None)
    a = gd.Arena(24, CPU, lead=4)
    assert a.view(torch.float32, (2, 3)).is_contiguous() and a.view(torch.float32, (2, 3)).data_ptr() == a.ptr
    assert np.isnan(a.view(torch.float32, (6,)).numpy()).all() and np.isnan(a.view(torch.float16, (12,)).numpy()).all()
    assert (a.view(torch.int32, (6,)).numpy() == -1).all()
    # every byte outside the payload is watched: the lead, the pads, both guards
    for where in ("lead", "pad", "first", "behind", "last"):
        a = gd.Arena(24, CPU, lead=4)
        off = {"lead": -1, "pad": -5, "first": -a.offset, "behind": a.nbytes, "last": a.buf.numel() - a.offset - 1}[where]
        a.buf[a.offset + off] = 0
        front_ok, back_ok, first = a.intact()
        assert (front_ok, back_ok, first) == (off >= 0, off < 0, off), off
    a = gd.Arena(24, CPU, lead=4)
    a.payload[:] = 0                                        # the payload itself is the caller's
    assert a.intact() == (True, True, None) and not a.poisoned()


def test_a_correct_decode_passes(oracle):
    ref_s, ref_l = oracle[5]
    for kind, nb in (("sentinel", None), ("shifted", None), ("neighbour", oracle[6][0])):
        st, ll, ws = _arenas(ref_s, kind, nb)
        _fake_decode(st, ll, ws, ref_s, ref_l)
        _check(st, ll, ws, ref_s, ref_l)


@pytest.mark.parametrize("defect, message", [
    ("behind_states", r"states: bytes behind the buffer were written \(first at offset 480,"),
    ("front_of_workspace", r"workspace: bytes in front of the buffer were written \(first at offset -1 "),
    ("last_frame", r"states differ from the oracle at song 1, frame 16 \(of 17\)"),
    ("tail", r"states past the end of song 1 \(17 frames\) are not -1: frame 17 holds"),
    ("loglik_B", r"loglik: bytes behind the buffer were written \(first at offset 12,"),
])
def test_every_defect_is_flagged(oracle, defect, message):
    ref_s, ref_l = oracle[5]
    st, ll, ws = _arenas(ref_s)
    _fake_decode(st, ll, ws, ref_s, ref_l, defect)
    with pytest.raises(AssertionError, match=message):
        _check(st, ll, ws, ref_s, ref_l)


def test_a_wrong_loglik_is_flagged_by_bits(oracle):
    ref_s, ref_l = oracle[5]
    st, ll, ws = _arenas(ref_s)
    _fake_decode(st, ll, ws, ref_s, ref_l)
    v = ll.view(torch.int32, (B,))
    v[2] += 1                                               # one ulp
    with pytest.raises(AssertionError, match="loglik differs from the oracle at song 2"):
        _check(st, ll, ws, ref_s, ref_l)
    st, ll, ws = _arenas(ref_s)                             # never written: the fill reads as NaN
    _fake_decode(st, ll, ws, ref_s, ref_l)
    ll.payload[:] = gd.FILL
    with pytest.raises(AssertionError, match="loglik differs from the oracle at song 0"):
        _check(st, ll, ws, ref_s, ref_l)


def test_packed_outputs(oracle):
    ref_s, ref_l = oracle[5]
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    N = int(off[-1])
    packed = np.concatenate([ref_s[b, :n] for b, n in enumerate(LENS)]).astype(np.int32)
    for defect in (None, "first_frame"):
        st, ll = gd.Arena(N * 4, CPU), gd.Arena(B * 4, CPU)
        st.store(packed)
        ll.store(np.asarray(ref_l, np.float32))
        if defect:
            st.view(torch.int32, (N,))[off[1]] = gd.SENTINEL
            with pytest.raises(AssertionError, match=r"states differ from the oracle at song 1, frame 0 \(of 17\): got -7"):
                gd.assert_decode_outputs(st, ll, ref_s, ref_l, LENS, T, offsets=off)
        else:
            gd.assert_decode_outputs(st, ll, ref_s, ref_l, LENS, T, offsets=off)


def test_poison_premises(oracle):
    ref_s, _ = oracle[5]
    nb_s, _ = oracle[6]
    sent = gd.poison_states(ref_s, S, "sentinel")
    assert sent.dtype == np.int32 and sent.shape == ref_s.shape and np.all(sent == gd.SENTINEL)
    sh = gd.poison_states(ref_s, S, "shifted")
    assert sh.dtype == np.int32 and np.all(sh != ref_s) and np.all((sh >= 0) & (sh < S))
    nb = gd.poison_states(ref_s, S, "neighbour", nb_s)
    for b, n in enumerate(LENS):
        assert np.array_equal(nb[b, :n], nb_s[b, :n]) and np.all(nb[b, n:] == gd.SENTINEL)
        if n > 8:
            assert 2 * int(np.sum(nb[b, :n] != ref_s[b, :n])) >= n
    # the premises are asserted, not assumed: the reference's own path is no neighbour of itself
    with pytest.raises(AssertionError, match="differs from the reference in only 0 of 40 frames"):
        gd.poison_states(ref_s, S, "neighbour", ref_s)
    with pytest.raises(AssertionError, match="not one of the same songs"):
        gd.poison_states(ref_s, S, "neighbour", np.roll(nb_s, 1, axis=0))
