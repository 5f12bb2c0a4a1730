"""The issue slots taken out of the split-window floor forward kernel (forward_form 6) must not change a bit: the extra
column that leaves the frame maximum M by the ADDRESS of its publishing lane (one extra column, state S - 1, (S - 1) % 4 == 0:
its whole quad is otherwise idle) instead of by a select, the emission prefetch whose wait is folded into the last window
wait, and the merged waits of the late window quads.  Every case is checked against the CPU oracle and against the
one-target kernel (forward_form 1), and the raw history rows [B, T, SD] are compared byte for byte after zeroing the
workspace: pad column S holds M, so an extra column that leaked into the frame maximum, or a live state that dropped out
of it, shows there directly.  Which instantiation the launcher picked is asserted through those bytes only."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests.test_plan_host import _banded_matrix
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _history(dec, E, lens, form):
    """The history rows [B, T, SD] the forward kernel `form` leaves (workspace zeroed first)."""
    B, T, S = E.shape
    st = torch.empty((B, T), dtype=torch.int32, device=E.device)
    ll = torch.empty((B,), dtype=torch.float32, device=E.device)
    dec.set_option("forward_form", form)
    dec.decode_into(E, st, ll, lengths=lens, algo="group", phase="forward")      # allocates the workspace
    torch.cuda.synchronize()
    dec._ws.zero_()
    dec.decode_into(E, st, ll, lengths=lens, algo="group", phase="forward")
    torch.cuda.synchronize()
    dec.set_option("reset", 0)
    SD = (S + 5) // 4 * 4
    pad = (-dec._ws.data_ptr()) % 256
    return dec._ws[pad:pad + B * T * SD * 4].view(torch.int32).view(B, T, SD).cpu().numpy().copy()


def _check(dec, A, pi, E, lens, tag):
    """forward_form 6 against the oracle and against form 1: paths, log-likelihood bits, history bytes."""
    assert dec.info["floor_ok"] and dec.info["group_window"] == 32 and dec.info["n_dense_rows"] == 0, (tag, dec.info)
    ref_s, ref_l = vo.decode_c(A, pi, E.cpu().numpy(), lengths=None if lens is None else lens.cpu().numpy())
    out = {}
    for form in (6, 1):
        dec.set_option("forward_form", form)
        st, ll = dec.decode(E, lengths=lens, algo="group", out_dtype=torch.int32)
        dec.set_option("reset", 0)
        st, ll = st.cpu().numpy(), ll.cpu().numpy()
        assert np.array_equal(st, ref_s), (tag, form)
        assert np.array_equal(_bits(ll), _bits(ref_l)), (tag, form, ll, ref_l)
        out[form] = (st, ll)
    assert np.array_equal(out[6][0], out[1][0]) and np.array_equal(_bits(out[6][1]), _bits(out[1][1])), tag
    h6, h1 = _history(dec, E, lens, 6), _history(dec, E, lens, 1)
    assert np.array_equal(h6, h1), (tag, "history rows differ", np.argwhere(h6 != h1)[:8])


def _shipped(S):
    return synth.log_params(synth.tonet_transition(S - 1, 14 if S == 361 else 12), synth.floored_prior(S))


# (name, S, extra column, True: shipped tonet matrix); the last two must keep the select
MATRICES = [("tonet361", 361, 360, True), ("tonet321", 321, 320, True), ("S257", 257, 256, False), ("S357", 357, 356, False),
            ("S383", 383, 382, False), ("S300mid", 300, 148, False)]
_cache = {}


def _decoder(name, dev):
    """One decoder (and matrix) per case of MATRICES, shared by the parametrisations."""
    if name not in _cache:
        _, S, x, shipped = next(m for m in MATRICES if m[0] == name)
        if shipped:
            A, pi = _shipped(S)
        else:
            rng = np.random.default_rng(S)
            A = _banded_matrix(S, int(rng.integers(9, 15)), rng, extras=[x], floor=-50.0, quant=2)
            pi = -(rng.integers(0, 8, S) / 2).astype(np.float32)
        dec = ViterbiDecoder(A, pi, dev)
        assert dec.info["extras"] == [x], (name, dec.info["extras"])
        _cache[name] = (A, pi, dec)
    return _cache[name]


@pytest.mark.parametrize("where", ["extra", "before", "zero"])
@pytest.mark.parametrize("name", [m[0] for m in MATRICES])
def test_extra_column_rule(dev, name, where):
    """On about 80 % of the frames the frame maximum is planted on the extra column x (must stay out of M) / on state x - 1
    (the last live state of the neighbouring quad; for S = 383 a live state of x's own quad: must stay in M) / on state 0."""
    _, S, x, _ = next(m for m in MATRICES if m[0] == name)
    A, pi, dec = _decoder(name, dev)
    col = {"extra": x, "before": x - 1, "zero": 0}[where]
    B, T = 6, 200
    rng = np.random.default_rng(11)
    E = synth.emissions_peaks(B, T, S, seed=9).cpu().numpy().copy()
    on = rng.random((B, T)) < 0.8
    E[:, :, col] = np.where(on, E.max(axis=2) + rng.integers(1, 40, (B, T)).astype(np.float32) / 4, E[:, :, col])
    E = torch.from_numpy(E.astype(np.float32)).to(dev)
    lens = torch.tensor([200, 199, 25, 13, 2, 1], dtype=torch.int64, device=dev)
    _check(dec, A, pi, E, lens, (name, where))


@pytest.mark.parametrize("S", [361, 321])
def test_wait_bound_every_tail(dev, S):
    """Real-valued emissions that differ in every frame (a prefetch register read before its load landed changes bits), every
    tail of the twelve-frame round ragged in one batch, and T = 12, 13, 24, 25 as the batch's own T."""
    A, pi, dec = _decoder("tonet%d" % S, dev)
    rng = np.random.default_rng(S)
    lengths = list(range(1, 14)) + [24, 25, 37]
    E = torch.from_numpy((3.0 * rng.standard_normal((len(lengths), 40, S))).astype(np.float32)).to(dev)
    _check(dec, A, pi, E, torch.tensor(lengths, dtype=torch.int64, device=dev), (S, "ragged"))
    for T in (12, 13, 24, 25):
        _check(dec, A, pi, E[:2, :T].contiguous(), None, (S, T))


def test_idle_slot_hygiene(dev):
    """A third of the emissions -inf (never a whole frame): the slots the redirected lane writes must never reach M."""
    S = 361
    rng = np.random.default_rng(17)
    A = _banded_matrix(S, int(rng.integers(9, 15)), rng, extras=[S - 1], floor=-50.0, quant=2)
    pi = -(rng.integers(0, 8, S) / 2).astype(np.float32)
    dec = ViterbiDecoder(A, pi, dev)
    assert dec.info["extras"] == [S - 1]
    B, T = 4, 60
    Ez = -(rng.integers(0, 6, (B, T, S)) / 2).astype(np.float32)
    Ez[rng.random((B, T, S)) < 0.33] = -np.inf
    Ez[:, :, 100] = -1.0
    Ez[:, :, 300] = -1.5
    E = torch.from_numpy(Ez).to(dev)
    lens = torch.tensor([T, 25, 13, 1], dtype=torch.int64, device=dev)
    _check(dec, A, pi, E, lens, "-inf emissions")
