"""The split-window floor forward kernel (forward_form 6) whose full waves evaluate only the live window entries of their
targets ("floor_live_window" 0, the default) must not change a bit against the same kernel with the whole window
("floor_live_window" 1), against the one-target kernel (forward_form 1) and against the CPU oracle: paths, log-likelihood
bits and the raw history rows [B, T, SD] after zeroing the workspace (pad column S carries the frame maximum M).  The spike
emissions make the dropped candidates the row's true maximum, which fl(M + c_j) must then reproduce (the premise is checked on
the CPU in tests/test_floor_trim_host.py).  Which instantiation the launcher picked shows through those bytes only."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests.test_floor_trim_host import _s300mid, _tonet, _widths, spike_emissions
from tests.test_plan_host import _banded_matrix
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

LENGTHS = ([37, 25, 13, 2], [24, 12, 1])      # every tail of the twelve-frame round, in batches of at most six songs


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _run(dec, E, lens, form, whole):
    """(paths, log-likelihoods, history rows [B, T, SD]) of forward form `form` with "floor_live_window" = whole."""
    B, T, S = E.shape
    dec.set_option("forward_form", form)
    dec.set_option("floor_live_window", whole)
    st, ll = dec.decode(E, lengths=lens, algo="group", out_dtype=torch.int32)
    st2 = torch.empty((B, T), dtype=torch.int32, device=E.device)
    ll2 = torch.empty((B,), dtype=torch.float32, device=E.device)
    dec.decode_into(E, st2, ll2, lengths=lens, algo="group", phase="forward")      # allocates the workspace
    torch.cuda.synchronize()
    dec._ws.zero_()
    dec.decode_into(E, st2, ll2, lengths=lens, algo="group", phase="forward")
    torch.cuda.synchronize()
    dec.set_option("reset", 0)
    SD = (S + 5) // 4 * 4
    pad = (-dec._ws.data_ptr()) % 256
    hist = dec._ws[pad:pad + B * T * SD * 4].view(torch.int32).view(B, T, SD).cpu().numpy().copy()
    return st.cpu().numpy(), ll.cpu().numpy(), hist


def _check(dec, A, pi, E, lens, tag):
    assert dec.info["floor_ok"] and dec.info["group_window"] == 32 and dec.info["n_dense_rows"] == 0, (tag, dec.info)
    ref_s, ref_l = vo.decode_c(A, pi, E.cpu().numpy(), lengths=None if lens is None else lens.cpu().numpy())
    st, ll, h = _run(dec, E, lens, 6, 0)
    assert np.array_equal(st, ref_s), (tag, "paths differ from the oracle")
    assert np.array_equal(_bits(ll), _bits(ref_l)), (tag, ll, ref_l)
    for form, whole in ((6, 1), (1, 0)):
        st2, ll2, h2 = _run(dec, E, lens, form, whole)
        assert np.array_equal(st, st2) and np.array_equal(_bits(ll), _bits(ll2)), (tag, form, whole)
        assert np.array_equal(h, h2), (tag, form, whole, "history rows differ", np.argwhere(h != h2)[:8])


def _random(S, x, half):
    rng = np.random.default_rng(S)
    A = _banded_matrix(S, half, rng, extras=[x], floor=-50.0, quant=2)
    return A, -(rng.integers(0, 8, S) / 2).astype(np.float32)


# name -> (matrix builder, (proven live width of rows 0 .. 255, width the full waves run at))
MATRICES = {
    "tonet361": (lambda: _tonet(361), (29, 29)),
    "tonet321": (lambda: _tonet(321), (25, 25)),
    "S257": (lambda: _random(257, 256, 12), (31, 32)),      # row 255 is clamped to lo = S - W: source 255 sits at position 30
    "S383": (lambda: _random(383, 382, 13), (27, 29)),      # half-width 13: 27 live positions
    "S300mid": (_s300mid, (21, 25)),                        # the extra column mid-grid, trailing in the windows of rows 127 .. 137
}
_cache = {}


def _decoder(name, dev):
    if name not in _cache:
        A, pi = MATRICES[name][0]()
        assert _widths(A, pi) == MATRICES[name][1], (name, _widths(A, pi))
        _cache[name] = (A, pi, ViterbiDecoder(A, pi, dev))
    return _cache[name]


def _emissions(kind, B, T, S, quant):
    rng = np.random.default_rng(S + len(kind))
    if kind == "peaks":
        return synth.emissions_peaks(B, T, S, seed=9).cpu().numpy()
    if kind == "spikes":
        return spike_emissions(B, T, S, seed=5, quant=quant)
    if kind == "inf":                          # a third of the entries -inf, never a whole frame
        E = -(rng.integers(0, 6, (B, T, S)) / 2).astype(np.float32)
        E[rng.random((B, T, S)) < 0.33] = -np.inf
        E[:, :, 100] = -1.0
        E[:, :, S - 61] = -1.5
        return E
    return (3.0 * rng.standard_normal((B, T, S))).astype(np.float32)      # "real": differs in every frame


@pytest.mark.parametrize("kind", ["peaks", "spikes", "inf", "real"])
@pytest.mark.parametrize("name", list(MATRICES))
def test_trimmed_window_is_bit_exact(dev, name, kind):
    A, pi, dec = _decoder(name, dev)
    S = A.shape[0]
    B, T = 6, 200
    E = torch.from_numpy(_emissions(kind, B, T, S, quant=name.startswith("S"))).to(dev)
    lens = torch.tensor([200, 199, 25, 13, 2, 1], dtype=torch.int64, device=dev)
    _check(dec, A, pi, E, lens, (name, kind))


@pytest.mark.parametrize("name", ["tonet361", "tonet321", "S300mid"])
def test_every_tail_of_the_round(dev, name):
    """Ragged lengths 1, 2, 12, 13, 24, 25, 37, on emissions that differ in every frame and on the spikes."""
    A, pi, dec = _decoder(name, dev)
    S = A.shape[0]
    for kind in ("real", "spikes"):
        Eall = _emissions(kind, 4, 40, S, quant=name.startswith("S"))[:, :37]
        for lengths in LENGTHS:
            E = torch.from_numpy(Eall[:len(lengths)].copy()).to(dev)
            _check(dec, A, pi, E, torch.tensor(lengths, dtype=torch.int64, device=dev), (name, kind, lengths))
    E = torch.from_numpy(_emissions("real", 2, 25, S, quant=False)).to(dev)
    for T in (12, 13, 24, 25):
        _check(dec, A, pi, E[:, :T].contiguous(), None, (name, T))
