"""The split-window floor forward kernel (forward_form 6) runs the rounds of its frame loop whose emission requests all stay inside
the song ("interior" rounds) in a loop body without the row clamp, the last full round and the tail in the clamped body.  Not a
bit may change against the one-target kernel (forward_form 1) and the CPU oracle: paths, log-likelihood bits and the raw history
rows [B, T, SD] after zeroing the workspace (pad column S carries the frame maximum M).

The song lengths sit on every boundary of that split for the prefetch depth 12: no interior round, exactly one, two and more, each
with an empty tail, a one-frame tail and the longest tail.  Which class a length lands in is checked on the CPU first, through the
host library's replay of the loop (tests/test_floor_split_rounds_host.py); that replay, not this test, is what shows that no
request passes a song's last row (a row requested too far is one no frame uses).  What shows here is a frame that got the wrong
row: the emissions differ from frame to frame, and the batches are ragged so that one launch runs every class side by side."""
import numpy as np
import pytest
import torch

from tests.test_floor_split_rounds_host import round_classes
from tests.test_floor_trim_host import spike_emissions
from tests.test_gpu_floor_split_join import MATRICES, _case, _decoder, _noise
from tests.test_gpu_floor_split_trim import _check

pytestmark = pytest.mark.gpu

PF = 12
# length -> (interior rounds, clamped full rounds, tail frames)
CLASSES = {
    1: (0, 0, 0), 2: (0, 0, 1), 12: (0, 0, 11),
    13: (0, 1, 0), 14: (0, 1, 1), 24: (0, 1, 11),
    25: (1, 1, 0), 26: (1, 1, 1), 36: (1, 1, 11),
    37: (2, 1, 0), 38: (2, 1, 1),
    49: (3, 1, 0), 50: (3, 1, 1), 61: (4, 1, 0),
}
BATCHES = ([61, 37, 25, 13, 2, 1], [50, 38, 26, 14, 12], [49, 36, 24])      # at most six songs each
T = 61
# (matrix, emission dtype): fp32 reaches the trimmed instantiations (29, 25), the whole window with the extra column in M's slot
# quad (S257) and the select instantiation (S300mid); fp16 always takes the whole window, with and without the slot quad
CASES = [("tonet361", torch.float32), ("tonet321", torch.float32), ("S257", torch.float32), ("S300mid", torch.float32),
         ("tonet361", torch.float16), ("S300mid", torch.float16)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from viterbi_spl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def test_lengths_land_in_their_round_class():
    """Premise, on the CPU: every length runs the rounds it is meant to run."""
    assert sorted(n for b in BATCHES for n in b) == sorted(CLASSES)
    for n, want in CLASSES.items():
        assert round_classes(n, PF) == want and round_classes(n) == want, (n, round_classes(n, PF), want)
    seen = {(min(ni, 2), nt) for ni, _, nt in CLASSES.values()}
    assert seen >= {(ni, nt) for ni in (0, 1, 2) for nt in (0, 1)} and {(0, 11), (1, 11)} <= seen


def _songs(S):
    """[6, T, S]: quantised noise (multiples of 1/2, exact in fp16), the even songs with the spike set of tests/test_floor_trim_host.py."""
    E = _noise(np.random.default_rng(S), 6, T, S)
    E[0::2] = spike_emissions(3, T, S, seed=5, quant=True)
    return E


@pytest.mark.parametrize("name,dtype", CASES, ids=[f"{n}-{'f16' if d == torch.float16 else 'f32'}" for n, d in CASES])
def test_round_split_is_bit_exact(dev, name, dtype):
    test_lengths_land_in_their_round_class()          # before any GPU call
    assert name in MATRICES
    c = _case(name)
    S = c["A"].shape[0]
    Eall = _songs(S)
    assert np.array_equal(Eall.astype(np.float16).astype(np.float32), Eall)
    for lengths in BATCHES:
        assert len(lengths) <= 6 and max(lengths) <= T
        E = torch.from_numpy(Eall[:len(lengths), :max(lengths)].copy()).to(dev).to(dtype)
        _check(_decoder(name, dev), c["A"], c["pi"], E, torch.tensor(lengths, dtype=torch.int64, device=dev), (name, str(dtype), lengths))
