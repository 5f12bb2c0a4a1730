"""The wave form's checkpointed and packed entry points on the geometries of tests/test_gpu_parity.py::test_wave_form_geometries
(tests/floor_grid.py wave_geometry: 321 .. 383 states, half-widths 1 .. 14, 0 - 2 extra columns anywhere), where that test runs
decode only: decode_checkpointed (wave.hip WaveHist::CkptPass / Segment), decode_packed (the slot walk, per-song bases) and
decode_packed_checkpointed (WaveHist::PackedCkptPass / PackedSegment, per-unit bases) under every "wave_uniform" setting, and the two
checkpointed ones under every "wave_two" register budget (the packed decode's header text does not list it).  Extra columns in the
middle of the states take the general variants; the shipped matrices, with the one extra column last, take the specialised ones.

Eleven songs of 200, 1, 2, 3, 13, 14, 63, 64, 65, 129 and 199 frames on the half-integer grid (exact ties, exact in fp16), packed in a
fixed shuffled order, segments of 64 frames, storage type alternating by seed.  Bar: states and log-likelihood bits equal to the CPU
oracle run on every song alone."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests import floor_grid as fg
from viterbi_spl_amd import ViterbiDecoder, _lib

pytestmark = pytest.mark.gpu

K = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x, np.float32)
    return x.view(np.uint32)


@pytest.mark.parametrize("seed", fg.WAVE_FORM_SEEDS)
def test_wave_variants_on_every_geometry(dev, seed):
    S, half, extras, A, pi, _ = fg.wave_geometry(seed)
    dec = ViterbiDecoder(A, pi, dev)
    assert dec.info["wave_ok"] and dec.info["extras"] == extras, (seed, S, half, extras, dec.info)
    lens = fg.LENGTHS
    B, T = len(lens), fg.T
    E32 = -(np.random.default_rng(1900 + seed).integers(0, 12, (B, T, S)) / 2).astype(np.float32)
    ref_s, ref_l = vo.decode_c(A, pi, E32, lengths=lens)
    E = torch.from_numpy(E32).to(dev)
    E = E.half() if seed & 1 else E
    ln = torch.from_numpy(lens).to(dev)
    order = fg.pack_order(lens)
    off = fg.offsets_of(lens[order])
    Ep = torch.cat([E[b, :int(lens[b])] for b in order], dim=0).contiguous()

    def padded(what):
        st, ll = dec.decode_checkpointed(E, segment_frames=K, lengths=ln, out_dtype=torch.int32)
        assert np.array_equal(st.cpu().numpy(), ref_s), (seed, S, half, extras, what, "decode_checkpointed: states")
        assert np.array_equal(_bits(ll), _bits(ref_l)), (seed, S, half, extras, what, "decode_checkpointed: log-likelihood bits")

    def packed(entry, what, **kw):
        st, ll = getattr(dec, entry)(Ep, off, out_dtype=torch.int32, **kw)
        st = st.cpu().numpy()
        for k, b in enumerate(order):
            assert np.array_equal(st[off[k]:off[k + 1]], ref_s[b, :lens[b]]), (seed, S, half, extras, what, entry, "states of song", int(b))
        assert np.array_equal(_bits(ll), _bits(ref_l[order])), (seed, S, half, extras, what, entry, "log-likelihood bits")

    try:
        for uni in (0, 1, 2, 3):    # specialised variants where the plan proves them | neither | the first only | three groups
            dec.set_option("wave_uniform", uni)
            padded(("wave_uniform", uni))
            packed("decode_packed", ("wave_uniform", uni))
            packed("decode_packed_checkpointed", ("wave_uniform", uni), segment_frames=K)
        dec.set_option("reset", 0)
        for two in (0, 1, 2):       # the register budgets of the wave kernel
            dec.set_option("wave_two", two)
            padded(("wave_two", two))
            packed("decode_packed_checkpointed", ("wave_two", two), segment_frames=K)
    finally:
        dec.set_option("reset", 0)
