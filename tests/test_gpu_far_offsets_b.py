"""Construction B of tests/far_offsets.py on the GPU: thousands of songs of about 1500 frames, B * T past element 2^31 and byte 2^32
of the emissions and of the history -- the regime the library is advertised for, at the smallest size that reaches it.  The batch
is 8 distinct songs repeated; the oracle decodes the 8, every copy must equal its original, bit for bit.  Padded (wave and
workgroup forms) and packed (plain, checkpointed, bounded, float64, float64 checkpointed)."""
import numpy as np
import pytest
import torch

from tests import f64_ref, far_offsets as fo
from tests.common import f32_bits
from viterbi_spl_amd import ViterbiDecoder, _lib

pytestmark = pytest.mark.gpu

T = 1500


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _base(S, f16, seed):
    return fo.base_songs(S, T, f16, seed)


def _decoder(golden, dev, name):
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    return dec, A, pi, fo.history_rows(_lib.load(), dec._plan)


UNIFORM = [("tonet361", False, ("wave", "group")), ("msnet321", True, ("wave", "group")), ("jdc722", True, ("banded",)),
           ("jdc722", False, ("banded",)), ("durrieu722", True, ("auto",))]


@pytest.mark.parametrize("name,f16,algos", UNIFORM, ids=[f"{n}-{'f16' if h else 'f32'}" for n, h, _ in UNIFORM])
def test_uniform_decode(golden, dev, name, f16, algos):
    """decode() of [B, 1500, S] with ragged lengths: the last songs lie past both marks of the emissions and of each form's history."""
    dec, A, pi, rows = _decoder(golden, dev, name)
    S, isz = dec.S, 2 if f16 else 4
    used = [rows["group" if a == "banded" else a] for a in algos]     # ("banded" on a plan without the wave form: the workgroup kernel)
    widest = max(used, key=lambda ri: ri[0] * ri[1])
    B, _ = fo.shape_b(S, isz, widest, T)
    assert B * T * S > max(fo.mark_elements(isz)) and all(B * T * r > max(fo.mark_elements(i)) for r, i in used)
    fo.need_free(B * T * (S * isz + widest[0] * widest[1]) + B * T * 4)
    base = _base(S, f16, seed=31)
    ref_s, ref_l = fo.expected_a(A, pi, base, fo.LENS_B)
    E = torch.from_numpy(base).to(dev).repeat(B // 8, 1, 1)
    ln = torch.tensor(fo.LENS_B, dtype=torch.int64, device=dev).repeat(B // 8)
    want_s = torch.from_numpy(ref_s).to(dev)
    with fo.measured(f"b/decode/{name}/{'f16' if f16 else 'f32'}", (B, T, S)):
        for algo in algos:
            assert dec.forward_family(B, algo) == ("wave" if algo == "wave" else "dense" if algo == "auto" else "group"), algo
            st, ll = dec.decode(E, lengths=ln, algo=algo, out_dtype=torch.int32)
            for b in (0, 7, B - 8, B - 1):
                assert np.array_equal(st[b].cpu().numpy(), ref_s[b % 8]), (name, algo, b)
            assert bool((st.view(B // 8, 8, T) == want_s[None]).all()), (name, algo)
            assert np.array_equal(f32_bits(ll.cpu().numpy()).reshape(B // 8, 8), np.tile(f32_bits(ref_l), (B // 8, 1))), (name, algo)
    del dec, E, st, ll
    fo.release()


def _packed_batch(dev, A, pi, S, f16, hist, f64=False, lens8=fo.LENS_B):
    """fo.packed_batch_b at the real marks -> (E [N, S] on the device, offsets, expected states [8, T], the same of one period of 8
    recordings concatenated, expected loglik [8], the recordings asserted one by one)."""
    p = fo.packed_batch_b(A, pi, _base(S, f16, seed=47), lens8, hist, f16, f64=f64)
    N = int(p["off"][-1])
    fo.need_free(N * (S * (2 if f16 else 4) + hist[0] * hist[1]) + N * 4)
    E = torch.from_numpy(p["period"]).to(dev).repeat(p["B"] // 8, 1)
    assert E.shape[0] == N
    return E, p["off"], p["ref_s"], p["want"], p["ref_l"], p["picks"]


def _check_packed(st, ll, off, ref_s, want, ref_l, picks, what, bits=f32_bits):
    B = len(off) - 1
    for b in picks:                                                # the first, the last and every recording that holds a mark row
        n = int(off[b + 1] - off[b])
        assert np.array_equal(st[int(off[b]):int(off[b + 1])].cpu().numpy(), ref_s[b % 8, :n]), (what, "recording", b)
    want_d = torch.from_numpy(want).to(st.device)
    assert bool((st.view(B // 8, -1) == want_d[None]).all()), what
    assert np.array_equal(bits(ll.cpu().numpy()).reshape(B // 8, 8), np.tile(bits(ref_l), (B // 8, 1))), what


PACKED = [("tonet361", False), ("tonet361", True), ("msnet321", False), ("jdc722", True), ("jdc722", False), ("durrieu722", True)]


@pytest.mark.parametrize("name,f16", PACKED, ids=[f"{n}-{'f16' if h else 'f32'}" for n, h in PACKED])
def test_packed_decodes(golden, dev, name, f16):
    """decode_packed, and under a bound decode_packed_checkpointed (wave-form plans) and decode_packed_bounded (every plan with a
    packed decode): the packed emission rows, the int64 offsets times the row strides, the history and the states of the last
    recordings lie past the marks."""
    dec, A, pi, rows = _decoder(golden, dev, name)
    E, off, ref_s, want, ref_l, picks = _packed_batch(dev, A, pi, dec.S, f16, rows["packed"])
    with fo.measured(f"b/decode_packed/{name}/{'f16' if f16 else 'f32'}", (len(off) - 1, int(off[-1]), dec.S)):
        st, ll = dec.decode_packed(E, off, out_dtype=torch.int32)
        _check_packed(st, ll, off, ref_s, want, ref_l, picks, (name, "packed"))
        for K in (64, 1024):
            if dec.info["wave_ok"]:
                st, ll = dec.decode_packed_checkpointed(E, off, segment_frames=K, out_dtype=torch.int32)
                _check_packed(st, ll, off, ref_s, want, ref_l, picks, (name, "packed_checkpointed", K))
            st, ll = dec.decode_packed_bounded(E, off, segment_frames=K, out_dtype=torch.int32)
            _check_packed(st, ll, off, ref_s, want, ref_l, picks, (name, "packed_bounded", K))
    del dec, E, st, ll
    fo.release()


PACKED_F64 = [("tonet361", False), ("jdc722", True), ("msnet321", True)]
# the NumPy float64 reference costs S^2 per frame (1.5 ms at S = 722): the 722-state case cycles through shorter recordings, and more of them
LENS_F64_722 = (400, 399, 373, 1, 337, 400, 277, 302)


@pytest.mark.parametrize("name,f16", PACKED_F64, ids=[f"{n}-{'f16' if h else 'f32'}" for n, h in PACKED_F64])
def test_packed_f64_decodes(golden, dev, name, f16):
    """decode_f64_packed (rows of doubles, one per packed frame) and decode_f64_packed_checkpointed against tests/f64_ref.py."""
    dec, A, pi, rows = _decoder(golden, dev, name)
    E, off, ref_s, want, ref_l, picks = _packed_batch(dev, A, pi, dec.S, f16, rows["f64_packed"], f64=True,
                                                      lens8=LENS_F64_722 if dec.S > 400 else fo.LENS_B)
    with fo.measured(f"b/decode_f64_packed/{name}/{'f16' if f16 else 'f32'}", (len(off) - 1, int(off[-1]), dec.S)):
        st, ll = dec.decode_f64_packed(E, off, out_dtype=torch.int32)
        _check_packed(st, ll, off, ref_s, want, ref_l, picks, (name, "f64_packed"), f64_ref.bits64)
        for K in (64, 1024):
            st, ll = dec.decode_f64_packed_checkpointed(E, off, segment_frames=K, out_dtype=torch.int32)
            _check_packed(st, ll, off, ref_s, want, ref_l, picks, (name, "f64_packed_checkpointed", K), f64_ref.bits64)
    del dec, E, st, ll
    fo.release()
