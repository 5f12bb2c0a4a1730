"""GPU tests of the packed ragged decode for plans without the wave form (the 722-state grids): banded plans with the floor
form (jdc722, jdc721, imm722w: one workgroup per forward slot, lane back-trace) and step plans (durrieu722, durrieu721: the step
kernel per slot, lazy back-trace over per-song chunk lists).  All through the C ABI via ViterbiDecoder.  Bar: states bit-exact and
log-likelihood bit-equal against the CPU oracle run on every song alone.
GROUP_PLANS are (W, NWT) = (84, 12) and (128, 12); every other pair of the variant: tests/test_gpu_floor_variant_grid.py."""
import time

import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

GROUP_PLANS = ["jdc722", "jdc721", "imm722w", "durrieu722", "durrieu721"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _params(golden, name):
    return golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]


def _pack(E, lens):
    """[B, T, S] + lengths -> packed [sum T_b, S], offsets."""
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return torch.cat([E[b, :int(n)] for b, n in enumerate(lens)], dim=0).contiguous(), off


def _unpack(states, off, T):
    out = np.full((len(off) - 1, T), -1, np.int32)
    for b in range(len(off) - 1):
        out[b, :off[b + 1] - off[b]] = states[off[b]:off[b + 1]]
    return out


@pytest.mark.parametrize("name", GROUP_PLANS)
def test_packed_group_small(golden, dev, name):
    """A handful of songs (lengths 1, 2, odd, even, equal; the list of test_packed_decode_small), every emission kind, fp32 and fp16
    storage: the oracle's states and log-likelihoods of every song alone."""
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    assert not dec.info["wave_ok"]
    S, T = dec.S, 333
    lens = np.array([T, 1, 2, 150, T - 1, 3, 64, 65, 66, 4, 5, T, 129, 1, 77], np.int64)
    for kind, gen in (("peaks", synth.emissions_peaks), ("dense", synth.emissions_dense), ("ties", synth.emissions_ties)):
        for dt in (torch.float32, torch.float16):
            E = gen(len(lens), T, S, seed=9, device=dev, dtype=dt)
            ref_s, ref_l = vo.decode_c(A, pi, E.float().cpu().numpy(), lengths=lens)
            Ep, off = _pack(E, lens)
            st, ll = dec.decode_packed(Ep, off, out_dtype=torch.int32)
            assert np.array_equal(_unpack(st.cpu().numpy(), off, T), ref_s), (name, kind, dt)
            assert np.array_equal(ll.cpu().numpy(), ref_l), (name, kind, dt)


@pytest.mark.parametrize("name", ["jdc722", "durrieu722"])
def test_packed_group_more_songs_than_slots(golden, dev, name):
    """800 recordings (at least three per compute unit, so every workgroup walks several songs back to back), fp16, lengths uniform
    in [T/4, T] with T = 600 plus a few of one and two frames; songs repeat with period 40, lengths do not.  Every state and
    log-likelihood equals the oracle's decode of that song alone, and a second decode returns identical bytes.  The oracle's part,
    timed on 16 CPU threads (twenty songs per oracle call): 33 s for durrieu722, 35 s for jdc722."""
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    S, T, NU = dec.S, 600, 40
    n_cus = torch.cuda.get_device_properties(dev).multi_processor_count
    B = max(800, 3 * n_cus + 32)
    assert B >= 3 * n_cus
    rng = np.random.default_rng(41)
    lens = rng.integers(T // 4, T + 1, B).astype(np.int64)
    lens[[5, 333, 600, B - 1]] = (1, 2, 1, T)
    base = synth.emissions_peaks(NU, T, S, seed=78, device=dev, dtype=torch.float16)
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum(lens)
    Ep = torch.empty((int(off[-1]), S), dtype=torch.float16, device=dev)
    for b in range(B):
        Ep[off[b]:off[b + 1]] = base[b % NU, :lens[b]]
    st, ll = dec.decode_packed(Ep, off, out_dtype=torch.int32)
    st, ll = st.cpu().numpy(), ll.cpu().numpy()
    base_h = base.float().cpu().numpy()
    t0 = time.time()
    for u in range(NU):                                                          # the oracle, once per distinct (song, length)
        idx = np.arange(u, B, NU)
        Eu = np.broadcast_to(base_h[u], (len(idx), T, S))
        rs, rl = vo.decode_c(A, pi, np.ascontiguousarray(Eu), lengths=lens[idx])
        for k, b in enumerate(idx):
            assert np.array_equal(st[off[b]:off[b + 1]], rs[k, :lens[b]]), (name, b, int(lens[b]))
            assert ll[b] == rl[k], (name, b)
    print(name, "oracle seconds", round(time.time() - t0, 1))
    st2, ll2 = dec.decode_packed(Ep, off, out_dtype=torch.int32)
    assert np.array_equal(st2.cpu().numpy(), st) and np.array_equal(ll2.cpu().numpy(), ll)


@pytest.mark.parametrize("name", GROUP_PLANS)
def test_packed_group_equals_padded(golden, dev, name):
    """One ragged batch per plan: decode_packed returns the bytes of decode(lengths=) on the batch padded to the longest song."""
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    S, T = dec.S, 1300
    lens = np.array([T, 1, 700, 2, 1299, 64, 1025, 333, 5, T, 129, 900, 17], np.int64)
    E = synth.emissions_dense(len(lens), T, S, seed=23, device=dev, dtype=torch.float16)
    ps, pl = dec.decode(E, lengths=torch.from_numpy(lens).to(dev), out_dtype=torch.int32)
    Ep, off = _pack(E, lens)
    st, ll = dec.decode_packed(Ep, off, out_dtype=torch.int32)
    assert np.array_equal(_unpack(st.cpu().numpy(), off, T), ps.cpu().numpy()), name
    assert ll.cpu().numpy().tobytes() == pl.cpu().numpy().tobytes(), name


@pytest.mark.parametrize("name", ["jdc722", "durrieu722"])
def test_packed_group_full_length_song(golden, dev, name):
    """One song of T = 30000 frames next to a song of one frame, fp16: the lane back-trace (jdc722) and the lazy back-trace
    (durrieu722) with as many chunks per song as their rules allow, against the oracle."""
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    S, T = dec.S, 30000
    E = synth.emissions_peaks(1, T, S, seed=3, device=dev, dtype=torch.float16)
    lens = np.array([T, 1], np.int64)
    Ep = torch.cat([E[0], E[0, 77:78]], dim=0).contiguous()
    off = np.array([0, T, T + 1], np.int64)
    st, ll = dec.decode_packed(Ep, off, out_dtype=torch.int32)
    st, ll = st.cpu().numpy(), ll.cpu().numpy()
    for b in range(2):
        rs, rl = vo.decode_c(A, pi, Ep[off[b]:off[b + 1]].float().unsqueeze(0).cpu().numpy())
        assert np.array_equal(st[off[b]:off[b + 1]], rs[0]), (name, b, int(lens[b]))
        assert ll[b] == rl[0], (name, b)


def test_decode_recordings_on_a_722_state_grid(dev):
    """reference_api.SoftMaxViterbi.decode_recordings on the jdc grid (721 bins + unvoiced, band of +/- 40): recordings of different
    lengths through one builder launch, one packed decode and one voicing map -- every recording's (voiced, bins) equal to
    decode_logits of that recording alone."""
    from tests.common import logits_case
    from viterbi_spl_amd import reference_api as ra
    A, pi = synth.tonet_transition(721, 40), synth.floored_prior(722)
    vit = ra.SoftMaxViterbi(A, pi, device=dev)
    assert vit._decoder.S == 722 and not vit._decoder.info["wave_ok"]
    lens = [257, 1, 64, 1000, 2, 333, 129]
    recs = [logits_case(200 + k, n, 722) for k, n in enumerate(lens)]
    got = vit.decode_recordings(recs)
    assert len(got) == len(lens)
    for k, x in enumerate(recs):
        v1, b1 = vit.decode_logits(x)
        assert got[k][0].shape == (lens[k],) and torch.equal(got[k][0], v1) and torch.equal(got[k][1], b1), k


@pytest.mark.parametrize("name", ["jdc722", "durrieu722"])
def test_packed_group_error_paths(golden, dev, name):
    """vit_decode_packed at the C ABI for the workgroup forms: status codes, not exceptions -- bad offsets, a workspace that is too
    small, an empty batch (the codes of test_packed_decode_error_paths)."""
    lib = _lib.load()
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    S = dec.S
    E = synth.emissions_peaks(1, 50, S, seed=1, device=dev)[0].contiguous()
    st = torch.empty((50,), dtype=torch.int32, device=dev)
    ll = torch.empty((2,), dtype=torch.float32, device=dev)
    need = dec.workspace_bytes_packed(2, 50)
    assert need > 50 * 724 * 4
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    wp = (ws.data_ptr() + 255) & ~255

    def call(off, nbytes=need, B=None):
        off = np.asarray(off, np.int64)
        return lib.vit_decode_packed(dec._plan, E.data_ptr(), _lib.VIT_F32, len(off) - 1 if B is None else B, off.ctypes.data, wp, nbytes,
                                     st.data_ptr(), ll.data_ptr(), None)
    assert call([0, 20, 50]) == 0
    torch.cuda.synchronize()
    ref_s, ref_l = vo.decode_c(A, pi, np.stack([np.pad(E[:20].cpu().numpy(), ((0, 30), (0, 0))), np.pad(E[20:].cpu().numpy(), ((0, 20), (0, 0)))]),
                               lengths=np.array([20, 30], np.int64))
    assert np.array_equal(st[:20].cpu().numpy(), ref_s[0, :20]) and np.array_equal(st[20:].cpu().numpy(), ref_s[1, :30])
    assert np.array_equal(ll.cpu().numpy(), ref_l)
    assert call([1, 20, 50]) == -1                         # offsets must start at 0           (VIT_EINVAL)
    assert call([0, 20, 20]) == -1                         # an empty song
    assert call([0, 30, 20]) == -1                         # decreasing
    assert call([0, 20, 50], nbytes=need - 1) == -4        # VIT_EWORKSPACE
    assert call([0], B=0) == 0                             # nothing to do
