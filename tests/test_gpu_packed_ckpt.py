"""GPU tests of the packed checkpointed decode (vit_decode_packed_checkpointed, wave-form plans): ragged recordings in one packed
buffer, decoded under a workspace budget.  Bar: states and log-likelihood bits equal to decode_packed and to the CPU oracle run on
every recording alone."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

EDGE_LENS = np.array([1, 2, 63, 64, 65, 127, 128, 129, 193, 700, 1], np.int64)
GEN = {"peaks": synth.emissions_peaks, "dense": synth.emissions_dense}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _params(golden, name):
    return golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]


def _offsets(lens):
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return off


def _pack(E, lens):
    """[B, T, S] + lengths -> packed [sum T_b, S], offsets."""
    return torch.cat([E[b, :int(n)] for b, n in enumerate(lens)], dim=0).contiguous(), _offsets(lens)


def _bits(x):
    return x.detach().cpu().numpy().view(np.int32)


def _assert_matches_oracle(st, ll, off, ref_s, ref_l, what):
    st, ll = st.cpu().numpy(), ll.cpu().numpy()
    for b in range(len(off) - 1):
        assert np.array_equal(st[off[b]:off[b + 1]], ref_s[b, :off[b + 1] - off[b]]), (what, "states of recording", b)
    assert np.array_equal(ll.view(np.int32), ref_l.view(np.int32)), (what, "log-likelihood bits")


@pytest.mark.parametrize("kind", ["peaks", "dense"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("name", ["tonet361", "msnet321"])
def test_bit_equality_at_the_segment_edges(golden, dev, name, dt, kind):
    """Recordings of 1, 2, 63, 64, 65, 127, 128, 129, 193, 700 and 1 frames in one buffer, segments of 64 frames: a single frame, no
    checkpoint, a checkpoint exactly at the end, one frame into a new segment.  Then segments of 128 frames, and of 4096 (every
    recording is one segment).  States and log-likelihood bits of decode_packed and of the oracle, for every recording."""
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    assert dec.info["wave_ok"]
    E = GEN[kind](len(EDGE_LENS), 700, dec.S, seed=21, device=dev, dtype=dt)
    ref_s, ref_l = vo.decode_c(A, pi, E.float().cpu().numpy(), lengths=EDGE_LENS)
    Ep, off = _pack(E, EDGE_LENS)
    want_s, want_l = dec.decode_packed(Ep, off, out_dtype=torch.int32)
    _assert_matches_oracle(want_s, want_l, off, ref_s, ref_l, (name, kind, dt, "decode_packed"))
    for K in (64, 128, 4096):
        st, ll = dec.decode_packed_checkpointed(Ep, off, segment_frames=K, out_dtype=torch.int32)
        assert st.dtype == torch.int32 and st.shape == want_s.shape and ll.shape == want_l.shape
        assert torch.equal(st, want_s) and np.array_equal(_bits(ll), _bits(want_l)), (name, kind, dt, K)
        _assert_matches_oracle(st, ll, off, ref_s, ref_l, (name, kind, dt, K))
    st64, _ = dec.decode_packed_checkpointed(Ep, torch.from_numpy(off), segment_frames=64)       # offsets as a tensor, int64 states
    assert st64.dtype == torch.int64 and torch.equal(st64, want_s.to(torch.int64))


def test_more_units_than_unit_slots(golden, dev):
    """About 2100 recordings of 65 .. 130 frames and one of 700, segments of 64 frames, fp16: more recordings than a launch of pass 2
    takes units (8 per compute unit), so launches hold fewer units than are ready; the long recording keeps total frames / longest
    small (few pass-1 wavefronts, each walking several recordings) and goes on for eleven launches while the others finish after
    two or three.  Equal to decode_packed on every recording, to the oracle on twelve: the shortest, the longest, two of 128
    frames (a multiple of the segment length) and the rest of the first distinct emission rows."""
    A, pi = _params(golden, "tonet361")
    dec = ViterbiDecoder(A, pi, dev)
    n_cus = torch.cuda.get_device_properties(dev).multi_processor_count
    S, K, NU, TL = 361, 64, 48, 700
    B = max(2100, 8 * n_cus + 52)
    rng = np.random.default_rng(77)
    lens = rng.integers(65, 131, B).astype(np.int64)
    lens[[0, 1, 2, 3, B - 1]] = (65, 128, TL, 130, 128)
    assert B > 8 * n_cus, "the test wants more recordings than units per launch"
    base = synth.emissions_peaks(NU, TL, S, seed=91, device=dev, dtype=torch.float16)        # recording b holds song b % NU, lengths differ
    base[NU // 2:] = synth.emissions_dense(NU - NU // 2, TL, S, seed=92, device=dev, dtype=torch.float16)
    off = _offsets(lens)
    song = torch.from_numpy(np.repeat(np.arange(B) % NU, lens)).to(dev)
    frame = torch.from_numpy(np.concatenate([np.arange(n) for n in lens])).to(dev)
    Ep = base[song, frame].contiguous()
    assert Ep.shape == (int(off[-1]), S) and 150_000 < off[-1] < 400_000
    want_s, want_l = dec.decode_packed(Ep, off, out_dtype=torch.int32)
    st, ll = dec.decode_packed_checkpointed(Ep, off, segment_frames=K, out_dtype=torch.int32)
    assert torch.equal(st, want_s) and np.array_equal(_bits(ll), _bits(want_l))
    picks = np.array([0, 1, 2, 3, B - 1, 5, 6, 7, 8, 9, 10, 11])
    assert lens[picks].min() == lens.min() and lens[picks].max() == lens.max() and (lens[picks] % K == 0).any()
    ref_s, ref_l = vo.decode_c(A, pi, base[picks % NU].float().cpu().numpy(), lengths=lens[picks])
    st, ll = st.cpu().numpy(), ll.cpu().numpy()
    for k, b in enumerate(picks):
        assert np.array_equal(st[off[b]:off[b + 1]], ref_s[k, :lens[b]]), (b, int(lens[b]))
        assert ll[b:b + 1].view(np.int32) == ref_l[k:k + 1].view(np.int32), b


def test_stays_inside_its_workspace(golden, dev):
    """A caller-owned workspace of exactly workspace_bytes_packed_checkpointed + 256 bytes, between 1 MB of guard bytes on either
    side, everything filled with 0xFF (NaN patterns): the result of the library-owned workspace, guards intact, a second call
    returns identical bytes.  One byte less is refused before anything runs.  The size on THIS device: n_units x (K + 1) + sum (n_b
    - 1) + n_units rows of 384 floats, n_units = min(B, 8 x compute units), plus tables."""
    lib = _lib.load()
    A, pi = _params(golden, "tonet361")
    dec = ViterbiDecoder(A, pi, dev)
    lens = np.concatenate([EDGE_LENS, [1000, 333]]).astype(np.int64)
    E = synth.emissions_peaks(len(lens), 1000, dec.S, seed=4, device=dev)
    Ep, off = _pack(E, lens)
    want_s, want_l = dec.decode_packed(Ep, off, out_dtype=torch.int32)
    G = 1 << 20
    n_units = min(len(lens), 8 * torch.cuda.get_device_properties(dev).multi_processor_count)
    for K in (64, 100, 640):
        need = dec.workspace_bytes_packed_checkpointed(off, K)
        rows = n_units * (K + 1) + int(((lens + K - 1) // K - 1).sum()) + n_units
        assert rows * 384 * 4 <= need <= rows * 384 * 4 + 24 * len(lens) + 8 * int(((lens + K - 1) // K).sum()) + 152 * n_units + 16 * 256
        buf = torch.full((G + 256 + need + 256 + G,), 0xFF, dtype=torch.uint8, device=dev)
        o = G + (-(buf.data_ptr() + G)) % 256                                # first 256-byte aligned address behind the front guard
        ws = buf[o:o + need + 256]
        assert ws.data_ptr() % 256 == 0
        for _ in range(2):
            st, ll = dec.decode_packed_checkpointed(Ep, off, segment_frames=K, out_dtype=torch.int32, workspace=ws)
            torch.cuda.synchronize()
            assert torch.equal(st, want_s) and np.array_equal(_bits(ll), _bits(want_l)), K
        assert bool((buf[:o] == 0xFF).all()), (K, "bytes in front of the workspace were written")
        assert bool((buf[o + need:] == 0xFF).all()), (K, "bytes behind the workspace were written")
        with pytest.raises(ValueError):
            dec.decode_packed_checkpointed(Ep, off, segment_frames=K, workspace=ws[:need + 255])
        st = torch.full((int(off[-1]),), 12345, dtype=torch.int32, device=dev)
        ll = torch.full((len(lens),), 7.0, dtype=torch.float32, device=dev)
        args = (dec._plan, Ep.data_ptr(), _lib.VIT_F32, len(lens), off.ctypes.data, ws.data_ptr())
        assert lib.vit_decode_packed_checkpointed(*args, need - 1, st.data_ptr(), ll.data_ptr(), K, None) == -4      # VIT_EWORKSPACE
        torch.cuda.synchronize()
        assert bool((st == 12345).all()) and bool((ll == 7.0).all())
        assert lib.vit_decode_packed_checkpointed(*args, need, st.data_ptr(), ll.data_ptr(), K, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(st, want_s) and np.array_equal(_bits(ll), _bits(want_l)), K


def test_refusals_are_loud_and_early(golden, dev):
    """Plans without the wave form -- a 722-state floor plan, a step plan, an unstructured matrix -- get size 0, ViterbiHipError and
    VIT_EUNSUPPORTED; a segment length out of range and bad offsets VIT_EINVAL.  Nothing is enqueued in any of these cases: `states`
    and `loglik` keep their sentinels."""
    lib = _lib.load()
    lens = np.array([100, 200, 65], np.int64)
    off = _offsets(lens)

    def call(dec, E, K, offsets=off, B=None):
        st = torch.full((int(off[-1]),), 12345, dtype=torch.int32, device=dev)
        ll = torch.full((len(lens),), 7.0, dtype=torch.float32, device=dev)
        ws = torch.empty((1 << 26) + 256, dtype=torch.uint8, device=dev)
        offsets = np.asarray(offsets, np.int64)
        rc = lib.vit_decode_packed_checkpointed(dec._plan, E.data_ptr(), _lib.VIT_F32, len(offsets) - 1 if B is None else B, offsets.ctypes.data,
                                                (ws.data_ptr() + 255) & ~255, 1 << 26, st.data_ptr(), ll.data_ptr(), K, None)
        torch.cuda.synchronize()
        assert bool((st == 12345).all()) and bool((ll == 7.0).all()), "a refused call wrote its outputs"
        return rc

    for name in ("jdc722", "durrieu722", "dense97"):
        dec = ViterbiDecoder(*_params(golden, name), dev)
        assert not dec.info["wave_ok"]
        E = synth.emissions_dense(1, int(off[-1]), dec.S, seed=1, device=dev)[0].contiguous()
        assert int(lib.vit_workspace_bytes_packed_checkpointed(dec._plan, 3, off.ctypes.data, 64)) == 0, name
        with pytest.raises(_lib.ViterbiHipError):
            dec.workspace_bytes_packed_checkpointed(off, 64)
        with pytest.raises(_lib.ViterbiHipError):
            dec.decode_packed_checkpointed(E, off, segment_frames=64)
        with pytest.raises(_lib.ViterbiHipError, match="no packed checkpointed decode" if name != "dense97" else "packed decode needs"):
            dec.plan_workspace_packed(off, 1000)
        assert call(dec, E, 64) == -5, name                                   # VIT_EUNSUPPORTED
    dec = ViterbiDecoder(*_params(golden, "tonet361"), dev)
    E = synth.emissions_dense(1, int(off[-1]), dec.S, seed=1, device=dev)[0].contiguous()
    for K in (63, (1 << 24) + 1, 0, -5):
        assert int(lib.vit_workspace_bytes_packed_checkpointed(dec._plan, 3, off.ctypes.data, K)) == 0, K
        assert call(dec, E, K) == -1, K                                       # VIT_EINVAL
        with pytest.raises(_lib.ViterbiHipError):
            dec.decode_packed_checkpointed(E, off, segment_frames=K)
    for bad in ([1, 100, 300, 365], [0, 100, 100, 365], [0, 300, 100, 365]):  # not from 0, an empty recording, decreasing
        assert call(dec, E, 64, offsets=bad) == -1, bad
        assert int(lib.vit_workspace_bytes_packed_checkpointed(dec._plan, 3, np.asarray(bad, np.int64).ctypes.data, 64)) == 0
        with pytest.raises(ValueError):
            dec.decode_packed_checkpointed(E, bad, segment_frames=64)
    with pytest.raises(ValueError):
        dec.decode_packed_checkpointed(E, off[:-1], segment_frames=64)       # offsets must end at the number of rows
    assert lib.vit_decode_packed_checkpointed(dec._plan, E.data_ptr(), 7, 3, off.ctypes.data, 256, 1 << 26, 256, None, 64, None) == -1    # dtype
    assert lib.vit_decode_packed_checkpointed(dec._plan, E.data_ptr(), 0, 3, None, 256, 1 << 26, 256, None, 64, None) == -1              # offsets
    assert call(dec, E, 64, offsets=[0], B=0) == 0                            # nothing to do


def test_budget_policy(golden, dev):
    """decode_packed(max_workspace_bytes=...) over shrinking budgets on one ragged set: "full" while the history fits, then
    "checkpointed" with a segment length that never grows; identical bits under every budget; a budget below the smallest need
    (for this set that is the need at K = 64) raises and names it.  decode_recordings under a tight budget returns what it returns
    without one."""
    A, pi = _params(golden, "tonet361")
    dec = ViterbiDecoder(A, pi, dev)
    lens = np.array([4100, 1, 2, 1500, 4099, 3, 2049, 65, 4096], np.int64)
    E = synth.emissions_peaks(len(lens), 4100, 361, seed=3, device=dev)
    Ep, off = _pack(E, lens)
    del E
    full = dec.workspace_bytes_packed(len(lens), int(off[-1]))
    needs = {K: dec.workspace_bytes_packed_checkpointed(off, K) for K in (8192, 4096, 2048, 1024, 512, 256, 128, 64)}
    assert min(needs.values()) == needs[64] < full // 15
    want_s, want_l = dec.decode_packed(Ep, off, out_dtype=torch.int32)
    seen, Ks = [], []
    for budget in (None, 2 * full, full, full - 1, full // 2, full // 3, full // 5, full // 9, full // 15, needs[64]):
        mode = dec.plan_workspace_packed(off, budget)
        seen.append(mode["mode"])
        assert budget is None or mode["workspace_bytes"] <= budget
        if mode["mode"] == "checkpointed":
            assert mode["workspace_bytes"] == needs[mode["segment_frames"]]
            assert all(needs[K] > budget for K in needs if K > mode["segment_frames"]), "a longer segment fits"
            Ks.append(mode["segment_frames"])
        st, ll = dec.decode_packed(Ep, off, out_dtype=torch.int32, max_workspace_bytes=budget)
        assert torch.equal(st, want_s) and np.array_equal(_bits(ll), _bits(want_l)), (budget, mode)
    assert seen[:3] == ["full"] * 3 and seen[3] == "checkpointed" and seen[-1] == "checkpointed", seen
    assert seen == sorted(seen, key=lambda m: m != "full"), seen              # never back to "full"
    assert Ks == sorted(Ks, reverse=True) and Ks[-1] == 64 and len(set(Ks)) >= 3, Ks
    with pytest.raises(_lib.ViterbiHipError, match=str(needs[64])):
        dec.decode_packed(Ep, off, max_workspace_bytes=needs[64] - 1)
    with pytest.raises(_lib.ViterbiHipError, match=str(needs[64])):
        dec.plan_workspace_packed(off, 1000)

    from tests.common import logits_case
    from viterbi_spl_amd import reference_api as ra
    vit = ra.Viterbi(synth.tonet_transition(360, 14), synth.floored_prior(361), device=dev)
    rlens = [257, 1, 64, 1000, 2, 333, 129]
    recs = [logits_case(100 + k, n, 360) for k, n in enumerate(rlens)]
    roff = _offsets(rlens)
    tight = vit._decoder.workspace_bytes_packed_checkpointed(roff, 64)
    assert vit._decoder.plan_workspace_packed(roff, tight) == {"mode": "checkpointed", "segment_frames": 64, "workspace_bytes": tight}
    got, want = vit.decode_recordings(recs, max_workspace_bytes=tight), vit.decode_recordings(recs)
    assert len(got) == len(want) == len(rlens)
    for k in range(len(rlens)):
        assert got[k][0].shape == (rlens[k],) and torch.equal(got[k][0], want[k][0]) and torch.equal(got[k][1], want[k][1]), k
    with pytest.raises(_lib.ViterbiHipError):
        vit.decode_recordings(recs, max_workspace_bytes=tight - 1)
