"""GPU tests of the bounded packed decode (vit_decode_packed_bounded): ragged recordings in one packed buffer, decoded under a
workspace budget by the plans without the wave form -- the 722- and 721-state floor plans (jdc722, jdc721, imm722w: the
packed-checkpoint variant of the one-target floor kernel, sparse back-trace over the units) and step plans (durrieu722, durrieu721:
the same variant of the step kernel, lazy back-trace over the units).  Bar: states and log-likelihood bits equal to decode_packed
and to the CPU oracle run on every recording alone.
GROUP_PLANS are (W, NWT) = (84, 12) and (128, 12); every other pair of the variant: tests/test_gpu_floor_variant_grid.py."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

GROUP_PLANS = ["jdc722", "jdc721", "imm722w", "durrieu722", "durrieu721"]
EDGE_LENS = np.array([1, 2, 63, 64, 65, 127, 128, 129, 193, 700, 1], np.int64)
GEN = {"peaks": synth.emissions_peaks, "dense": synth.emissions_dense}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _params(golden, name):
    return golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]


def _scan_only_jdc722(golden):
    """jdc722 with one in-window entry below its row's constant (tests/test_gpu_ckpt_group.py): banded, the floor form not proven."""
    A = np.array(golden["params"]["jdc722_logA_T"], np.float32, copy=True)
    vals, counts = np.unique(A[300], return_counts=True)
    A[300, 303] = np.float32(vals[np.argmax(counts)]) - np.float32(5)
    return A, golden["params"]["jdc722_log_pi"]


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


@pytest.mark.parametrize("kind,dt", [("peaks", torch.float32), ("dense", torch.float16)], ids=["peaks-f32", "dense-f16"])
@pytest.mark.parametrize("name", GROUP_PLANS)
def test_bit_equality_at_the_segment_edges(golden, dev, name, dt, kind):
    """Recordings of 1, 2, 63, 64, 65, 127, 128, 129, 193, 700 and 1 frames in one buffer, segments of 64 frames: a single frame, no
    checkpoint, a checkpoint exactly at the end (which must NOT be stored: the row behind a recording's last checkpoint is the next
    recording's first), one frame into a new segment.  Then segments of 128 frames, and of 4096 (every recording is one segment).
    States and log-likelihood bits of decode_packed and of the oracle, for every recording."""
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    assert not dec.info["wave_ok"]
    E = GEN[kind](len(EDGE_LENS), 700, dec.S, seed=21, device=dev, dtype=dt)
    ref_s, ref_l = vo.decode_c(A, pi, E.float().cpu().numpy(), lengths=EDGE_LENS)
    Ep, off = _pack(E, EDGE_LENS)
    want_s, want_l = dec.decode_packed(Ep, off, out_dtype=torch.int32)
    _assert_matches_oracle(want_s, want_l, off, ref_s, ref_l, (name, kind, dt, "decode_packed"))
    for K in (64, 128, 4096):
        st, ll = dec.decode_packed_bounded(Ep, off, segment_frames=K, out_dtype=torch.int32)
        assert st.dtype == torch.int32 and st.shape == want_s.shape and ll.shape == want_l.shape
        assert torch.equal(st, want_s) and np.array_equal(_bits(ll), _bits(want_l)), (name, kind, dt, K)
        _assert_matches_oracle(st, ll, off, ref_s, ref_l, (name, kind, dt, K))
    st64, _ = dec.decode_packed_bounded(Ep, torch.from_numpy(off), segment_frames=64)       # offsets as a tensor, int64 states
    assert st64.dtype == torch.int64 and torch.equal(st64, want_s.to(torch.int64))


@pytest.mark.parametrize("name", ["jdc722", "durrieu722"])
def test_more_units_than_a_launch_takes(golden, dev, name):
    """52 recordings more than a launch of pass 2 takes units, 65 .. 130 frames each, and one of 700; segments of 64 frames, fp16.
    Launches hold fewer units than are ready; the long recording keeps total frames / longest small (few pass-1 slots, each walking
    several recordings) and goes on for eleven launches.  Equal to decode_packed on every recording, to the oracle on eight: the
    shortest, the longest, two of 128 frames (a multiple of the segment length) and four more."""
    lib = _lib.load()
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    S, K, NU, TL = dec.S, 64, 16, 700
    per_launch = int(lib.vit_packed_bounded_units(dec._plan, 1 << 30))
    n_cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert per_launch == (1 if name == "jdc722" else 2) * n_cus
    B = per_launch + 52
    rng = np.random.default_rng(77)
    lens = rng.integers(65, 131, B).astype(np.int64)
    lens[[0, 1, 2, 3, B - 1]] = (65, 128, TL, 130, 128)
    base = synth.emissions_peaks(NU, TL, S, seed=91, device=dev, dtype=torch.float16)        # recording b holds song b % NU, lengths differ
    base[NU // 2:] = synth.emissions_dense(NU - NU // 2, TL, S, seed=92, device=dev, dtype=torch.float16)
    off = _offsets(lens)
    song = torch.from_numpy(np.repeat(np.arange(B) % NU, lens)).to(dev)
    frame = torch.from_numpy(np.concatenate([np.arange(n) for n in lens])).to(dev)
    Ep = base[song, frame].contiguous()
    assert Ep.shape == (int(off[-1]), S)
    assert int(off[-1]) // TL < B, "pass-1 slots must walk several recordings"
    want_s, want_l = dec.decode_packed(Ep, off, out_dtype=torch.int32)
    st, ll = dec.decode_packed_bounded(Ep, off, segment_frames=K, out_dtype=torch.int32)
    assert torch.equal(st, want_s) and np.array_equal(_bits(ll), _bits(want_l))
    picks = np.array([0, 1, 2, 3, B - 1, 5, 6, 7])
    assert lens[picks].min() == lens.min() and lens[picks].max() == lens.max() and (lens[picks] == 128).any()
    ref_s, ref_l = vo.decode_c(A, pi, base[picks % NU].float().cpu().numpy(), lengths=lens[picks])
    st, ll = st.cpu().numpy(), ll.cpu().numpy()
    for k, b in enumerate(picks):
        assert np.array_equal(st[off[b]:off[b + 1]], ref_s[k, :lens[b]]), (b, int(lens[b]))
        assert ll[b:b + 1].view(np.int32) == ref_l[k:k + 1].view(np.int32), b


@pytest.mark.parametrize("name", ["jdc722", "durrieu722"])
def test_stays_inside_its_workspace(golden, dev, name):
    """A caller-owned workspace of exactly workspace_bytes_packed_bounded + 256 bytes, between 1 MB of guard bytes on either side,
    everything filled with 0xFF (NaN patterns): the oracle's result, guards intact, a second call returns identical bytes.  One byte
    less is refused before anything runs.  The size on THIS device: units x (K + 2 | K + 1) + sum (n_b - 1) + slots rows of (S + 5) /
    4 * 4 floats, units = vit_packed_bounded_units, slots = min(B, 8 x compute units), plus tables."""
    lib = _lib.load()
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    lens = np.concatenate([EDGE_LENS, [1000, 333]]).astype(np.int64)
    E = synth.emissions_peaks(len(lens), 1000, dec.S, seed=4, device=dev)
    ref_s, ref_l = vo.decode_c(A, pi, E.cpu().numpy(), lengths=lens)
    Ep, off = _pack(E, lens)
    G = 1 << 20
    B = len(lens)
    units = int(lib.vit_packed_bounded_units(dec._plan, B))
    assert units == B
    sd, extra = (dec.S + 5) // 4 * 4, 2 if name == "jdc722" else 1
    for K in (64, 100, 640):
        assert lens.max() > K
        need = dec.workspace_bytes_packed_bounded(off, K)
        nseg = (lens + K - 1) // K
        rows = units * (K + extra) + int((nseg - 1).sum()) + B
        assert rows * sd * 4 <= need <= rows * sd * 4 + 24 * B + 8 * int(nseg.sum()) + 152 * B + 16 * 256
        buf = torch.full((G + 256 + need + 256 + G,), 0xFF, dtype=torch.uint8, device=dev)
        o = G + (-(buf.data_ptr() + G)) % 256                                # first 256-byte aligned address behind the front guard
        ws = buf[o:o + need + 256]
        assert ws.data_ptr() % 256 == 0
        first = None
        for _ in range(2):
            st, ll = dec.decode_packed_bounded(Ep, off, segment_frames=K, out_dtype=torch.int32, workspace=ws)
            torch.cuda.synchronize()
            _assert_matches_oracle(st, ll, off, ref_s, ref_l, (name, K))
            if first is not None:
                assert torch.equal(st, first[0]) and np.array_equal(_bits(ll), _bits(first[1])), K
            first = (st, ll)
        assert bool((buf[:o] == 0xFF).all()), (K, "bytes in front of the workspace were written")
        assert bool((buf[o + need:] == 0xFF).all()), (K, "bytes behind the workspace were written")
        with pytest.raises(ValueError):
            dec.decode_packed_bounded(Ep, off, segment_frames=K, workspace=ws[:need + 255])
        st = torch.full((int(off[-1]),), 12345, dtype=torch.int32, device=dev)
        ll = torch.full((B,), 7.0, dtype=torch.float32, device=dev)
        args = (dec._plan, Ep.data_ptr(), _lib.VIT_F32, B, off.ctypes.data, ws.data_ptr())
        assert lib.vit_decode_packed_bounded(*args, need - 1, st.data_ptr(), ll.data_ptr(), K, None) == -4      # VIT_EWORKSPACE
        torch.cuda.synchronize()
        assert bool((st == 12345).all()) and bool((ll == 7.0).all())
        assert lib.vit_decode_packed_bounded(*args, need, st.data_ptr(), ll.data_ptr(), K, None) == 0
        torch.cuda.synchronize()
        _assert_matches_oracle(st, ll, off, ref_s, ref_l, (name, K, "C ABI"))


def test_refusals_are_loud_and_early(golden, dev):
    """An unstructured matrix and a scan-only banded plan get size 0, ViterbiHipError and VIT_EUNSUPPORTED; a segment length out of
    range and bad offsets VIT_EINVAL.  Nothing is enqueued in any of these cases: `states` and `loglik` keep their sentinels."""
    lib = _lib.load()
    lens = np.array([100, 200, 65], np.int64)
    off = _offsets(lens)

    def call(dec, E, K, offsets=off, B=None):
        st = torch.full((int(off[-1]),), 12345, dtype=torch.int32, device=dev)
        ll = torch.full((len(lens),), 7.0, dtype=torch.float32, device=dev)
        ws = torch.empty((1 << 26) + 256, dtype=torch.uint8, device=dev)
        offsets = np.asarray(offsets, np.int64)
        rc = lib.vit_decode_packed_bounded(dec._plan, E.data_ptr(), _lib.VIT_F32, len(offsets) - 1 if B is None else B, offsets.ctypes.data,
                                           (ws.data_ptr() + 255) & ~255, 1 << 26, st.data_ptr(), ll.data_ptr(), K, None)
        torch.cuda.synchronize()
        assert bool((st == 12345).all()) and bool((ll == 7.0).all()), "a refused call wrote its outputs"
        return rc

    for what, (A, pi) in (("dense97", _params(golden, "dense97")), ("scan-only jdc722", _scan_only_jdc722(golden))):
        dec = ViterbiDecoder(A, pi, dev)
        E = synth.emissions_dense(1, int(off[-1]), dec.S, seed=1, device=dev)[0].contiguous()
        assert int(lib.vit_workspace_bytes_packed_bounded(dec._plan, 3, off.ctypes.data, 64)) == 0, what
        assert int(lib.vit_packed_bounded_units(dec._plan, 3)) == 0, what
        with pytest.raises(_lib.ViterbiHipError):
            dec.workspace_bytes_packed_bounded(off, 64)
        with pytest.raises(_lib.ViterbiHipError):
            dec.decode_packed_bounded(E, off, segment_frames=64)
        with pytest.raises(_lib.ViterbiHipError):
            dec.plan_workspace_packed_bounded(off, 1000)
        assert call(dec, E, 64) == -5, what                                   # VIT_EUNSUPPORTED
    for name in ("jdc722", "durrieu722"):
        dec = ViterbiDecoder(*_params(golden, name), dev)
        E = synth.emissions_dense(1, int(off[-1]), dec.S, seed=1, device=dev)[0].contiguous()
        for K in (63, (1 << 24) + 1, 0, -5):
            assert int(lib.vit_workspace_bytes_packed_bounded(dec._plan, 3, off.ctypes.data, K)) == 0, K
            assert call(dec, E, K) == -1, K                                   # VIT_EINVAL
            with pytest.raises(_lib.ViterbiHipError):
                dec.decode_packed_bounded(E, off, segment_frames=K)
        for bad in ([1, 100, 300, 365], [0, 100, 100, 365], [0, 300, 100, 365]):  # not from 0, an empty recording, decreasing
            assert call(dec, E, 64, offsets=bad) == -1, bad
            assert int(lib.vit_workspace_bytes_packed_bounded(dec._plan, 3, np.asarray(bad, np.int64).ctypes.data, 64)) == 0
            with pytest.raises(ValueError):
                dec.decode_packed_bounded(E, bad, segment_frames=64)
        assert lib.vit_decode_packed_bounded(dec._plan, E.data_ptr(), 7, 3, off.ctypes.data, 256, 1 << 26, 256, None, 64, None) == -1    # dtype
        assert lib.vit_decode_packed_bounded(dec._plan, E.data_ptr(), 0, 3, None, 256, 1 << 26, 256, None, 64, None) == -1              # offsets
        assert call(dec, E, 64, offsets=[0], B=0) == 0                        # nothing to do


def test_wave_form_plans_forward(golden, dev):
    """tonet361: decode_packed_bounded returns the bits of decode_packed_checkpointed, from a workspace of the same size."""
    A, pi = _params(golden, "tonet361")
    dec = ViterbiDecoder(A, pi, dev)
    E = synth.emissions_peaks(len(EDGE_LENS), 700, dec.S, seed=21, device=dev)
    Ep, off = _pack(E, EDGE_LENS)
    for K in (64, 128):
        assert dec.workspace_bytes_packed_bounded(off, K) == dec.workspace_bytes_packed_checkpointed(off, K)
        want_s, want_l = dec.decode_packed_checkpointed(Ep, off, segment_frames=K, out_dtype=torch.int32)
        st, ll = dec.decode_packed_bounded(Ep, off, segment_frames=K, out_dtype=torch.int32)
        assert torch.equal(st, want_s) and np.array_equal(_bits(ll), _bits(want_l)), K


@pytest.mark.parametrize("name", ["jdc722", "durrieu722"])
def test_budget_policy(golden, dev, name):
    """decode_packed(max_workspace_bytes=...) over shrinking budgets on one ragged set: "full" while the history fits, then
    "checkpointed" with a segment length that never grows and a size within the budget; identical bits under every budget; a budget
    below the smallest need raises and names it."""
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    lens = np.array([4100, 1, 2, 1500, 4099, 3, 2049, 65, 4096], np.int64)
    E = synth.emissions_peaks(len(lens), 4100, dec.S, seed=3, device=dev, dtype=torch.float16)
    Ep, off = _pack(E, lens)
    del E
    full = dec.workspace_bytes_packed(len(lens), int(off[-1]))
    needs = {K: dec.workspace_bytes_packed_bounded(off, K) for K in (8192, 4096, 2048, 1024, 512, 256, 128, 64)}
    least = min(needs.values())
    assert least == needs[64] < full // 9
    want_s, want_l = dec.decode_packed(Ep, off, out_dtype=torch.int32)
    seen, Ks = [], []
    for budget in (None, 2 * full, full, full - 1, full // 2, full // 3, full // 5, full // 9, needs[64]):
        mode = dec.plan_workspace_packed_bounded(off, budget)
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
    with pytest.raises(_lib.ViterbiHipError, match=str(least)):
        dec.decode_packed(Ep, off, max_workspace_bytes=least - 1)
    with pytest.raises(_lib.ViterbiHipError, match=str(least)):
        dec.plan_workspace_packed_bounded(off, 1000)


def test_imm_recordings_under_a_budget(dev):
    """ImmViterbi.decode_activations_recordings(list, max_workspace_bytes=tight), the step plan of the Durrieu matrix: the states of
    the call without a budget, on every recording; a budget below the least need raises."""
    from viterbi_spl_amd import ImmViterbi
    v = ImmViterbi(20, 721, device=dev)
    rlens = [257, 1, 64, 300, 2, 129]
    xs = [synth.hf0_activations(721, n, seed=40 + k, device=dev) for k, n in enumerate(rlens)]
    roff = _offsets(rlens)
    tight = v._decoder.workspace_bytes_packed_bounded(roff, 64)
    assert v._decoder.plan_workspace_packed_bounded(roff, tight) == {"mode": "checkpointed", "segment_frames": 64, "workspace_bytes": tight}
    got, want = v.decode_activations_recordings(xs, max_workspace_bytes=tight), v.decode_activations_recordings(xs)
    assert len(got) == len(want) == len(rlens)
    for k in range(len(rlens)):
        assert got[k].dtype == torch.int64 and got[k].shape == (rlens[k],) and torch.equal(got[k], want[k]), k
    with pytest.raises(_lib.ViterbiHipError):
        v.decode_activations_recordings(xs, max_workspace_bytes=tight - 1)
