"""GPU tests of the emission builders with float16 storage (viterbi_spl_amd/csrc/emission_half.hip, vit_obs_build): float32 logits ->
float16 emissions, float16 -> float32 and float16 -> float16, and of the float16 snippet hand-off (vit_snippets_append_f16).

The contract is bitwise and needs no tolerance: a float16 logit is widened exactly at the load, the arithmetic is the float32
builder's, the float32 result is rounded to nearest even at the store.  So every typed launch is compared, as bit patterns, with
the float32 builder (which tests/test_gpu_builders.py pins to oracle/observation_oracle.py) on ``logits.float()``, followed by
torch's ``.half()`` where the emissions are float16.  Every output lies in a poisoned arena (tests/guarded.py) whose bytes outside
the rows must stay what they were: a float16 row is 2 * S bytes, so with an odd S every other row starts off a 4-byte boundary, and
a packed store that is one half too wide lands in the next row or behind the buffer.

Non-vacuity (conditions on the INPUTS, asserted on the GPU's float32 rows; a test that trips them has lost its inputs, not found a
bug): every float16-emission case holds at least one value that ``.half()`` keeps as a nonzero subnormal (|v| < 2^-14: a flush
would show) and one that rounds away from zero (|half(v)| > |v|: a toward-zero conversion would show).  The planted frames below
supply the subnormals -- log p of a dominant peak -- in modes 0, 1 and 2 without a prior; with a prior mode 2's rows are
log(p / prior), which the planted frames put near +5.6, not near 0, so a mode-2 case runs with AND without its prior and the
subnormal condition is asked of the pair; the rounding-direction condition is asked of every launch on its own."""
import numpy as np
import pytest
import torch

from tests.common import logits_case
from tests.far_offsets import VTH2, builder_prior
from tests.guarded import Arena, assert_intact
from viterbi_spl_amd import _lib, synth
from viterbi_spl_amd import emissions as em
from viterbi_spl_amd import reference_api as ra

pytestmark = pytest.mark.gpu

F32, F16 = torch.float32, torch.float16
COMBOS = [(F32, F16), (F16, F32), (F16, F16)]
COMBO_IDS = ["f32-f16", "f16-f32", "f16-f16"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def n_cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _register_form(U, spw):
    return spw in (5, 15) and U > 64 and U > 2 * spw


def _fstep(U, spw, n_cus):
    """Frames between a wave's consecutive frames at full size (launch_obs: eight workgroups of four waves per CU in the register
    form, six in the LDS form)."""
    return (32 if _register_form(U, spw) else 24) * n_cus


def _gpu(mode, x, spw, prior=None, out=None, dtype=F32):
    if mode == 0:
        return em.shaun_log_emissions(x, single_side_peak_width=spw, out=out, dtype=dtype)
    if mode == 1:
        return em.softmax_log_emissions(x, single_side_peak_width=spw, out=out, dtype=dtype)
    return em.softmax_scaled_log_emissions(x, VTH2, prior, single_side_peak_width=spw, out=out, dtype=dtype)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)


def _rounding_frames(U, mode, spw):
    """16 frames f = 0 .. 15: a dominant peak at logit +12, a second peak 9 + f / 2 nats below it, background -30; in mode 1 the
    unvoiced column 10 + f / 2 below the top.  Every value is a float16 number.  log p of the dominant peak is -e^-(9 + f / 2) and
    smaller: 13-14 float32 emissions per 16 frames with 0 < |v| < 2^-14 on the CPU oracle (modes 0, 1, 2 without a prior).  The two
    peaks sit a third and two thirds into the row, moved where a short row needs it: past the bins that are never a peak
    (1 .. spw // 2) and more than spw apart."""
    x = np.full((16, U), -30.0, np.float32)
    f = np.arange(16, dtype=np.float32)
    a = max(U // 3, spw // 2 + 1)
    b = max((2 * U) // 3, a + spw + 1)
    assert b < U
    x[:, a] = 12.0
    x[:, b] = 12.0 - (9.0 + f / 2)
    if mode == 1:
        x = np.concatenate([(12.0 - (10.0 + f / 2))[:, None].astype(np.float32), x], axis=1)
    assert np.array_equal(x.astype(np.float16).astype(np.float32), x)
    return x


def _in_arena(dev, array, lead_elems):
    """A host array in a poisoned arena, `lead_elems` elements past a 256-byte boundary -> (arena, typed device view)."""
    a = Arena(array.nbytes, dev, lead=lead_elems * array.itemsize)
    return a, a.store(array)


def _out_arena(dev, n, S, dtype, lead_elems):
    item = 2 if dtype == F16 else 4
    a = Arena(n * S * item, dev, lead=lead_elems * item)
    return a, a.view(dtype, (n, S))


def _check_case(dev, mode, x, spw, priors, lt, et, leads, what):
    """One geometry in one dtype combination.  x: float32 host logits (rounded to float16 here when lt is float16).  priors: the
    priors to run with (mode 2: [None, prior]; otherwise [None]).  leads: (logits lead, out lead) pairs in elements.  Returns
    nothing; asserts the bitwise contract, the arenas and the non-vacuity conditions."""
    U = x.shape[1] - (mode == 1)
    n = x.shape[0]
    xs = x.astype(np.float16) if lt == F16 else x
    wide = torch.from_numpy(xs.astype(np.float32)).to(dev)
    sub = False
    for prior in priors:
        pd = torch.from_numpy(prior).to(dev) if prior is not None else None
        want32 = _gpu(mode, wide, spw, pd)
        want = want32.half() if et == F16 else want32
        if et == F16:
            h = want.float()
            sub = sub or bool(((h != 0) & (h.abs() < 2.0 ** -14)).any())
            assert bool((h.abs() > want32.abs()).any()), f"{what} prior {prior is not None}: the inputs give no emission that rounds away from zero"
        for lead_in, lead_out in leads:
            ain, xd = _in_arena(dev, xs, lead_in)
            aout, out = _out_arena(dev, n, U + 1, et, lead_out)
            got = _gpu(mode, xd, spw, pd, out=out, dtype=et)
            torch.cuda.synchronize()
            assert got.data_ptr() == out.data_ptr() and got.dtype == et
            bad = (_bits(got) != _bits(want)).any(dim=1).nonzero().flatten()
            assert bad.numel() == 0, (f"{what} prior {prior is not None} leads {lead_in, lead_out}: {bad.numel()} rows differ from the "
                                      f"float32 builder, first {bad[:8].tolist()}")
            assert_intact(aout, f"{what}: emissions")
            assert_intact(ain, f"{what}: logits")
    if et == F16:
        assert sub, f"{what}: the inputs give no emission that float16 keeps as a nonzero subnormal"


# ---- 1. full launch size -------------------------------------------------------------------------------------------------
FULL_CASES = [("reg", 0, 360, 5), ("reg", 1, 721, 15), ("reg", 2, 320, 5), ("reg", 0, 500, 15), ("lds", 0, 360, 3), ("lds", 1, 721, 31)]


@pytest.mark.parametrize("lt,et", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("form,mode,U,spw", FULL_CASES, ids=[f"{c[0]}-mode{c[1]}-U{c[2]}-spw{c[3]}" for c in FULL_CASES])
def test_full_launch_size(dev, n_cus, form, mode, U, spw, lt, et):
    """n = 160 * n_cus + 3 frames: at the launch cap every wave walks ~5 frames, the register form's rolling prefetch of both
    register sets runs (past 4 * 32 * n_cus frames), the last pass of some waves skips its second set.  The rounding frames are
    planted at fstep, 2 * fstep and the end.  Bit-equal to the float32 builder on the widened logits (rounded with .half() for
    float16 emissions); the rows past n and the bytes in front of row 0 keep their poison.  Mode 2 runs with and without its prior."""
    assert _register_form(U, spw) == (form == "reg")
    fstep = _fstep(U, spw, n_cus)
    n = 160 * n_cus + 3
    assert n > 4 * 32 * n_cus and n > 2 * fstep + 16
    x = logits_case(U + 7 * spw + mode, n, U + (mode == 1))
    sp = _rounding_frames(U, mode, spw)
    for at in (fstep, 2 * fstep, n - len(sp)):
        x[at:at + len(sp)] = sp
    priors = [None, builder_prior(U)] if mode == 2 else [None]
    _check_case(dev, mode, x, spw, priors, lt, et, [(0, 0)], f"full size mode {mode} U {U} spw {spw}")


# ---- 2. instantiation edges ----------------------------------------------------------------------------------------------
EDGE_CASES = [(m, U, spw) for m in (0, 1, 2) for spw in (5, 15) for U in (64, 65, 66, 320, 321, 384, 385, 512, 513, 767, 768)] + \
             [(m, 30, 15) for m in (0, 1, 2)]


@pytest.mark.parametrize("lt,et", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("mode,U,spw", EDGE_CASES)
def test_instantiation_edges(dev, mode, U, spw, lt, et):
    """The bins-per-lane boundaries of the register form (5 / 6 / 8 / 12 bins: U = 320 | 321, 384 | 385, 512 | 513, 768), partial
    last lanes, the smallest register-form rows and the LDS fall-back (U = 64; U = 30 with half-width 15), odd and even S: 64 frames,
    the rounding frames first.  Each case runs with its buffers on a 256-byte boundary and a second time with every float16 buffer
    starting at an ODD element (2 bytes past the boundary: no row of an even S, and every other row of an odd S, is 4-byte aligned
    then); float32 buffers move by one element as well.  Poison on both sides of logits and emissions."""
    x = logits_case(U + spw + mode, 64, U + (mode == 1))
    x[:16] = _rounding_frames(U, mode, spw)
    priors = [None, builder_prior(U)] if mode == 2 else [None]
    _check_case(dev, mode, x, spw, priors, lt, et, [(0, 0), (1, 1)], f"edges mode {mode} U {U} spw {spw}")


# ---- 3. the rounding cases are in the inputs --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,U,spw", [(0, 360, 5), (0, 360, 3), (1, 721, 15), (2, 320, 5)])
def test_rounding_frames_reach_float16_subnormals(dev, mode, U, spw):
    """What the planted frames are for, on the float32 builder's own rows: at least 13 of their emissions lie in (0, 2^-14) in
    magnitude and survive .half() as nonzero subnormals; logits_case frames hold values whose nearest-even and toward-zero roundings
    differ (hundreds per 64 frames)."""
    x = torch.from_numpy(_rounding_frames(U, mode, spw)).to(dev)
    v = _gpu(mode, x, spw)
    small = (v != 0) & (v.abs() < 2.0 ** -14)
    assert int(small.sum()) >= 13, int(small.sum())
    assert int(((v.half() != 0) & small).sum()) >= 13
    y = _gpu(mode, torch.from_numpy(logits_case(U + spw + mode, 64, U + (mode == 1))).to(dev), spw)
    assert int((y.half().float().abs() > y.abs()).sum()) >= 100


# ---- 4. refusals and empty launches ---------------------------------------------------------------------------------------
def test_refusals_and_empty_launches(dev):
    """vit_obs_build: a bad dtype code, a bad mode and null pointers are VIT_EINVAL; the geometries no kernel serves (more than 768
    bins, half-width 0, >= U, > 64) are refused in every dtype combination, the float32 pair included, and leave a poisoned `out`
    untouched; zero frames return an empty result; out= of another dtype than dtype= raises ValueError."""
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    x = torch.zeros((4, 360), device=dev)
    o = torch.zeros((4, 361), device=dev)
    obs = _lib.ObsParams(0, 360, 5, 0.0, 0.0, 2.0, None)
    assert lib.vit_obs_build(obs, x.data_ptr(), _lib.VIT_F32, 4, o.data_ptr(), _lib.VIT_F32, stream) == _lib.VIT_OK
    for ld, ed in ((2, 0), (0, 2), (-1, 1), (1, 7)):
        assert lib.vit_obs_build(obs, x.data_ptr(), ld, 4, o.data_ptr(), ed, stream) == -1
    for ld in (_lib.VIT_F32, _lib.VIT_F16):
        for ed in (_lib.VIT_F32, _lib.VIT_F16):
            assert lib.vit_obs_build(obs, None, ld, 4, o.data_ptr(), ed, stream) == -1
            assert lib.vit_obs_build(obs, x.data_ptr(), ld, 4, None, ed, stream) == -1
            assert lib.vit_obs_build(None, x.data_ptr(), ld, 4, o.data_ptr(), ed, stream) == -1
            assert lib.vit_obs_build(obs, x.data_ptr(), ld, -1, o.data_ptr(), ed, stream) == -1
            assert lib.vit_obs_build(obs, None, ld, 0, None, ed, stream) == _lib.VIT_OK
            for bad_mode in (-1, 3):
                assert lib.vit_obs_build(_lib.ObsParams(bad_mode, 360, 5, 0.0, 0.0, 2.0, None), x.data_ptr(), ld, 4, o.data_ptr(), ed, stream) == -1
    for lt, et in COMBOS + [(F32, F32)]:
        for mode in (0, 1, 2):
            for U, spw in ((769, 5), (360, 0), (360, 360), (100, 100), (360, 65)):
                xd = torch.zeros((4, U + (mode == 1)), device=dev, dtype=lt)
                arena, out = _out_arena(dev, 4, U + 1, et, 0)
                with pytest.raises(_lib.ViterbiHipError):
                    _gpu(mode, xd, spw, out=out, dtype=et)
                torch.cuda.synchronize()
                assert arena.poisoned(), (lt, et, mode, U, spw, "a refused call wrote")
            for shape in ((0, 360), (2, 0, 360)):
                xd = torch.zeros(shape[:-1] + (360 + (mode == 1),), device=dev, dtype=lt)
                got = _gpu(mode, xd, 5, dtype=et)
                assert tuple(got.shape) == shape[:-1] + (361,) and got.dtype == et
    x16 = x.half()
    for xin in (x, x16):
        with pytest.raises(ValueError):
            em.shaun_log_emissions(xin, out=torch.empty((4, 361), device=dev, dtype=F32), dtype=F16)
        with pytest.raises(ValueError):
            em.shaun_log_emissions(xin, out=torch.empty((4, 361), device=dev, dtype=F16))
        with pytest.raises(ValueError):
            em.softmax_scaled_log_emissions(xin, VTH2, None, out=torch.empty((4, 361), device=dev, dtype=F16), dtype=F32)
        with pytest.raises(ValueError):
            em.shaun_log_emissions(xin, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        em.softmax_log_emissions(torch.zeros((4, 361), device=dev, dtype=torch.bfloat16))


# ---- 5. the snippet hand-off ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["Viterbi", "SoftMaxViterbi"])
def test_recording_accumulator_float16_snippets(dev, cls):
    """RecordingAccumulator.append with float16 snippets (vit_snippets_append_f16), the shapes of
    test_gpu_builders.py::test_recording_accumulator_partial_tiles: rows bit-equal to appending ``snippets.float()`` (the "shaun"
    subtraction of channel 0 is a float32 subtraction of the widened values) and to the host's transpose, nothing written past the
    rows held."""
    n_bins = 321
    vit = getattr(ra, cls)(synth.tonet_transition(n_bins, 14), synth.floored_prior(n_bins + 1), device=dev)
    acc, ref = ra.RecordingAccumulator(vit, max_frames=20000), ra.RecordingAccumulator(vit, max_frames=20000)
    acc._rows.fill_(float("nan"))
    rng = np.random.default_rng(11)
    host = []
    for n, F, padded in ((3, 1, 0), (70, 63, 13), (7, 65, 1), (5, 100, 30), (70, 65, 0), (2, 100, 0), (1, 63, 62), (4, 100, 99)):
        b = rng.normal(-6, 2, (n, acc.channels, F)).astype(np.float16)
        bd = torch.from_numpy(b).to(dev)
        acc.append(bd, padded)
        ref.append(bd.float(), padded)
        lg = np.transpose(b.astype(np.float32), [0, 2, 1])
        lg = (lg[..., 1:] - lg[..., :1]).reshape(-1, n_bins) if cls == "Viterbi" else lg.reshape(-1, acc.channels)
        host.append(lg[:len(lg) - padded])
        torch.cuda.synchronize()
        assert torch.isnan(acc._rows[acc.n_frames:]).all(), (n, F, padded, "a row past the recording was written")
    host = np.concatenate(host, axis=0)
    assert acc.n_frames == ref.n_frames == len(host)
    assert acc.logits().dtype == F32
    assert torch.equal(acc.logits().view(torch.int32), ref.logits().view(torch.int32))
    assert acc.logits().cpu().numpy().tobytes() == host.tobytes()
    with pytest.raises(ValueError):
        acc.append(torch.zeros((1, acc.channels, 4), device=dev, dtype=torch.bfloat16))
