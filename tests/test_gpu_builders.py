"""GPU tests of the emission builders (viterbi_spl_amd/csrc/emission.hip) where the other builder tests do not reach: full launch
size (every wave walks many frames, both register sets of the register form roll), the edges of every instantiation, and the float32
range edge of exp (subnormal probabilities); plus the hand-off kernels beside them (voicing map / notes, snippet append) beyond one
grid pass or tile.  Reference: oracle/observation_oracle.py, pinned to the reference's builders by tests/test_oracle.py.
Bar: the same structural log(tiny) set, probabilities within rtol 1e-5 (modes 0 and 1), log-likelihoods within 2e-5 (mode 2)."""
import os

import numpy as np
import pytest
import torch

from tests.common import RANGE_SPANS, RANGE_TOPS, logits_case, range_edge_logits
# (the oracle side of the comparison and its bar are shared with tests/test_gpu_far_offsets_rows.py)
from tests.far_offsets import FLOOR, TINY, VTH2, assert_builder_matches as _assert_matches, builder_oracle as _oracle, builder_prior as _prior
from viterbi_spl_amd import ViterbiDecoder, _lib, synth
from viterbi_spl_amd import emissions as em
from viterbi_spl_amd import reference_api as ra

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


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
    """Frames between a wave's consecutive frames at full size: launch_obs caps the register form's grid at eight workgroups of four
    waves per CU, the LDS form's at six."""
    return (32 if _register_form(U, spw) else 24) * n_cus


def _gpu(mode, x, spw, prior=None, out=None):
    """The GPU builder of `mode` on device logits -> log-emissions [n, U+1]."""
    if mode == 0:
        return em.shaun_log_emissions(x, single_side_peak_width=spw, out=out)
    if mode == 1:
        return em.softmax_log_emissions(x, single_side_peak_width=spw, out=out)
    assert out is None
    return em.softmax_scaled_log_emissions(x, VTH2, prior, single_side_peak_width=spw)


def _special_frames(U, spw, mode, rng):
    """16 frames where a builder goes wrong: a constant frame, the maximum at bin 0 (left-end rule), at bins 1 and spw // 2 (never
    a peak), at U - 1, quantised ties (the FIRST maximum of a window is the peak), a peak every spw + 1 bins (more than 64 when the
    row allows: two rounds of the compaction), and eight range-edge frames (tests.common.range_edge_logits).  [16, U (+1 in mode 1)]"""
    def noise():
        return (rng.standard_normal(U) * 3).astype(np.float32)
    fr = [np.full(U, 1.5, np.float32)]
    for b in (0, 1, max(1, spw // 2), U - 1):
        x = noise()
        x[b] = x.max() + 3
        fr.append(x)
    fr.append(np.round(noise()))
    fr.append(np.round(noise() / 4))
    x = np.float32(-30) - (np.arange(U) % (spw + 1)).astype(np.float32)
    x[::spw + 1] = noise()[::spw + 1]
    fr.append(x)
    x = np.stack(fr)
    if mode == 1:
        x = np.concatenate([(rng.standard_normal((len(x), 1)) * 3).astype(np.float32), x], axis=1)
    r = range_edge_logits(U, spw, RANGE_TOPS + RANGE_SPANS if mode == 2 else RANGE_TOPS, unvoiced_column=mode == 1)
    x = np.concatenate([x, r[np.linspace(0, len(r) - 1, 16 - len(x)).round().astype(int)]])
    assert x.shape == (16, U + (mode == 1))
    return np.ascontiguousarray(x, np.float32)


# ---- 1. full launch size: every frame of a wave after its first, both register sets rolling ----------------------------------
FULL_CASES = ([("reg", m, U, spw, False) for m in (0, 1) for U in (320, 360, 500, 721) for spw in (5, 15)]
              + [("reg", 2, U, 5, pr) for U in (320, 360, 721) for pr in (False, True)]
              + [("lds", m, U, spw, m == 2) for m in (0, 1, 2) for U in (360, 721) for spw in (3, 31)])


@pytest.mark.parametrize("form,mode,U,spw,with_prior", FULL_CASES, ids=[f"{c[0]}-mode{c[1]}-U{c[2]}-spw{c[3]}{'-prior' if c[4] else ''}" for c in FULL_CASES])
def test_full_launch_size(dev, n_cus, form, mode, U, spw, with_prior):
    """n = 160 * n_cus + 3 frames: at the launch cap every wave walks ~5 (register form: ~2.5 per register set) frames, the last pass
    of some waves skips its second set.  (1) the launch equals, bit for bit, 256-frame launches of the same rows (one frame per
    wave: the builders compute every frame on its own); (2) ~600 sampled rows - the pass boundaries, the planted frames, the last
    rows - against the oracle; (3) written through out= into a NaN-filled larger buffer, the rows past n stay NaN."""
    assert _register_form(U, spw) == (form == "reg")
    fstep = _fstep(U, spw, n_cus)
    n = 160 * n_cus + 3
    assert n > 4 * 32 * n_cus and n > 2 * fstep + 16          # the rolling prefetch of both register sets runs
    rng = np.random.default_rng(1000 * mode + U + spw)
    x = logits_case(U + 7 * spw + mode, n, U + (mode == 1))
    sp = _special_frames(U, spw, mode, rng)
    planted = []
    for at in (2 * fstep, fstep, n - len(sp)):
        x[at:at + len(sp)] = sp
        planted += range(at, at + len(sp))
    prior = _prior(U) if with_prior else None
    prior_dev = torch.from_numpy(prior).to(dev) if with_prior else None
    xd = torch.from_numpy(x).to(dev)
    if mode < 2:
        buf = torch.full((n + 37, U + 1), float("nan"), device=dev)
        big = _gpu(mode, xd, spw, out=buf[:n])
        assert big.data_ptr() == buf.data_ptr()
    else:
        big = _gpu(mode, xd, spw, prior_dev)
    small = torch.empty_like(big)
    for i in range(0, n, 256):
        if mode < 2:
            _gpu(mode, xd[i:i + 256], spw, out=small[i:i + 256])
        else:
            small[i:i + 256] = _gpu(mode, xd[i:i + 256], spw, prior_dev)
    torch.cuda.synchronize()
    diff = (big.view(torch.int32) != small.view(torch.int32)).any(dim=1).nonzero().flatten()
    assert diff.numel() == 0, f"full-size launch differs from 256-frame launches in {diff.numel()} rows, first {diff[:8].tolist()} (fstep {fstep})"
    if mode < 2:
        assert torch.isnan(buf[n:]).all(), "a row past n_frames was written"
    rows = {0, 1, n - 3, n - 2, n - 1} | {k * fstep + j for k in range(n // fstep + 1) for j in (-1, 0, 1)} | set(planted)
    rows = {r for r in rows if 0 <= r < n}
    rows |= set(rng.choice(n, 600 - len(rows), replace=False).tolist())
    rows = np.asarray(sorted(rows))
    got = big[torch.from_numpy(rows).to(dev)].cpu().numpy()
    _assert_matches(got, _oracle(mode, x[rows], spw, prior), mode, f"mode {mode} U {U} spw {spw}")


# ---- 2. instantiation edges at small n ----------------------------------------------------------------------------------
EDGE_CASES = ([(m, U, spw) for m in (0, 1, 2) for spw in (5, 15) for U in (65, 66, 320, 321, 384, 385, 512, 513, 767, 768, 64)]
              + [(m, 30, 15) for m in (0, 1, 2)])


@pytest.mark.parametrize("mode,U,spw", EDGE_CASES)
def test_instantiation_edges(dev, mode, U, spw):
    """The bins-per-lane boundaries of the register form (5 / 6 / 8 / 12: U = 320 | 321, 384 | 385, 512 | 513, 768) and partial last
    lanes, the smallest register-form rows (65, 66) and the LDS fall-back (U = 64, and U = 30 with half-width 15), 64 frames with
    the planted frames first, against the oracle."""
    rng = np.random.default_rng(100 * U + spw + mode)
    x = logits_case(U + spw + mode, 64, U + (mode == 1))
    x[:16] = _special_frames(U, spw, mode, rng)
    prior = _prior(U) if mode == 2 else None
    got = _gpu(mode, torch.from_numpy(x).to(dev), spw, torch.from_numpy(prior).to(dev) if prior is not None else None).cpu().numpy()
    assert got.shape == (64, U + 1)
    _assert_matches(got, _oracle(mode, x, spw, prior), mode, f"mode {mode} U {U} spw {spw}")


def test_refusals_and_empty_launches(dev):
    """Geometries no kernel serves are refused (more than 768 bins, half-width 0, >= U, > 64); zero frames return an empty result."""
    for mode in (0, 1, 2):
        for U, spw in ((769, 5), (360, 0), (360, 360), (100, 100), (360, 65)):
            x = torch.zeros((4, U + (mode == 1)), device=dev)
            with pytest.raises(_lib.ViterbiHipError):
                _gpu(mode, x, spw)
        for shape in ((0, 360), (2, 0, 360)):
            x = torch.zeros(shape[:-1] + (360 + (mode == 1),), device=dev)
            got = _gpu(mode, x, 5)
            assert tuple(got.shape) == shape[:-1] + (361,)


# ---- 3. the float32 range edge of exp ----------------------------------------------------------------------------------
RANGE_CASES = [(0, 360, 5, None), (0, 320, 15, None), (0, 721, 5, None), (0, 500, 15, None), (0, 360, 3, None),
               (1, 360, 15, None), (1, 320, 5, None), (1, 721, 15, None), (1, 360, 31, None),
               (2, 320, 5, "scaled"), (2, 320, 5, "unscaled"), (2, 360, 5, "random"), (2, 721, 15, "random"), (2, 360, 3, "random")]


@pytest.mark.parametrize("mode,U,spw,prior_kind", RANGE_CASES)
def test_float32_range_edge(dev, mode, U, spw, prior_kind):
    """Peaks (and, in modes 1 and 2, the unvoiced logit) 80 .. 120 nats below the frame's top: e^-d is subnormal from ~87.4 on,
    and log(p + tiny) lies above log(tiny) by +0.42 at 88 nats, 4.7e-4 at 95.  Against the oracle, and at the reference's own
    geometries also against its recorded outputs (tests/golden/obs_range_goldens.npz)."""
    tops = RANGE_TOPS + RANGE_SPANS if mode == 2 else RANGE_TOPS
    x = range_edge_logits(U, spw, tops, unvoiced_column=mode == 1)
    if prior_kind == "scaled" or prior_kind == "unscaled":
        prior = np.load(os.path.join(GOLDEN, "params.npz"))["msnet321_pi"].astype(np.float32)
    else:
        prior = _prior(U) if prior_kind == "random" else None
    use_prior = prior if prior_kind != "unscaled" else None
    got = _gpu(mode, torch.from_numpy(x).to(dev), spw, torch.from_numpy(use_prior).to(dev) if use_prior is not None else None).cpu().numpy()
    want_p = _oracle(mode, x, spw, use_prior)
    sub = (want_p > 0) & (want_p < TINY)
    assert np.any(sub & (np.log(want_p + TINY) > FLOOR + 1e-4)), "the frames must reach the subnormal band"
    _assert_matches(got, want_p, mode, f"range edge mode {mode} U {U} spw {spw}")
    name = {(0, 360, 5): "shaun", (1, 360, 15): "softmax"}.get((mode, U, spw), prior_kind if mode == 2 and U == 320 else None)
    if name is not None:
        og = np.load(os.path.join(GOLDEN, "obs_range_goldens.npz"))
        assert tuple(og[f"{name}_args"]) == (U, spw) + tuple(tops)
        _assert_matches(got, og[f"{name}_probs"], mode, f"range edge vs reference goldens ({name})")


# ---- 4. the hand-off kernels -------------------------------------------------------------------------------------------
def test_voicing_map_and_notes_beyond_one_grid_pass(dev):
    """voicing / voicing_notes are grid-stride loops over at most 2048 x 256 threads: [3, T] states, T = 524 290 (not a multiple of
    256, 3 T > 3 * 2048 * 256 + 5: four passes), random states in [-1, n_bins] and -1, 0, n_bins - 1, n_bins planted at the ends and
    at the pass boundaries.  Against NumPy, exactly."""
    n_bins = 360
    dec = ViterbiDecoder(*synth.log_params(synth.tonet_transition(n_bins, 14), synth.floored_prior(n_bins + 1)), dev)
    B, T = 3, 524290
    assert B * T > 3 * 2048 * 256 + 5 and T % 256
    rng = np.random.default_rng(7)
    st = rng.integers(-1, n_bins + 1, (B, T)).astype(np.int32)
    flat = st.reshape(-1)
    special = np.asarray([-1, 0, n_bins - 1, n_bins], np.int32)
    for at in [0, flat.size - 4] + [k * 2048 * 256 - 2 for k in (1, 2, 3)]:
        flat[at:at + 4] = special
    note_range = (np.arange(n_bins) / 5.0 + 30.0).astype(np.float32)
    want_v = (st >= 0) & (st < n_bins)
    want_b = np.where(st < 0, -1, np.minimum(st, n_bins - 1)).astype(np.int32)
    want_n = np.where(want_v, note_range[np.maximum(want_b, 0)], np.float32(0))
    sd = torch.from_numpy(st).to(dev)
    voiced, bins = dec.voicing(sd)
    assert voiced.dtype == torch.bool and tuple(voiced.shape) == (B, T)
    assert np.array_equal(voiced.cpu().numpy(), want_v) and np.array_equal(bins.cpu().numpy(), want_b)
    voiced, bins, notes = dec.voicing_notes(sd, note_range)
    assert np.array_equal(voiced.cpu().numpy(), want_v) and np.array_equal(bins.cpu().numpy(), want_b)
    assert notes.cpu().numpy().tobytes() == want_n.tobytes()


@pytest.mark.parametrize("cls", ["Viterbi", "SoftMaxViterbi"])
def test_recording_accumulator_partial_tiles(dev, cls):
    """RecordingAccumulator.append (64 x 64 LDS tiles): 322 channels (321 or 322 columns: partial column tiles), F = 1, 63, 65, 100
    frames per snippet (partial frame tiles), up to 70 snippets, padded_frames cutting the last snippet inside a tile or at its
    edge.  Bit for bit the host's transpose / subtract / reshape, and nothing written past the rows held (the buffer is NaN-filled)."""
    n_bins = 321
    vit = getattr(ra, cls)(synth.tonet_transition(n_bins, 14), synth.floored_prior(n_bins + 1), device=dev)
    acc = ra.RecordingAccumulator(vit, max_frames=20000)
    assert acc.channels == 322 and acc.cols == (321 if cls == "Viterbi" else 322)
    acc._rows.fill_(float("nan"))                     # (the buffer behind the rows held: must stay untouched)
    rng = np.random.default_rng(11)
    host = []
    for n, F, padded in ((3, 1, 0), (70, 63, 13), (7, 65, 1), (5, 100, 30), (70, 65, 0), (2, 100, 0), (1, 63, 62), (4, 100, 99)):
        b = rng.normal(-6, 2, (n, acc.channels, F)).astype(np.float32)
        acc.append(torch.from_numpy(b).to(dev), padded)
        lg = np.transpose(b, [0, 2, 1])
        lg = (lg[..., 1:] - lg[..., :1]).reshape(-1, n_bins) if cls == "Viterbi" else lg.reshape(-1, acc.channels)
        host.append(lg[:len(lg) - padded])
        torch.cuda.synchronize()
        assert torch.isnan(acc._rows[acc.n_frames:]).all(), (n, F, padded, "a row past the recording was written")
    host = np.concatenate(host, axis=0)
    assert acc.n_frames == len(host)
    assert acc.logits().cpu().numpy().tobytes() == host.tobytes()
