"""The row-independent kernels past element 2^31 and byte 2^32 of their buffers: the three emission builders (vit_obs_shaun,
vit_obs_softmax, vit_obs_softmax_scaled), vit_obs_activations, vit_voicing_map and vit_voicing_notes.

Rows are independent, so the input is a block of P = 4099 rows (a prime: no wrapped offset is a whole number of periods) repeated
up to the size.  Three checks: (1) every row of the large launch equals, bit for bit, the row of a launch on the block alone (low
offsets) -- the whole buffer, compared on the device; (2) the first and last 64 rows, 64 rows around every mark and 4096 seeded
rows, read back from the large buffer, hold no poison and match oracle/observation_oracle.py at the bar of tests/test_gpu_builders.py
(exp and log run on the GPU: the same structural zeros, probabilities within 1e-5 relative), the voicing kernels NumPy exactly;
(3) the outputs are poisoned first."""
import numpy as np
import pytest
import torch

from tests import far_offsets as fo
from tests.common import logits_case
from tests.far_offsets import assert_builder_matches as _assert_matches, builder_oracle as _oracle, builder_prior as _prior
from viterbi_spl_amd import _lib, emissions as em, synth

pytestmark = pytest.mark.gpu

P = 4099


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _tiled(block, n):
    """[n, ...]: the rows of `block` repeated."""
    reps = -(-n // block.shape[0])
    return block.repeat((reps,) + (1,) * (block.dim() - 1))[:n].contiguous()


def _equals_block(big, small, what):
    """Every row r of `big` equals row r % P of `small`, by bits."""
    n, p = big.shape[0], small.shape[0]
    full = n // p * p
    kind = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[big.element_size()]
    b, s = big.view(kind), small.view(kind)
    diff = (b[:full].view(n // p, p, -1) != s.view(1, p, -1)).any(dim=2)                  # [periods, p]
    if bool(diff.any()):                                       # (reduced per axis first: the mask holds more than 2^31 entries)
        periods, rows = diff.any(dim=1).nonzero().flatten(), diff.any(dim=0).nonzero().flatten()
        raise AssertionError(f"{what}: rows differ from the block's in {periods.numel()} periods (first {periods[:4].tolist()}), "
                             f"block rows {rows[:8].tolist()}")
    assert torch.equal(b[full:], s[:n - full]), f"{what}: the last partial period differs"


BUILDERS = [(0, 360, 5, False), (1, 360, 15, False), (2, 320, 5, True), (0, 721, 5, False)]


@pytest.mark.parametrize("mode,U,spw,with_prior", BUILDERS, ids=[f"mode{m}-U{u}-spw{s}" for m, u, s, _ in BUILDERS])
def test_emission_builders(dev, mode, U, spw, with_prior):
    cols = U + (mode == 1)
    buffers = [(cols, 4), (U + 1, 4)]
    n = fo.rows_past(buffers) + 64
    fo.need_free(n * 4 * (cols + U + 1) * 2)
    xb = logits_case(50 + mode, P, cols)
    prior = _prior(U) if with_prior else None
    prior_dev = torch.from_numpy(prior).to(dev) if with_prior else None
    block = torch.from_numpy(xb).to(dev)
    x = _tiled(block, n)
    with fo.measured(f"rows/obs_mode{mode}/U{U}", (n, cols)):
        if mode < 2:
            out = torch.full((n, U + 1), float("nan"), device=dev)
            fn = em.shaun_log_emissions if mode == 0 else em.softmax_log_emissions
            fn(x, single_side_peak_width=spw, out=out)
            small = fn(block, single_side_peak_width=spw)
        else:
            poison = torch.full((n, U + 1), float("nan"), device=dev)
            out = em.softmax_scaled_log_emissions(x, 0.5, prior_dev, single_side_peak_width=spw, out=poison)
            small = em.softmax_scaled_log_emissions(block, 0.5, prior_dev, single_side_peak_width=spw)
        _equals_block(out, small, f"mode {mode}")
        rows = fo.probe_rows(n, buffers, seed=mode)
        got = out[torch.from_numpy(rows).to(dev)].cpu().numpy()
    assert not np.isnan(got).any(), "a compared row keeps the poison"
    _assert_matches(got, _oracle(mode, xb[rows % P], spw, prior), mode, f"far rows, mode {mode} U {U}")
    del x, out, small
    fo.release()


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_activations(dev, f16):
    """vit_obs_activations on hf0 [721, N] with 721 * N and N * 722 past the marks: one recording, so the statistics are the block's
    and every output row is the block's row."""
    U = 721
    isz = 2 if f16 else 4
    buffers = [(U + 1, isz)]
    n = max(fo.rows_past(buffers), (1 << 31) // U + 1) + 64
    assert U * n > 1 << 31
    fo.need_free(n * (U * 4 + (U + 1) * isz) * 2)
    hb = synth.hf0_activations(U, P, seed=5, device=dev)                      # [U, P]
    hf0 = hb.repeat(1, -(-n // P))[:, :n]                                     # (a column slice: the row stride is a little above n)
    dt = torch.float16 if f16 else torch.float32
    with fo.measured(f"rows/obs_activations/{'f16' if f16 else 'f32'}", (U, n)):
        out = torch.full((n, U + 1), float("nan"), dtype=dt, device=dev)
        _, stats = em.activation_log_emissions(hf0, out=out, dtype=dt, return_stats=True)
        small, stats_b = em.activation_log_emissions(hb, dtype=dt, return_stats=True)
        assert torch.equal(stats.view(torch.int32), stats_b.view(torch.int32))
        _equals_block(out, small, "activations")
        rows = fo.probe_rows(n, buffers, seed=9)
        got = out[torch.from_numpy(rows).to(dev)]
        assert not torch.isnan(got).any(), "a compared row keeps the poison"
        assert torch.equal(got.view(torch.int16 if f16 else torch.int32), small[torch.from_numpy(rows % P).to(dev)].view(torch.int16 if f16 else torch.int32))
    del hf0, out, small, got
    fo.release()


def test_voicing_map_and_notes(dev):
    """vit_voicing_map / vit_voicing_notes over n > 2^31 states: states in [-1, n_bins] with the edge values planted, the outputs
    poisoned; against the NumPy definition (include/viterbi_hip.h: negative states give voiced = 0, bins = -1), exactly."""
    lib = _lib.load()
    n_bins = 360
    n = (1 << 31) + 3 * P + 5
    fo.need_free(n * (4 + 1 + 4 + 4) + (2 << 30))
    rng = np.random.default_rng(12)
    sb = rng.integers(-1, n_bins + 1, P).astype(np.int32)
    sb[:4] = sb[-4:] = np.asarray([-1, 0, n_bins - 1, n_bins], np.int32)
    note_range = (np.arange(n_bins) / 5.0 + 30.0).astype(np.float32)
    want_v = ((sb >= 0) & (sb < n_bins)).astype(np.uint8)
    want_b = np.where(sb < 0, -1, np.minimum(sb, n_bins - 1)).astype(np.int32)
    want_n = np.where(want_v.astype(bool), note_range[np.maximum(want_b, 0)], np.float32(0)).astype(np.float32)
    st = _tiled(torch.from_numpy(sb).to(dev), n)
    nr = torch.from_numpy(note_range).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rows = fo.probe_rows(n, [(1, 4)], seed=3)          # (byte 2^32 of the one-byte `voiced` needs 2^32 states: 56 GB of buffers, not run)
    rows_d = torch.from_numpy(rows).to(dev)
    with fo.measured("rows/voicing", (n,)):
        for notes_too in (False, True):
            voiced = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
            bins = torch.full((n,), -77, dtype=torch.int32, device=dev)
            notes = torch.full((n,), float("nan"), dtype=torch.float32, device=dev) if notes_too else None
            if notes_too:
                rc = lib.vit_voicing_notes(st.data_ptr(), n, n_bins, nr.data_ptr(), voiced.data_ptr(), bins.data_ptr(), None, notes.data_ptr(), stream)
            else:
                rc = lib.vit_voicing_map(st.data_ptr(), n, n_bins, voiced.data_ptr(), bins.data_ptr(), stream)
            assert rc == 0
            _equals_block(voiced.view(-1, 1), torch.from_numpy(want_v).to(dev).view(-1, 1), "voiced")
            _equals_block(bins.view(-1, 1), torch.from_numpy(want_b).to(dev).view(-1, 1), "bins")
            assert np.array_equal(voiced[rows_d].cpu().numpy(), want_v[rows % P]) and np.array_equal(bins[rows_d].cpu().numpy(), want_b[rows % P])
            if notes_too:
                _equals_block(notes.view(-1, 1), torch.from_numpy(want_n).to(dev).view(-1, 1), "notes")
                assert notes[rows_d].cpu().numpy().tobytes() == want_n[rows % P].tobytes()
            del voiced, bins, notes
    del st
    fo.release()
