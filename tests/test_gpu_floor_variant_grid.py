"""The Packed, Ckpt and PackedCkpt variants of banded_floor_forward_kernel, and the back-trace instantiations behind them, on every
(window width, target waves) pair a plan reaches: the 25 plans of tests/floor_grid.py (22 by the band recipe, 3 sparse bands; the five
pairs no plan reaches are listed there), in both storage types.  Through ViterbiDecoder: decode(algo="group") as the baseline,
decode_packed (vit_decode_packed: slot walk, lane back-trace), decode_checkpointed (vit_decode_checkpointed: pass 1 / segments,
sparse back-trace over the workgroup rows) and decode_packed_bounded (vit_decode_packed_bounded: pass 1 over slots, segment units).

Inputs per plan (floor_grid.plan_batches): T = 200; songs of 200, 1, 2, 3, 13, 14, 63, 64, 65, 129 and 199 frames -- one frame, both
sides of the twelve-frame unroll, both sides of one and two segments of 64 frames -- with synth.emissions_peaks and with
synth.emissions_ties, on the fp16 grid so that one oracle run serves both storage types; the ties batch carries a twelfth song of
200 frames with one finite emission per frame whose path (asserted on the oracle's) enters a target through the first and through
the last window entry and visits the unvoiced column (the three sparse-band plans have no extra column: window edges only).  A
third batch, floor_grid.emissions_hops, makes the path leave the window in most steps (asserted on the oracle's paths, also around
frames 64 and 128): there the candidate fl(M + c_j) decides, M the frame maximum of the kernel's idle slot S -- the i.i.d. kinds and
the forced song never ask for it.  The packed buffers hold the songs in a fixed shuffled order; with total frames / longest song = 3
and 4 forward slots every workgroup walks several songs back to back.

Bar: states and log-likelihood BITS equal to the CPU oracle (oracle.viterbi_oracle.decode_c) run on every song alone; no
tolerances.  Which plan each entry point serves is a literal table here, held against the library's size queries; a refused plan is
refused with nothing written.  The refusal edges (S == 64 NWT: no idle slot S) are refused by all three and served by decode."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests import floor_grid as fg
from tests import stream_grid as sg
from tests.f64_ref import band_params
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

IDS = [fg.plan_id(e) for e in fg.GRID]
# (W, NWT) of the grid plans each entry point serves.  vit_decode_packed: every pair of the floor form.  vit_decode_checkpointed: the
# pairs of floor_ckpt_pair (W >= 64 or NWT >= 8), back-traced by the sparse kernel over the workgroup rows, which applies to every
# grid plan (kc = ceil((W + 5) / 64) <= 3 candidates per lane, W + 32 inside the span of 64 / 128 / 160 floats, the span inside a row of
# (S + 5) / 4 * 4 floats), else by the lane form (an instantiated width, W <= S: every grid plan too).  vit_decode_packed_bounded: the
# same pairs, the sparse kernel only.
PACKED_SERVED = {(16, 2), (16, 4), (16, 6), (16, 8), (16, 12), (32, 2), (32, 4), (32, 6), (32, 8), (32, 12),
                 (64, 4), (64, 6), (64, 8), (64, 12), (84, 4), (84, 6), (84, 8), (84, 12),
                 (96, 4), (96, 6), (96, 8), (96, 12), (128, 6), (128, 8), (128, 12)}
CKPT_SERVED = {(16, 8), (16, 12), (32, 8), (32, 12),
               (64, 4), (64, 6), (64, 8), (64, 12), (84, 4), (84, 6), (84, 8), (84, 12),
               (96, 4), (96, 6), (96, 8), (96, 12), (128, 6), (128, 8), (128, 12)}
BOUNDED_SERVED = {(16, 8), (16, 12), (32, 8), (32, 12),
                  (64, 4), (64, 6), (64, 8), (64, 12), (84, 4), (84, 6), (84, 8), (84, 12),
                  (96, 4), (96, 6), (96, 8), (96, 12), (128, 6), (128, 8), (128, 12)}
UNSUPPORTED = -5                       # VIT_EUNSUPPORTED
CKPT_SEGMENTS = (64, 100, 4096)        # one row per 64 frames | a length that divides nothing | a single segment
BOUNDED_SEGMENTS = (64, 100)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x, np.float32)
    return x.view(np.uint32)


def _plan_case(dev, entry):
    """decoder and, per batch, (name, emissions float32 on the fp16 grid, lengths, the oracle's states and log-likelihoods): built once
    per plan and left unchanged (tests/stream_grid.py plan_case, shared with tests/test_gpu_stream_grid.py)."""
    dec, batches, _ = sg.plan_case(dev, entry)
    return dec, batches


def _same_padded(st, ll, ref_s, ref_l, what):
    assert np.array_equal(st.cpu().numpy(), ref_s), (what, "states")
    assert np.array_equal(_bits(ll), _bits(ref_l)), (what, "log-likelihood bits", ll.cpu().numpy(), ref_l)


def _same_packed(st, ll, order, off, ref_s, ref_l, what):
    st = st.cpu().numpy()
    assert st.shape == (int(off[-1]),)
    for k, b in enumerate(order):
        assert np.array_equal(st[off[k]:off[k + 1]], ref_s[b, :off[k + 1] - off[k]]), (what, "states of song", int(b))
    assert np.array_equal(_bits(ll), _bits(ref_l[order])), (what, "log-likelihood bits")


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("entry", fg.GRID, ids=IDS)
def test_every_variant_equals_the_oracle(dev, entry, f16):
    W, n, S, half, recipe = entry
    dec, batches = _plan_case(dev, entry)
    tag = (fg.plan_id(entry), "f16" if f16 else "f32")
    assert (W, n) in PACKED_SERVED
    try:
        for name, E32, lens, ref_s, ref_l in batches:
            E = torch.from_numpy(np.array(E32)).to(dev)
            E = E.half() if f16 else E
            ln = torch.from_numpy(np.array(lens)).to(dev)
            st, ll = dec.decode(E, lengths=ln, algo="group", out_dtype=torch.int32)
            _same_padded(st, ll, ref_s, ref_l, tag + (name, "decode"))

            order = fg.pack_order(lens)
            off = fg.offsets_of(lens[order])
            Ep = torch.cat([E[b, :int(lens[b])] for b in order], dim=0).contiguous()
            st, ll = dec.decode_packed(Ep, off, out_dtype=torch.int32)
            _same_packed(st, ll, order, off, ref_s, ref_l, tag + (name, "decode_packed"))
            for key, values in (("win_shift", (0, 1, 2, 3) if not f16 else ()), ("bt_warm", (0,))):
                for v in values:                     # every LDS window shift | no warm-up: the verify / repair pass decides
                    dec.set_option(key, v)
                    st, ll = dec.decode_packed(Ep, off, out_dtype=torch.int32)
                    _same_packed(st, ll, order, off, ref_s, ref_l, tag + (name, "decode_packed", key, v))
                    dec.set_option("reset", 0)

            if (W, n) in CKPT_SERVED:
                for K in CKPT_SEGMENTS:
                    st, ll = dec.decode_checkpointed(E, segment_frames=K, lengths=ln, out_dtype=torch.int32)
                    _same_padded(st, ll, ref_s, ref_l, tag + (name, "decode_checkpointed", K))
                dec.set_option("bt_fast_rows", 1)    # every row through the sparse kernel's general code
                st, ll = dec.decode_checkpointed(E, segment_frames=64, lengths=ln, out_dtype=torch.int32)
                _same_padded(st, ll, ref_s, ref_l, tag + (name, "decode_checkpointed", 64, "bt_fast_rows"))
                dec.set_option("reset", 0)
            if (W, n) in BOUNDED_SERVED:
                for K in BOUNDED_SEGMENTS:
                    st, ll = dec.decode_packed_bounded(Ep, off, segment_frames=K, out_dtype=torch.int32)
                    _same_packed(st, ll, order, off, ref_s, ref_l, tag + (name, "decode_packed_bounded", K))
    finally:
        dec.set_option("reset", 0)


def _refused_untouched(dev, dec, entry_points):
    """The C ABI of every named entry point on three songs of 200, 5 and 100 frames: VIT_EUNSUPPORTED, and `states` / `loglik` keep their
    sentinels (an accepted call with lengths starts by filling states with -1)."""
    if not entry_points:
        return
    lib = _lib.load()
    B, T = 3, 200
    lens = np.asarray([T, 5, 100], np.int64)
    off = fg.offsets_of(lens)
    E = synth.emissions_dense(B, T, dec.S, seed=1, device=dev)
    Ep = torch.cat([E[b, :int(lens[b])] for b in range(B)], dim=0).contiguous()
    ln = torch.from_numpy(lens).to(dev)
    ws = torch.empty((1 << 24) + 256, dtype=torch.uint8, device=dev)
    wp, wb = (ws.data_ptr() + 255) & ~255, 1 << 24
    for name in entry_points:
        st = torch.full((B, T), 12345, dtype=torch.int32, device=dev)
        ll = torch.full((B,), 7.0, dtype=torch.float32, device=dev)
        if name == "checkpointed":
            rc = lib.vit_decode_checkpointed(dec._plan, E.data_ptr(), _lib.VIT_F32, B, T, ln.data_ptr(), wp, wb, st.data_ptr(), ll.data_ptr(), 64, None)
            with pytest.raises(_lib.ViterbiHipError):
                dec.decode_checkpointed(E, segment_frames=64, lengths=ln)
        elif name == "packed":
            rc = lib.vit_decode_packed(dec._plan, Ep.data_ptr(), _lib.VIT_F32, B, off.ctypes.data, wp, wb, st.data_ptr(), ll.data_ptr(), None)
            with pytest.raises(_lib.ViterbiHipError):
                dec.decode_packed(Ep, off)
        else:
            rc = lib.vit_decode_packed_bounded(dec._plan, Ep.data_ptr(), _lib.VIT_F32, B, off.ctypes.data, wp, wb, st.data_ptr(), ll.data_ptr(), 64, None)
            with pytest.raises(_lib.ViterbiHipError):
                dec.decode_packed_bounded(Ep, off, segment_frames=64)
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED, (name, rc)
        assert bool((st == 12345).all()) and bool((ll == 7.0).all()), (name, "a refused call wrote its outputs")


def _sizes(dec):
    """(size > 0) of the three size queries, for three songs of 200, 5 and 100 frames and segments of 64."""
    lib = _lib.load()
    off = fg.offsets_of(np.asarray([200, 5, 100], np.int64))
    packed = int(lib.vit_workspace_bytes_packed(dec._plan, 3, int(off[-1])))
    ckpt = int(lib.vit_workspace_bytes_checkpointed(dec._plan, 3, 200, 64))
    bounded = int(lib.vit_workspace_bytes_packed_bounded(dec._plan, 3, off.ctypes.data, 64))
    assert (int(lib.vit_packed_bounded_units(dec._plan, 3)) > 0) == (bounded > 0)
    return {"packed": packed > 0, "checkpointed": ckpt > 0, "packed_bounded": bounded > 0}


def test_served_tables_cover_the_grid():
    """The literal tables against the grid and the predicates: Packed serves all 25 grid plans, the two checkpointed decodes the 19
    with W >= 64 or NWT >= 8; nothing in a table is not a grid plan."""
    have = {(W, n) for W, n, _, _, _ in fg.GRID}
    assert PACKED_SERVED == have and len(PACKED_SERVED) == 25
    assert CKPT_SERVED == {p for p in have if fg.floor_ckpt_pair(*p)} and len(CKPT_SERVED) == 19
    assert BOUNDED_SERVED == CKPT_SERVED and len(BOUNDED_SERVED) == 19
    assert all(fg.sparse_backtrace_applies_group(S, W) for W, n, S, _, _ in fg.GRID)


@pytest.mark.parametrize("entry", fg.GRID, ids=IDS)
def test_sizes_and_refusals_follow_the_tables(dev, entry):
    """size > 0 exactly where the table says the entry point serves the plan; where it does not, the decode is refused untouched."""
    W, n, S, half, recipe = entry
    dec = ViterbiDecoder(*fg.plan_params(entry), dev)
    want = {"packed": (W, n) in PACKED_SERVED, "checkpointed": (W, n) in CKPT_SERVED, "packed_bounded": (W, n) in BOUNDED_SERVED}
    assert _sizes(dec) == want, entry
    _refused_untouched(dev, dec, [k for k, served in want.items() if not served])


@pytest.mark.parametrize("S,half", fg.REFUSAL_EDGES)
def test_refusal_edges(dev, S, half):
    """S == 64 NWT: the idle slot S the variants keep the frame maximum in does not exist.  Size 0 and VIT_EUNSUPPORTED from all three
    entry points, nothing written; decode serves the plan and equals the oracle (by the scan form where the width has one, else by
    the dense kernel: the plain floor kernel wants the idle slot too, so algo "auto", not "group")."""
    A, pi = band_params(S, half)
    dec = ViterbiDecoder(A, pi, dev)
    assert dec.info["banded_ok"] and dec.info["floor_ok"] and not dec.info["wave_ok"] and S == 64 * fg.waves_for(S), dec.info
    assert _sizes(dec) == {"packed": False, "checkpointed": False, "packed_bounded": False}
    _refused_untouched(dev, dec, ["packed", "checkpointed", "packed_bounded"])
    E = synth.emissions_peaks(len(fg.LENGTHS), fg.T, S, seed=S, device=dev)
    ref_s, ref_l = vo.decode_c(A, pi, E.cpu().numpy(), lengths=fg.LENGTHS)
    st, ll = dec.decode(E, lengths=torch.from_numpy(fg.LENGTHS).to(dev), out_dtype=torch.int32)
    _same_padded(st, ll, ref_s, ref_l, (S, half, "decode"))
