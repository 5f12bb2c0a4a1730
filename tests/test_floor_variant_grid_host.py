"""Host tier of the plan grid of the float32 workgroup variants (tests/floor_grid.py): every grid plan is what the grid says it is
-- banded, floor-proven, no dense rows, no wave form, the stated window width and target-wave count, an idle slot S --, the grid
covers every (W, NWT) pair the Packed, Ckpt and PackedCkpt variants of banded_floor_forward_kernel are instantiated for except the
literal list no plan can reach, the predicates mirrored in floor_grid.py are the ones in the sources, and the inputs the GPU tier
(tests/test_gpu_floor_variant_grid.py) decodes hit the window edges they aim at.  No GPU."""
import os
import re

import numpy as np
import pytest

from oracle import viterbi_oracle as vo
from tests import floor_grid as fg
from tests.f64_ref import band_params
from tests.plan_replay import HostPlan
from tests.test_plan_host import _banded_matrix

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "viterbi_spl_amd", "csrc")
IDS = [fg.plan_id(e) for e in fg.GRID]


def _source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _ints(text):
    return tuple(int(x) for x in text.split(","))


def test_mirrored_predicates_are_the_sources():
    """The widths, the wave counts and the predicates floor_grid.py restates, read from plan.hpp and kernels.hpp: a new width, a new
    wave count or a changed predicate fails here until the mirror -- and with it the coverage test below -- follows."""
    plan_hpp, kernels_hpp = _source("plan.hpp"), _source("kernels.hpp")
    assert _ints(re.search(r"kBandedWidths\[\] = \{([^}]*)\}", plan_hpp).group(1)) == fg.WIDTHS
    assert _ints(re.search(r"const int opts\[5\] = \{([^}]*)\}", kernels_hpp).group(1)) == fg.WAVES
    for text in ("constexpr bool floor_form_instantiated(int W, int nwt) { return nwt > 0 && W <= 128 && nwt <= 12; }",
                 "return floor_ok && n_dense == 0 && nwt > 0 && S < nwt * 64 && banded_width_instantiated(W) && floor_form_instantiated(W, nwt);",
                 "constexpr bool floor_ckpt_pair(int W, int nwt) { return W >= 64 || nwt >= 8; }",
                 "return floor_packed_applies(S, W, floor_ok, n_dense) && floor_ckpt_pair(W, banded_waves_for(S));",
                 "constexpr bool floor_pckpt_applies(int S, int W, bool floor_ok, int n_dense) { return floor_ckpt_applies(S, W, floor_ok, n_dense); }"):
        assert text in kernels_hpp, text
    for S in range(1, 900):
        need = (S + 63) // 64
        assert fg.waves_for(S) == (min(w for w in fg.WAVES if w >= need) if need <= 12 else 0)


def test_grid_covers_every_instantiated_pair():
    """Packed: every pair of the floor form; Ckpt / PackedCkpt: those with W >= 64 or NWT >= 8.  Each has a grid plan or stands in
    UNREACHED, never both; an unreached pair is one for which no state count has both 2 W <= S (the plan picks no wider window)
    and banded_waves_for(S) == NWT."""
    packed = {(W, n) for W in fg.WIDTHS for n in fg.WAVES if fg.floor_form_instantiated(W, n)}
    ckpt = {p for p in packed if fg.floor_ckpt_pair(*p)}
    assert len(packed) == 30 and len(ckpt) == 24
    have = {(W, n) for W, n, _, _, _ in fg.GRID}
    assert len(have) == len(fg.GRID) == 25 and len(fg.BAND_GRID) == 22 and len(fg.SPARSE_GRID) == 3
    assert not have & set(fg.UNREACHED) and len(set(fg.UNREACHED)) == len(fg.UNREACHED) == 5
    assert have | set(fg.UNREACHED) == packed
    assert {p for p in have if fg.floor_ckpt_pair(*p)} | {p for p in fg.UNREACHED if fg.floor_ckpt_pair(*p)} == ckpt
    assert len({p for p in have if fg.floor_ckpt_pair(*p)}) == 19
    for W, n in packed:
        reachable = any(fg.waves_for(S) == n and 2 * W <= S and S < 64 * n for S in range(32, 64 * n))
        assert reachable == ((W, n) not in fg.UNREACHED), (W, n)


@pytest.mark.parametrize("entry", fg.GRID, ids=IDS)
def test_grid_plan_is_what_the_grid_says(entry):
    W, n, S, half, recipe = entry
    A, pi = fg.plan_params(entry)
    p = HostPlan(A, pi)
    assert p.ok and p.floor_ok and p.n_dense == 0 and not p.wave_ok, entry
    assert (p.S, p.W, fg.waves_for(S)) == (S, W, n) and S < 64 * n, (entry, p.W)
    assert p.max_window == 2 * half + 1 <= W
    assert p.extras == ([S - 1] if recipe == "band" else [])
    assert np.isfinite(A).all()                                           # (any step of the forced song is a finite candidate)
    assert fg.floor_packed_applies(S, p.W, p.floor_ok, p.n_dense)
    assert fg.sparse_backtrace_applies_group(S, W)                        # the sparse back-trace serves the rows of every grid plan
    lo = p.lo[:S]
    # (a sparse band's first rows start at column 0 or 1 by parity: those plans also run the back-traces' table lookup of lo)
    assert np.array_equal(lo[half:], np.clip(np.arange(half, S) - half, 0, S - W))
    assert np.array_equal(lo[:half], np.zeros(half)) == (recipe == "band")
    # the inputs of the GPU tier: on the fp16 grid, and the forced song's path (the oracle's) goes through both window edges and
    # through the unvoiced column
    (_, peaks, lens_p), (_, ties, lens_t), (_, hops, lens_h) = fg.plan_batches(entry, A, lo, p.extras)
    assert peaks.shape == hops.shape == (11, fg.T, S) and ties.shape == (12, fg.T, S) and lens_t[-1] == fg.T
    # the hops batch leaves the window (the frame-maximum candidate decides), the i.i.d. kinds hardly ever do
    hop_s, hop_l = vo.decode_c(A, pi, hops, lengths=lens_h)
    assert np.isfinite(hop_l).all()
    fg.premise_hops(hop_s, lens_h, W, lo, p.extras)
    assert np.array_equal(peaks.astype(np.float16).astype(np.float32), peaks)
    assert int(lens_t.sum()) // int(lens_t.max()) == 4                    # forward slots of the packed decode: each walks several songs
    forced, walk = fg.forced_song(A, W, half, lo, p.extras[0] if p.extras else None)
    assert np.array_equal(forced, ties[-1])
    ref_s, ref_l = vo.decode_c(A, pi, forced[None])
    assert np.array_equal(ref_s[0], walk) and np.isfinite(ref_l[0])
    fg.premise_forced(ref_s[0], W, lo, p.extras[0] if p.extras else None)


@pytest.mark.parametrize("S,half", fg.REFUSAL_EDGES)
def test_refusal_edges_have_no_idle_slot(S, half):
    """Banded and floor-proven like the grid plans, but S == 64 NWT: the variants' predicate refuses them."""
    A, pi = band_params(S, half)
    p = HostPlan(A, pi)
    assert p.ok and p.floor_ok and p.n_dense == 0 and not p.wave_ok
    assert S == 64 * fg.waves_for(S) and p.W in fg.WIDTHS and p.max_window == 2 * half + 1
    assert not fg.floor_packed_applies(S, p.W, p.floor_ok, p.n_dense)
    assert fg.floor_packed_applies(S - 1, p.W, p.floor_ok, p.n_dense)     # (the idle slot alone decides)


@pytest.mark.parametrize("pair", sorted(fg.SPARSE_GRID))
def test_full_bands_do_not_reach_the_sparse_pairs(pair):
    """The full-band recipes at the state count and half-width of a sparse grid plan: every column is an exception in more than a
    quarter of the rows, the plan finds more extra columns than it takes and proves nothing."""
    S, half = fg.SPARSE_GRID[pair]
    assert 2 * half + 1 > S // 4
    assert not HostPlan(*band_params(S, half)).ok
    rng = np.random.default_rng(S)
    assert not HostPlan(_banded_matrix(S, half, rng, floor=-50.0, quant=2), -(rng.integers(0, 8, S) / 2).astype(np.float32)).ok


def test_wave_form_seeds():
    """WAVE_FORM_SEEDS are the geometries of test_wave_form_geometries whose plan has the wave form: S + extra columns < 384."""
    got = []
    for seed in fg.WAVE_GEOMETRY_SEEDS:
        S, half, extras, A, pi, _ = fg.wave_geometry(seed)
        p = HostPlan(A, pi)
        assert p.ok and p.extras == extras and p.wave_ok == (S + len(extras) < 384), (seed, S, half, extras)
        got += [seed] * p.wave_ok
    assert tuple(got) == fg.WAVE_FORM_SEEDS and len(got) >= 8


def test_pack_order_is_shuffled():
    for lens in (fg.LENGTHS, np.append(fg.LENGTHS, fg.T)):
        order = fg.pack_order(lens)
        assert sorted(order.tolist()) == list(range(len(lens)))
        assert not np.array_equal(order, np.argsort(lens)) and not np.array_equal(order, np.argsort(-lens))
