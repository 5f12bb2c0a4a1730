"""Host tier of the streaming-session grid (tests/stream_grid.py, tests/test_gpu_stream_grid.py): the literal tables of what a session
serves against vit_workspace_bytes_stream and against the predicates in the sources; the constants and divisors behind the
chunk counts the long GPU sessions rely on, read from the sources and recomputed; the session workspace's chunk-entry table;
what the append schedules promise about launch boundaries; and the wrong-guess premise of the seven-chunk back-trace on
every grid plan.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import viterbi_oracle as vo
from tests import floor_grid as fg
from tests import stream_grid as sg
from tests.common import durrieu_log_params
from tests.f64_ref import band_params
from tests.plan_replay import HostPlan

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "viterbi_spl_amd", "csrc")
IDS = [fg.plan_id(e) for e in fg.GRID]


def _source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _const(text, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


@pytest.fixture(scope="module")
def lib():
    from viterbi_spl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _need(lib, A, pi, B, T_cap):
    A = np.ascontiguousarray(A, np.float32)
    pi = np.ascontiguousarray(pi, np.float32)
    plan = ctypes.c_void_p()
    assert lib.vit_plan_create(A.ctypes.data, pi.ctypes.data, A.shape[0], ctypes.byref(plan)) == 0
    need = int(lib.vit_workspace_bytes_stream(plan, B, T_cap))
    lib.vit_plan_destroy(plan)
    return need


def _session_predicate(p):
    """capi.hip st_family for a banded plan, restated over a HostPlan: the Stream instantiation and a back-trace over its rows.  It
    does not ask whether the plan has the wave form."""
    lane = p.n_dense == 0 and p.W in fg.WIDTHS and p.W <= p.S
    return bool(p.ok) and fg.floor_packed_applies(p.S, p.W, p.floor_ok, p.n_dense) and (fg.sparse_backtrace_applies_group(p.S, p.W) or lane)


# ------------------------------------------------------------------ the served tables
def test_stream_served_is_the_grid_and_the_predicates_are_the_sources():
    """Every (W, NWT) pair of the grid has an entry in STREAM_SERVED and nothing else has; the predicates the tables restate are the
    ones in the sources."""
    have = {(W, n) for W, n, _, _, _ in fg.GRID}
    assert not have - sg.STREAM_SERVED, ("grid pairs without an entry in STREAM_SERVED", sorted(have - sg.STREAM_SERVED))
    assert sg.STREAM_SERVED == have and len(sg.STREAM_SERVED) == 25
    kernels_hpp, capi = _source("kernels.hpp"), _source("capi.hip")
    for text in ("constexpr bool floor_stream_applies(int S, int W, bool floor_ok, int n_dense) { return floor_packed_applies(S, W, floor_ok, n_dense); }",
                 "constexpr bool step_kernel_instantiated(int S, int bw, int kb) { return bw == 20 && kb == 9 && S - 1 > 704 && S - 1 <= 768; }"):
        assert text in kernels_hpp, text
    for text in ("return vit::floor_stream_applies(p->S, p->bp.W, p->bp.floor_ok, p->bp.n_dense) && (ck_sparse_applies(p, kFamGroup) || ck_lane_applies(p)) ? kFamGroup : kFamNone;",
                 "return step_applies(p) ? kFamStep : kFamNone;",
                 "bool ck_lane_applies(const vit_plan* p) { return p->bp.n_dense == 0 && vit::banded_width_instantiated(p->bp.W) && p->bp.W <= p->S; }"):
        assert text in capi, text
    body = capi[capi.index("int st_family(const vit_plan* p) {"):]
    assert "wave_ok" not in body[:body.index("\n}\n")]


@pytest.mark.parametrize("entry", fg.GRID, ids=IDS)
def test_grid_plans_are_served(lib, entry):
    W, n, S, half, recipe = entry
    A, pi = fg.plan_params(entry)
    assert ((W, n) in sg.STREAM_SERVED) == _session_predicate(HostPlan(A, pi)) is True
    SD = (S + 5) // 4 * 4
    for B, T in ((1, 1), (11, sg.T_CAP), (12, sg.T_CAP), (16, 30000)):
        need = _need(lib, A, pi, B, T)
        assert need > 0 and need % 256 == 0, (entry, B, T, need)
        assert B * T * SD * 4 <= need <= B * T * SD * 4 + 256 + B * 2048 + 8 * 256, (entry, B, T, need)


@pytest.mark.parametrize("S,half", fg.REFUSAL_EDGES)
def test_refusal_edges_are_refused(lib, S, half):
    A, pi = band_params(S, half)
    assert not _session_predicate(HostPlan(A, pi))
    assert _need(lib, A, pi, 11, sg.T_CAP) == 0


@pytest.mark.parametrize("n", sorted(sg.STEP_SERVED))
def test_step_plans(lib, n):
    A, pi = durrieu_log_params(n, 20)
    p = HostPlan(A, pi)
    assert p.step_ok and (p.step_bw, p.step_kb) == (20, 9) and not p.ok
    need = _need(lib, A, pi, 6, 157)
    assert (need > 0) == sg.STEP_SERVED[n] == (704 < n <= 768), (n, need)
    if need:
        SD = (n + 1 + 5) // 4 * 4
        assert need % 256 == 0 and 6 * 157 * (n + 1) * 4 <= need <= 6 * 157 * (SD + 4) * 4 + 256 + 6 * 2048 + 8 * 256, (n, need)


def test_wave_form_geometries(lib):
    """What the library answers for the wave-form geometries, written down in WAVE_SEED_SERVED, and why: st_family ignores wave_ok, so
    a floor-proven plan with an idle slot and an instantiated window is served although decode would run it in the wave form."""
    assert sorted(sg.WAVE_SEED_SERVED) == sorted(fg.WAVE_FORM_SEEDS)
    extras_seen = set()
    for seed in fg.WAVE_FORM_SEEDS:
        S, half, extras, A, pi, _ = fg.wave_geometry(seed)
        p = HostPlan(A, pi)
        assert p.ok and p.wave_ok
        need = _need(lib, A, pi, len(fg.LENGTHS), sg.T_CAP)
        assert (need > 0) == sg.WAVE_SEED_SERVED[seed] == _session_predicate(p), (seed, need)
        if need:
            assert (p.W, fg.waves_for(S)) in sg.STREAM_SERVED
            extras_seen.add(len(extras))
    assert extras_seen == {0, 1, 2}


# ------------------------------------------------------------------ the chunk counts of the long sessions
def test_natural_chunk_counts_of_the_long_sessions():
    """kBtWarm, kBtWarmSparse, kBtMaxChunks and kLaneMaxChunks from kernels.hpp, the divisors of the three *_backtrace_chunks from
    their files: the long sessions of the GPU tier (recordings of 2304 and 1100 frames) are back-traced as four sparse, eighteen
    lane and two lazy chunks, on any number of compute units.  A retuned constant that brings one of them down to a single chunk
    fails here, with the length that would restore it."""
    hpp = _source("kernels.hpp")
    warm, warm_sparse = _const(hpp, "kBtWarm"), _const(hpp, "kBtWarmSparse")
    max_chunks, lane_max = _const(hpp, "kBtMaxChunks"), _const(hpp, "kLaneMaxChunks")
    sparse, rows, lane = _source("backtrace_sparse.hip"), _source("backtrace_rows.hip"), _source("backtrace_lane.hip")
    d_sparse = int(re.search(r"const long long cmax = T / \((\d+) \* kBtWarmSparse\) > 1", sparse).group(1))
    d_lazy = int(re.search(r"const long long cmax = T / \((\d+) \* kBtWarm\) > 1", rows).group(1))
    d_lane = int(re.search(r"const long long cmax = T / \((\d+) \* \(warm > 0 \? warm : 1\)\) > 1", lane).group(1))
    assert "long long c = (16ll * (n_cus > 0 ? n_cus : 256)) / (B > 0 ? B : 1);" in sparse
    assert "long long c = (2 * 1024 + B - 1) / (B > 0 ? B : 1);" in rows
    assert "const long long target = 16ll * 64 * (n_cus > 0 ? n_cus : 256);" in lane
    assert (d_sparse, d_lazy, d_lane) == (8, 8, 2) and (warm, warm_sparse, max_chunks, lane_max) == (128, 64, 32, 256)
    B, T = len(sg.LONG_LENGTHS), max(sg.LONG_LENGTHS)
    assert T <= sg.LONG_T_CAP and T % sg.LONG_APPEND == 0
    for n_cus in (1, 64, 256, 304):
        got = {"sparse": sg.sparse_chunks(B, T, n_cus, warm_sparse, max_chunks), "lane": sg.lane_chunks(B, T, n_cus, warm_sparse, lane_max),
               "lazy": sg.lazy_chunks(B, T, warm, max_chunks)}
        assert got == sg.LONG_CHUNKS, (n_cus, got)
    need_T = {"sparse": 2 * d_sparse * warm_sparse, "lane": 2 * d_lane * warm_sparse, "lazy": 2 * d_lazy * warm}
    for k, t in need_T.items():
        assert T >= t, f"the long sessions run one {k} chunk: raise stream_grid.LONG_LENGTHS[0] to at least {t}"
    # and the sessions of the grid are the one-chunk case unless a test tunes them
    assert sg.sparse_chunks(11, fg.T, 256) == sg.lane_chunks(11, fg.T, 256) == sg.lazy_chunks(6, 150) == 1


def test_session_workspace_holds_the_chunk_entries():
    """st_layout sizes the chunk-entry table as B * kLaneMaxChunks, and the sparse and lazy kernels (at most kBtMaxChunks entries per
    recording) share it; the counters the GPU tier reads sit right behind the history rows, kBtCounters per recording."""
    hpp, capi = _source("kernels.hpp"), _source("capi.hip")
    assert _const(hpp, "kBtMaxChunks") <= _const(hpp, "kLaneMaxChunks")
    assert "constexpr int kLaneMaskWords = kLaneMaxChunks / 32;" in hpp
    assert _const(hpp, "kBtCounters") == 16
    body = capi[capi.index("StLayout st_layout(const vit_plan* p, int family, int64_t B, int64_t T_cap) {"):]
    body = body[:body.index("\n}\n")]
    for text in ("s.off_cnt = align256((size_t)B * (size_t)T_cap * (size_t)hist_layout(p, family).SD * sizeof(float));",
                 "s.off_mask = s.off_cnt + align256((size_t)B * vit::kBtCounters * sizeof(int32_t));",
                 "s.off_len = s.off_entry + align256((size_t)B * vit::kLaneMaxChunks * sizeof(int32_t));"):
        assert text in body, text
    # a session honours bt_chunks up to the cap of the kernel that runs
    assert "VIT_TRY(segment_backtrace(plan, s->family, lane_bt, b, st, true));" in capi
    assert "auto chunks_of = [&](int chunks, int cap) { return tune_chunks ? tuned_chunks(tn, chunks, cap) : chunks; };" in capi


# ------------------------------------------------------------------ the schedules and the inputs
@pytest.mark.parametrize("name", sg.SCHEDULES)
def test_schedules_keep_their_promises(name):
    from tests.test_gpu_step_geometries import ragged
    for lens, T in ((fg.LENGTHS, fg.T), (np.append(fg.LENGTHS, fg.T), fg.T), (ragged(150), 150)):
        sched = sg.schedule(name, lens, T)
        sg.premise_schedule(name, sched, lens)
        assert all(1 <= n and cnt.max() >= 1 for n, cnt in sched)
        starts, _ = sg.launch_starts(sched, len(lens))
        if name == "segments":
            assert starts[0] == set(range(0, T, 64))
        if name == "odd":
            assert {63, 64, 65} <= starts[0]
        if name == "staggered":
            uni = sg.uniform_launches(sched, len(lens))
            assert not any(uni[:3]), "the first launches of `staggered` go through the tables"


@pytest.mark.parametrize("entry", fg.GRID, ids=IDS)
def test_seven_chunks_start_from_a_wrong_guess(entry):
    """The premise of the (7, 0) back-trace case on song 0 of every plan's hops batch (floor_grid.HOPS_RESEED picks another seed where
    the plain one has every guess right)."""
    W, n, S, half, recipe = entry
    A, pi = fg.plan_params(entry)
    p = HostPlan(A, pi)
    hops = fg.plan_batches(entry, A, p.lo[:S], p.extras)[2][1]
    ref_s, _ = vo.decode_c(A, pi, hops[:1])
    assert fg.premise_wrong_guess(A, pi, hops[0], ref_s[0], chunks=7) >= 1
