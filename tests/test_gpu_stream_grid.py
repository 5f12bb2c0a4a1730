"""Streaming sessions (vit_stream_*, ViterbiDecoder.stream) on every workgroup geometry and back-trace form.  tests/test_gpu_stream.py
holds the session's contract on the five golden plans with one-chunk back-traces of 203 frames; this module is the grid:

1. banded_floor_forward_kernel<.., WgVariant::Stream> on the 25 (window width, target waves) pairs of tests/floor_grid.py, both storage
   types, with the inputs of tests/test_gpu_floor_variant_grid.py (peaks | ties and the forced song | hops: the frame maximum decides,
   also in the steps into frames 64, 128 and 192), fed by the schedules of tests/stream_grid.py -- launches that start exactly on
   those frames, every prefetch depth and unroll remainder, recordings at different positions in one launch -- into sessions of
   207 rows per recording that are reused with reset(); a decode in the middle; every LDS window shift; the sparse and the lane
   back-trace as one, seven, 32 and 64 chunks without and with a warm-up; the other storage type and a shorter recording over
   stale rows.  The wave-form geometries of floor_grid.WAVE_FORM_SEEDS (none, one and two extra columns) ride along;
2. step4s_forward_kernel<.., WgVariant::Stream> at the edges of its range (705 .. 768 voiced states, every fill of the last quad)
   with the lazy back-trace chunked the same ways, and the gate: plans without a Stream instantiation are refused untouched;
3. two long sessions whose chunk count is the library's own: four sparse, eighteen lane and two lazy chunks.

Bar: states equal oracle.viterbi_oracle.decode_c run on every recording alone, -1 behind each length; log-likelihoods equal by
float32 bits; no tolerances.  Every chunk tensor holds NaN in the rows no recording takes."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests import floor_grid as fg
from tests import stream_grid as sg
from tests import test_gpu_step_geometries as geo
from tests.common import emissions_jumps
from tests.plan_replay import HostPlan
from viterbi_spl_amd import ViterbiDecoder, _lib

pytestmark = pytest.mark.gpu

IDS = [fg.plan_id(e) for e in fg.GRID]
EUNSUPPORTED = -5
BT_GRID = {0: ((0, -1), (7, 0), (32, 1)), 4: ((0, -1), (7, 0), (32, 1), (64, 0))}      # backtrace_form -> (bt_chunks, bt_warm)
BT_STEP = ((0, -1), (7, 0), (32, 1), (5, 40))
CT_CHUNKS_REPAIRED = ViterbiDecoder.COUNTERS.index("chunks_repaired")
CT_PER_SONG = 16                       # kernels.hpp kBtCounters (tests/test_stream_grid_host.py reads it there)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x, np.float32)
    return x.view(np.uint32)


def _meets_the_bar(st, ref_s, ref_l, lens, tag):
    """decode() of the session as it stands against the oracle at `lens`: the lengths, the states with -1 behind each length, the
    log-likelihood bits."""
    assert np.array_equal(st.lengths, lens), (tag, "lengths", st.lengths)
    s, l = st.decode(out_dtype=torch.int32)
    s = s.cpu().numpy()
    m = int(np.max(lens))
    assert s.shape == (len(lens), m), (tag, s.shape)
    assert all((ref_s[b, int(L):] == -1).all() for b, L in enumerate(lens))
    assert np.array_equal(s, ref_s[:, :m]), (tag, "states", np.argwhere(s != ref_s[:, :m])[:6])
    assert np.array_equal(_bits(l), _bits(ref_l)), (tag, "log-likelihood bits", l.cpu().numpy(), ref_l)


def _device_rows(dev, E32, lens, dtype):
    return sg.nan_rows(torch.from_numpy(np.array(E32)).to(dev).to(dtype), lens)


def _session_with_counters(dec, B, T_cap, SD):
    """A session in a workspace of the test's own, and a view of the back-trace's event counters in it: [B, 16] int32 behind the
    B * T_cap history rows (capi.hip st_layout: off_cnt)."""
    need = dec.workspace_bytes_stream(B, T_cap)
    assert need > 0
    buf = torch.zeros(need + 256, dtype=torch.uint8, device=dec.device)
    st = dec.stream(B, T_cap, workspace=buf)
    off = ((buf.data_ptr() + 255) & ~255) - buf.data_ptr() + (B * T_cap * SD * 4 + 255) // 256 * 256
    return st, buf[off:off + B * CT_PER_SONG * 4].view(torch.int32).view(B, CT_PER_SONG)


# ------------------------------------------------------------------ 1. the floor grid
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("entry", fg.GRID, ids=IDS)
def test_every_floor_pair_as_a_session(dev, entry, f16):
    """One session per batch, B recordings of 207 rows, reused across the four schedules with reset().  hops + segments: the first frame
    of every resumed launch is a hop (floor_grid.premise_hops), so the re-formed frame maximum decides it and the back-trace reads
    its bound from the pad column that launch stored; also decoded after two appends, and (float32) under every window shift.
    hops and ties, fully fed: both back-trace forms under BT_GRID -- (7, 0) after the premise that song 0 of the hops batch
    starts a chunk from a wrong guess, and the sparse kernel's counters must then show a repaired chunk in that song (so
    "bt_chunks" reaches a session's back-trace).  peaks: reset() and the other storage type in the same session, then reset() and
    only 70 frames of every recording over the stale rows and pad columns."""
    W, n, S, half, recipe = entry
    assert (W, n) in sg.STREAM_SERVED
    dec, batches, kept = sg.plan_case(dev, entry)
    A, pi = kept["A"], kept["pi"]
    dt, other = (torch.float16, torch.float32) if f16 else (torch.float32, torch.float16)
    tag = (fg.plan_id(entry), "f16" if f16 else "f32")
    SD = (S + 5) // 4 * 4
    try:
        for name, E32, lens, ref_s, ref_l in batches:
            B = len(lens)
            En = _device_rows(dev, E32, lens, dt)
            st, counters = _session_with_counters(dec, B, sg.T_CAP, SD)
            for sname in sg.SCHEDULES:
                sched = sg.schedule(sname, lens, fg.T)
                sg.premise_schedule(sname, sched, lens)
                st.reset()
                if (name, sname) == ("hops", "segments"):
                    if "hops128" not in kept:
                        kept["hops128"] = vo.decode_c(A, pi, E32, lengths=np.minimum(lens, 128))
                    sg.feed(st, En, sched, upto=2)
                    _meets_the_bar(st, *kept["hops128"], np.minimum(lens, 128), tag + (name, sname, "after two appends"))
                    sg.feed(st, En, sched, first=2)
                else:
                    sg.feed(st, En, sched)
                _meets_the_bar(st, ref_s, ref_l, lens, tag + (name, sname))

            if name in ("hops", "ties"):               # fully fed: the back-trace forms over the session's rows
                if name == "hops":
                    fg.premise_wrong_guess(A, pi, E32[0], ref_s[0], chunks=7)
                for form, tunings in BT_GRID.items():
                    for chunks, warm in tunings:
                        dec.set_option("backtrace_form", form)
                        dec.set_option("bt_chunks", chunks)
                        dec.set_option("bt_warm", warm)
                        _meets_the_bar(st, ref_s, ref_l, lens, tag + (name, "backtrace_form", form, chunks, warm))
                        dec.set_option("reset", 0)
                        if name == "hops" and (form, chunks, warm) == (0, 7, 0):
                            repaired = int(counters[0, CT_CHUNKS_REPAIRED])
                            assert repaired > 0, (tag, "seven chunks without a warm-up repaired nothing in song 0: is bt_chunks honoured?")

            if name == "hops" and not f16:             # every LDS window shift of the Stream kernel
                sched = sg.schedule("segments", lens, fg.T)
                for shift in (0, 1, 2, 3):
                    dec.set_option("win_shift", shift)
                    st.reset()
                    sg.feed(st, En, sched)
                    _meets_the_bar(st, ref_s, ref_l, lens, tag + (name, "win_shift", shift))
                    dec.set_option("reset", 0)

            if name == "peaks":
                st.reset()                              # the other storage type in the same session (same values: the fp16 grid)
                sg.feed(st, _device_rows(dev, E32, lens, other), sg.schedule("odd", lens, fg.T))
                _meets_the_bar(st, ref_s, ref_l, lens, tag + (name, "reset, other storage type"))
                if "peaks70" not in kept:
                    kept["peaks70"] = vo.decode_c(A, pi, E32, lengths=np.minimum(lens, 70))
                short = np.minimum(lens, 70)
                st.reset()                              # shorter recordings: stale rows and pad columns behind the new lengths
                sg.feed(st, _device_rows(dev, E32[:, :70], short, dt), sg.schedule("segments", short, 70))
                _meets_the_bar(st, *kept["peaks70"], short, tag + (name, "reset, 70 frames"))
            st.close()

        # one recording alone, 64 frames an append: every launch uniform (two scalars instead of the per-launch tables)
        name, E32, lens, ref_s, ref_l = batches[2]
        one = sg.schedule("segments", lens[:1], fg.T)
        assert all(sg.uniform_launches(one, 1))
        st = dec.stream(1, sg.T_CAP)
        sg.feed(st, _device_rows(dev, E32[:1], lens[:1], dt), one)
        _meets_the_bar(st, ref_s[:1], ref_l[:1], lens[:1], tag + (name, "one recording"))
        st.close()
    finally:
        dec.set_option("reset", 0)


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("seed", [s for s in fg.WAVE_FORM_SEEDS if sg.WAVE_SEED_SERVED[s]])
def test_wave_form_geometries_as_sessions(dev, seed, f16):
    """Plans that also have the wave form: a session runs the workgroup family all the same (st_family does not ask).  Narrow windows
    on six waves with no, one and two extra columns: a peaks batch on the `segments` schedule."""
    from viterbi_spl_amd import synth
    S, half, extras, A, pi, _ = fg.wave_geometry(seed)
    dec = ViterbiDecoder(A, pi, dev)
    assert dec.info["banded_ok"] and dec.info["floor_ok"] and dec.info["wave_ok"] and dec.info["extras"] == extras, dec.info
    assert (dec.info["group_window"], fg.waves_for(S)) in sg.STREAM_SERVED
    lens = fg.LENGTHS
    E32 = synth.emissions_peaks(len(lens), fg.T, S, seed=40 + seed).to(torch.float16).to(torch.float32).numpy()
    ref_s, ref_l = vo.decode_c(A, pi, E32, lengths=lens)
    sched = sg.schedule("segments", lens, fg.T)
    sg.premise_schedule("segments", sched, lens)
    st = dec.stream(len(lens), sg.T_CAP)
    sg.feed(st, _device_rows(dev, E32, lens, torch.float16 if f16 else torch.float32), sched)
    _meets_the_bar(st, ref_s, ref_l, lens, (seed, f16))
    st.close()


# ------------------------------------------------------------------ 2. step plans
STEP_T_CAP = geo.T_EDGE + 7


@pytest.mark.parametrize("kind", ["jumps", "dense"])
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("S", geo.EDGE_S)
def test_step_kernel_sessions_at_the_edges_of_their_range(dev, S, f16, kind):
    """The Stream variant of the step kernel at 705, 706, 707, 708 and 768 voiced states, recordings of 150, 149, 100, 13, 2 and 1
    frames in sessions of 157 rows: the schedules scaled to 150 frames (launches start at frames 64 and 128), then the lazy
    back-trace as one, seven, 32 and five chunks.  "jumps": the paths step through every distance band (asserted by edge_batch)."""
    A, pi, dec = geo.step_plan(dev, S)
    E, lens, ref_s, ref_l = geo.edge_batch(dev, S, A, pi, kind, f16)
    assert np.array_equal(lens, geo.ragged(geo.T_EDGE))
    B = len(lens)
    En = sg.nan_rows(E, lens)
    tag = (S, "f16" if f16 else "f32", kind)
    st = dec.stream(B, STEP_T_CAP)
    try:
        for sname in sg.SCHEDULES:
            sched = sg.schedule(sname, lens, geo.T_EDGE)
            sg.premise_schedule(sname, sched, lens)
            st.reset()
            sg.feed(st, En, sched)
            _meets_the_bar(st, ref_s, ref_l, lens, tag + (sname,))
        for chunks, warm in BT_STEP:
            dec.set_option("bt_chunks", chunks)
            dec.set_option("bt_warm", warm)
            _meets_the_bar(st, ref_s, ref_l, lens, tag + ("bt", chunks, warm))
            dec.set_option("reset", 0)
    finally:
        dec.set_option("reset", 0)
        st.close()


GATED = [("durrieu", 704, 20, 9), ("durrieu", 769, 20, 9), geo.OTHER[0]]


@pytest.mark.parametrize("case", GATED, ids=geo._id)
def test_the_gate_of_step_sessions(dev, case):
    """704 and 769 voiced states, and an accepted step geometry without a step kernel: the size query answers 0, vit_stream_open
    answers VIT_EUNSUPPORTED with the handle left null and the workspace as it was, ViterbiDecoder.stream raises."""
    A, pi, hp, dec = geo.plan_of(dev, *case)
    assert not dec.info["step_ok"] and not dec.info["banded_ok"]
    assert dec.workspace_bytes_stream(6, STEP_T_CAP) == 0
    lib = _lib.load()
    nbytes = 1 << 24
    buf = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=dev)
    ptr = (buf.data_ptr() + 255) & ~255
    sess = ctypes.c_void_p()
    assert lib.vit_stream_open(dec._plan, 6, STEP_T_CAP, ptr, nbytes, ctypes.byref(sess)) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert not sess.value and bool((buf == 0xA5).all())
    with pytest.raises(_lib.ViterbiHipError):
        dec.stream(6, STEP_T_CAP)


# ------------------------------------------------------------------ 3. the chunk counts the library picks
def _long_session(dev, dec, A, pi, E, forms):
    lens = np.asarray(sg.LONG_LENGTHS, np.int64)
    T = int(lens.max())
    ref_s, ref_l = vo.decode_c(A, pi, E.float().cpu().numpy(), lengths=lens)
    sched = sg.chunked(lens, [sg.LONG_APPEND] * (T // sg.LONG_APPEND))
    assert [n for n, _ in sched] == [768, 768, 768] and sched[1][1].tolist() == [768, 332]
    st = dec.stream(2, sg.LONG_T_CAP)
    try:
        sg.feed(st, sg.nan_rows(E, lens), sched)
        for form in forms:
            dec.set_option("backtrace_form", form)
            _meets_the_bar(st, ref_s, ref_l, lens, ("backtrace_form", form))
            dec.set_option("reset", 0)
    finally:
        dec.set_option("reset", 0)
        st.close()


def test_long_session_natural_chunks_banded(golden, dev):
    """tonet361, two recordings of 2304 and 1100 float16 frames in 768-frame appends (the accumulator's size), rows for 2400, no
    tuning option: the back-trace walks T = 2304 frames as min(16 CUs' waves / 2, 2304 / (8 kBtWarmSparse)) = 4 sparse chunks, and
    under backtrace_form 4 as 2304 / (2 kBtWarmSparse) = 18 lane chunks -- the speculative back-trace with its verify and repair
    passes over a session's rows (hist_rows = 2400 above T, the session's own length table, skip_nonpositive).  The counts follow
    from kBtWarmSparse = 64, kBtMaxChunks = 32, kLaneMaxChunks = 256 and the divisors 8 and 2 of sparse_backtrace_chunks and
    lane_backtrace_chunks; the library has no query for them, tests/test_stream_grid_host.py recomputes them from the sources.
    Emissions: floor_grid.emissions_hops (a hop into every multiple of 64, the launch boundaries 768 and 1536 among them)."""
    A, pi = golden["params"]["tonet361_logA_T"], golden["params"]["tonet361_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    assert dec.info["banded_ok"] and dec.info["floor_ok"]
    E = torch.from_numpy(fg.emissions_hops(2, sg.LONG_LENGTHS[0], dec.S, seed=361)).to(dev).half()
    _long_session(dev, dec, A, pi, E, forms=(0, 4))


def test_long_session_natural_chunks_step(golden, dev):
    """durrieu722, the same shape in float32: 2304 / (8 kBtWarm) = 2 chunks of the lazy kernel (kBtWarm = 128, backtrace_chunks).
    Emissions: tests.common.emissions_jumps (every distance band on the path)."""
    A, pi = golden["params"]["durrieu722_logA_T"], golden["params"]["durrieu722_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    hp = HostPlan(A, pi)
    assert hp.step_ok and dec.info["step_ok"] and not dec.info["banded_ok"]
    E = torch.from_numpy(emissions_jumps(2, sg.LONG_LENGTHS[0], dec.S, 722, hp.step_bw)).to(dev)
    _long_session(dev, dec, A, pi, E, forms=(0,))
