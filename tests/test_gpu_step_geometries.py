"""Step-structured plans on the GPU at the geometries the plan accepts (tests/test_step_plan_host.py proves the plans on the CPU):

1. the forward step kernels at the edges of their range -- 705 .. 768 voiced states, every fill of the last quad of states --
   through decode (both step forms and the plain dense kernel), decode_checkpointed, decode_packed and decode_packed_bounded;
2. the gate: 704 and 769 voiced states take the dense kernel, and the segment / packed entry points refuse them;
3. every other accepted geometry: the dense forward kernels (matrix-resident up to 368 states, streaming above) with the
   back-trace that reads the (kb + 1) x SP band table through the multiply-shift band index;
4. the chunked back-trace with many chunks and no warm-up on step plans.

States and log-likelihood bits equal oracle.viterbi_oracle.decode_c everywhere (signed zeros: log-likelihood by value).  Every test
asserts which plan flags hold and which forward family runs, so that a case that takes another kernel fails."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests.common import GEN, durrieu_log_params, emissions_jumps, jump_seed, path_bands, step_matrix
from tests.plan_replay import HostPlan
from viterbi_spl_amd import ViterbiDecoder, _lib

pytestmark = pytest.mark.gpu

EUNSUPPORTED = -5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _uniform(n):
    return np.full(n + 1, np.float32(np.log(np.float32(1.0 / (n + 1)))), np.float32)


_plans = {}


def plan_of(dev, kind, n, bw, kb=9):
    """(A, pi, HostPlan, ViterbiDecoder) of one geometry, built once per session; the premises every test states first."""
    key = (kind, n, bw, kb)
    if key not in _plans:
        if kind == "durrieu":
            A, pi = durrieu_log_params(n, bw)
        else:
            A, pi = step_matrix(n, bw, kb, np.random.default_rng(1000 * n + 16 * bw + kb)), _uniform(n)
        _plans[key] = (A, pi, HostPlan(A, pi), ViterbiDecoder(A, pi, dev))
    A, pi, hp, dec = _plans[key]
    assert hp.step_ok and (hp.step_bw, hp.step_kb) == (bw, kb) and not hp.ok, (key, hp.step_ok, hp.step_bw, hp.step_kb, hp.ok)
    assert not dec.info["banded_ok"] and not dec.info["wave_ok"]
    dec.set_option("reset", 0)
    return A, pi, hp, dec


def ragged(T):
    return np.asarray([T, T - 1, min(100, T), min(13, T), 2, 1], np.int64)


_inputs = {}


def batch(dev, tag, A, pi, T, kind, f16, seed, bw=None):
    """Emissions [6, T, S] on the device, ragged lengths and the oracle's answer for the plan `tag`, computed once and shared.
    kind "jumps": tests.common.emissions_jumps (needs the band width)."""
    key = (tag, T, kind, f16, seed)
    if key not in _inputs:
        dt = torch.float16 if f16 else torch.float32
        if kind == "jumps":
            E = torch.from_numpy(emissions_jumps(6, T, A.shape[0], seed, bw)).to(dev).to(dt)
        else:
            E = GEN[kind](6, T, A.shape[0], seed=seed, device=dev, dtype=dt)
        lens = ragged(T)
        ref_s, ref_l = vo.decode_c(A, pi, E.float().cpu().numpy(), lengths=lens)
        _inputs[key] = (E, lens, ref_s, ref_l)
    return _inputs[key]


def all_bands_on_the_path(ref_s, lens, n, bw, kb):
    """Premise of the "jumps" batches: the oracle's paths step through every distance band, the far one included."""
    assert path_bands(ref_s, lens, n, bw, kb) == list(range(kb + 1)), path_bands(ref_s, lens, n, bw, kb)


def check(st, ll, ref_s, ref_l, tag, by_value=False):
    st, ll = st.cpu().numpy(), ll.cpu().numpy()
    assert np.array_equal(st, ref_s), (tag, np.argwhere(st != ref_s)[:6])
    if by_value:
        assert np.array_equal(ll, ref_l), (tag, ll, ref_l)
    else:
        assert np.array_equal(_bits(ll), _bits(ref_l)), (tag, ll, ref_l)


# ------------------------------------------------------------------ 1. the forward step kernels at the edges of their range
EDGE_S = (706, 707, 708, 709, 769)      # n = 705: one state in the last quad | two | three | a full quad | 768: the last lane full
T_EDGE = 150


def step_plan(dev, S):
    A, pi, hp, dec = plan_of(dev, "durrieu", S - 1, 20)
    assert dec.info["step_ok"], "premise: the forward step kernel is instantiated for this plan"
    assert dec.forward_family(6, "auto") == "dense" and dec.forward_family(6, "dense") == "dense"
    return A, pi, dec


def edge_batch(dev, S, A, pi, kind, f16):
    if kind != "jumps":
        return batch(dev, S, A, pi, T_EDGE, kind, f16, seed=S)
    out = batch(dev, S, A, pi, T_EDGE, kind, f16, seed=jump_seed("durrieu", S - 1, 20, 9), bw=20)
    all_bands_on_the_path(out[2], out[1], S - 1, 20, 9)
    return out


@pytest.mark.parametrize("kind", ["dense", "ties", "jumps"])
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("S", EDGE_S)
def test_step_kernels_at_the_edges_of_their_range(dev, S, f16, kind):
    """algo "auto" with both step forms (bands split over two waves | one wave per lane group) and the plain dense kernel: a ragged
    batch [T, T - 1, 100, 13, 2, 1], then batches whose own T is 1, 2 and 3 (the prefetch tails).  Emissions: i.i.d. values, ties,
    and "jumps" (paths that step through every distance band: the far maximum and every band window decide)."""
    A, pi, dec = step_plan(dev, S)
    E, lens, ref_s, ref_l = edge_batch(dev, S, A, pi, kind, f16)
    lens_d = torch.from_numpy(lens).to(dev)
    for algo, form in (("auto", 0), ("auto", 3), ("dense", 0)):
        dec.set_option("step_form", form)
        st, ll = dec.decode(E, lengths=lens_d, algo=algo, out_dtype=torch.int32)
        check(st, ll, ref_s, ref_l, (S, f16, kind, algo, form))
        for Ts in (1, 2, 3):
            Es = E[:3, :Ts].contiguous()
            rs, rl = vo.decode_c(A, pi, Es.float().cpu().numpy())
            st, ll = dec.decode(Es, algo=algo, out_dtype=torch.int32)
            check(st, ll, rs, rl, (S, f16, kind, algo, form, "T", Ts))
    dec.set_option("reset", 0)


@pytest.mark.parametrize("kind", ["dense", "ties", "jumps"])
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("S", (707, 769))
def test_step_kernel_variants_at_the_edges(dev, S, f16, kind):
    """The Ckpt, Packed and PackedCkpt variants of the step kernels (decode_checkpointed, decode_packed, decode_packed_bounded with
    segments of 64 frames); the ragged lengths are the recordings, each compared with the oracle."""
    A, pi, dec = step_plan(dev, S)
    E, lens, ref_s, ref_l = edge_batch(dev, S, A, pi, kind, f16)
    B = len(lens)
    lens_d = torch.from_numpy(lens).to(dev)
    assert dec.workspace_bytes_checkpointed_or_zero(B, T_EDGE, 64) > 0
    st, ll = dec.decode_checkpointed(E, segment_frames=64, lengths=lens_d, out_dtype=torch.int32)
    check(st, ll, ref_s, ref_l, (S, f16, kind, "checkpointed"))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Ep = torch.cat([E[b, :int(lens[b])] for b in range(B)], dim=0).contiguous()
    assert dec.workspace_bytes_packed(B, int(off[-1])) > 0
    for name, run in (("packed", lambda: dec.decode_packed(Ep, off, out_dtype=torch.int32)),
                      ("packed_bounded", lambda: dec.decode_packed_bounded(Ep, off, segment_frames=64, out_dtype=torch.int32))):
        sp, lp = run()
        sp, lp = sp.cpu().numpy(), lp.cpu().numpy()
        assert np.array_equal(_bits(lp), _bits(ref_l)), (S, f16, kind, name, lp, ref_l)
        for b in range(B):
            assert np.array_equal(sp[off[b]:off[b + 1]], ref_s[b, :lens[b]]), (S, f16, kind, name, b)


# ------------------------------------------------------------------ 2. the gate
@pytest.mark.parametrize("S", (705, 770))
def test_the_gate_of_the_step_kernels(dev, S):
    """704 and 769 voiced states: the plan proves the step structure (20-bin bands, nine near bands), the forward step kernel is
    not instantiated -- "auto" and "dense" both run the dense kernel and equal the oracle, and the segment and packed entry points
    refuse the plan the way they refuse an unstructured matrix: size 0, VIT_EUNSUPPORTED, nothing enqueued."""
    A, pi, hp, dec = plan_of(dev, "durrieu", S - 1, 20)
    assert not dec.info["step_ok"], "premise: outside the instantiated range"
    assert dec.forward_family(6, "auto") == "dense"
    for f16, kind in ((False, "dense"), (True, "ties"), (False, "jumps"), (True, "jumps")):
        if kind == "jumps":
            E, lens, ref_s, ref_l = batch(dev, S, A, pi, T_EDGE, kind, f16, seed=jump_seed("durrieu", S - 1, 20, 9), bw=20)
            all_bands_on_the_path(ref_s, lens, S - 1, 20, 9)
        else:
            E, lens, ref_s, ref_l = batch(dev, S, A, pi, 100, kind, f16, seed=S)
        lens_d = torch.from_numpy(lens).to(dev)
        for algo in ("auto", "dense"):
            st, ll = dec.decode(E, lengths=lens_d, algo=algo, out_dtype=torch.int32)
            check(st, ll, ref_s, ref_l, (S, f16, kind, algo))
    E, lens, ref_s, ref_l = batch(dev, S, A, pi, 100, "dense", False, seed=S)
    B, T = E.shape[0], E.shape[1]
    lens_d = torch.from_numpy(lens).to(dev)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(off[-1])
    Ep = torch.cat([E[b, :int(lens[b])] for b in range(B)], dim=0).contiguous()
    lib, p = _lib.load(), dec._plan
    assert dec.workspace_bytes_checkpointed_or_zero(B, T, 64) == 0
    assert dec.workspace_bytes_packed(B, N) == 0
    assert int(lib.vit_workspace_bytes_packed_bounded(p, B, off.ctypes.data, 64)) == 0
    assert int(lib.vit_workspace_bytes_packed_checkpointed(p, B, off.ctypes.data, 64)) == 0
    with pytest.raises(_lib.ViterbiHipError):
        dec.decode_checkpointed(E, segment_frames=64, lengths=lens_d)
    with pytest.raises(_lib.ViterbiHipError):
        dec.decode_packed(Ep, off)
    with pytest.raises(_lib.ViterbiHipError):
        dec.decode_packed_bounded(Ep, off, segment_frames=64)
    # the raw calls with a workspace that would be large enough for any of them
    big = 1 << 27
    buf = torch.empty(big + 512, dtype=torch.uint8, device=dev)
    ws = (buf.data_ptr() + 255) & ~255
    states = torch.full((B * T,), 12345, dtype=torch.int32, device=dev)
    loglik = torch.full((B,), 7.0, dtype=torch.float32, device=dev)
    st, ll = states.data_ptr(), loglik.data_ptr()
    f32 = _lib.VIT_F32
    assert lib.vit_decode_checkpointed(p, E.data_ptr(), f32, B, T, lens_d.data_ptr(), ws, big, st, ll, 64, None) == EUNSUPPORTED
    assert lib.vit_decode_packed(p, Ep.data_ptr(), f32, B, off.ctypes.data, ws, big, st, ll, None) == EUNSUPPORTED
    assert lib.vit_decode_packed_bounded(p, Ep.data_ptr(), f32, B, off.ctypes.data, ws, big, st, ll, 64, None) == EUNSUPPORTED
    assert lib.vit_decode_packed_checkpointed(p, Ep.data_ptr(), f32, B, off.ctypes.data, ws, big, st, ll, 64, None) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((states == 12345).all()) and bool((loglik == 7.0).all()), "a refused call wrote its outputs"
    # and a decode still runs afterwards
    st2, ll2 = dec.decode(E, lengths=lens_d, out_dtype=torch.int32)
    check(st2, ll2, ref_s, ref_l, (S, "after the refusals"))


# ------------------------------------------------------------------ 3. dense forward, step-table back-trace
OTHER = [("durrieu", 128, 4, 9), ("durrieu", 300, 16, 9), ("durrieu", 367, 5, 9), ("durrieu", 368, 8, 9), ("durrieu", 500, 7, 9),
         ("durrieu", 641, 64, 9), ("durrieu", 1023, 64, 9),
         ("generated", 128, 4, 1), ("generated", 128, 4, 15), ("generated", 199, 12, 15), ("generated", 400, 5, 3),
         ("generated", 1023, 63, 15), ("generated", 1023, 64, 14)]


def _id(case):
    return "%s-n%d-bw%d-kb%d" % case


def other_plan(dev, case):
    A, pi, hp, dec = plan_of(dev, *case)
    assert not dec.info["step_ok"], "premise: no forward step kernel for this geometry"
    assert dec.forward_family(6, "auto") == "dense"
    return A, pi, dec


@pytest.mark.parametrize("kind", ["dense", "ties", "jumps"])
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("case", OTHER, ids=_id)
def test_dense_forward_with_the_step_table_backtrace(dev, case, f16, kind):
    """Step-structured plans without a forward step kernel: decode(algo="auto") runs a dense forward kernel, and every row of the
    back-trace takes the band-table branch of the generic kernel -- other band widths (the multiply-shift division), other table
    strides, one to fifteen near bands (the clamp), and the largest table (16 rows of 1024 floats in LDS)."""
    _, n, bw, kb = case
    A, pi, dec = other_plan(dev, case)
    T = 100 if n + 1 > 800 else 150
    if kind == "jumps":     # the i.i.d. kinds keep the path in the nearest bands; these step through every band
        E, lens, ref_s, ref_l = batch(dev, case, A, pi, T, kind, f16, seed=jump_seed(*case), bw=bw)
        all_bands_on_the_path(ref_s, lens, n, bw, kb)
    else:
        E, lens, ref_s, ref_l = batch(dev, case, A, pi, T, kind, f16, seed=n + bw)
    st, ll = dec.decode(E, lengths=torch.from_numpy(lens).to(dev), algo="auto", out_dtype=torch.int32)
    check(st, ll, ref_s, ref_l, (case, f16, kind))


def test_zero_bands_and_signed_zero_emissions(dev):
    """A generated matrix whose nearest bands are +0 (one sign per band: a mix is not a step matrix), a prior and emissions of +0
    and -0: the paths equal the oracle's, the log-likelihoods are equal by value (the sign of a zero sum is free)."""
    n, bw, kb = 199, 12, 15
    rng = np.random.default_rng(31)
    A = step_matrix(n, bw, kb, rng, zero_top=True)
    pi = np.where(rng.random(n + 1) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    hp = HostPlan(A, pi)
    assert hp.step_ok and (hp.step_bw, hp.step_kb) == (bw, kb) and not hp.ok
    assert np.any(_bits(A[:n, :n]) == 0) and not np.any(_bits(A[:n, :n]) == 0x80000000)
    dec = ViterbiDecoder(A, pi, dev)
    assert not dec.info["step_ok"] and not dec.info["banded_ok"] and dec.forward_family(6, "auto") == "dense"
    T = 150
    E = np.where(rng.random((6, T, n + 1)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    E[:, ::7] = -(rng.integers(0, 3, (6, len(range(0, T, 7)), n + 1)) / 2).astype(np.float32)
    lens = ragged(T)
    ref_s, ref_l = vo.decode_c(A, pi, E, lengths=lens)
    assert np.all(np.isfinite(ref_l))
    for f16 in (False, True):                               # (+-0, -0.5 and -1 are exact in float16: one oracle run serves both)
        Ed = torch.from_numpy(E).to(dev)
        Ed = Ed.half() if f16 else Ed
        assert np.any(_bits(Ed.float().cpu().numpy()) == 0x80000000)
        st, ll = dec.decode(Ed, lengths=torch.from_numpy(lens).to(dev), algo="auto", out_dtype=torch.int32)
        check(st, ll, ref_s, ref_l, ("signed zeros", f16), by_value=True)


# ------------------------------------------------------------------ 4. chunked back-trace on step plans
CHUNKED = ["durrieu722", ("durrieu", 706, 20, 9), ("durrieu", 300, 16, 9), ("generated", 199, 12, 15)]
CHUNK_SEED = 77


@pytest.mark.parametrize("kind", ["dense", "jumps"])
@pytest.mark.parametrize("case", CHUNKED, ids=lambda c: c if isinstance(c, str) else _id(c))
def test_chunked_backtrace_on_step_plans(golden, dev, case, kind):
    """Many chunks and no warm-up (most guessed entry states are wrong: the verify-and-repair pass does the work), one warm-up frame
    with every row through the general code, and chunkings that coalesce -- on the golden Durrieu plan, on a forward-kernel edge
    (S = 707) and on two geometries that decode with the dense kernel and the band table.  States and log-likelihood equal the
    oracle for "auto" and "dense".

    The generic (lazy) back-trace kernel that serves every plan here records no event counters (tests/golden/bt_counters.json,
    durrieu722_lazy: all zeros), so chunks_repaired cannot be read back and is not asserted.  In its place the premise is checked
    on the oracle's output: without a warm-up chunk c assumes the lowest-index arg-max of delta row hi_c as its entry state
    (bt_run_chunks, backtrace_common.hpp), and for the (7, 0) chunking that guess must differ from the path's state at frame hi_c
    for at least one chunk -- so a repair pass that did nothing would leave a wrong path."""
    if isinstance(case, str):
        A, pi = golden["params"][f"{case}_logA_T"], golden["params"][f"{case}_log_pi"]
        dec = ViterbiDecoder(A, pi, dev)
        hp = HostPlan(A, pi)
        assert hp.step_ok and not hp.ok and dec.info["step_ok"] and not dec.info["banded_ok"]
    else:
        A, pi, hp, dec = plan_of(dev, *case)
        assert dec.info["step_ok"] == (case[1] == 706)
    assert dec.forward_family(3, "auto") == "dense"
    S = A.shape[0]
    lens = np.asarray([700, 333, 2], np.int64)
    lens_d = torch.from_numpy(lens).to(dev)
    if kind == "jumps":
        E = torch.from_numpy(emissions_jumps(3, 700, S, CHUNK_SEED, hp.step_bw)).to(dev)
    else:
        E = GEN["dense"](3, 700, S, seed=CHUNK_SEED, device=dev)
    ref_s, ref_l = vo.decode_c(A, pi, E.cpu().numpy(), lengths=lens)
    if kind == "jumps":
        all_bands_on_the_path(ref_s, lens, S - 1, hp.step_bw, hp.step_kb)
    # premise: with seven chunks and no warm-up at least one chunk starts from a wrong guess
    wrong = 0
    Eh = E.cpu().numpy()
    for b in (0, 1):
        Lf = int(lens[b]) - 1
        hi = np.asarray([Lf * (c + 1) // 7 for c in range(6)], np.int64)
        _, _, rows = vo.decode_c(A, pi, np.ascontiguousarray(np.broadcast_to(Eh[b][None], (6,) + Eh[b].shape)), lengths=hi + 1, return_delta=True)
        wrong += int(np.sum(np.argmax(rows, axis=1) != ref_s[b, hi]))
    assert wrong > 0, "premise: every guess of the (7, 0) chunking is right -- pick another seed"
    for chunks, warm in ((7, 0), (32, 1), (5, 40), (2, 10000)):
        dec.set_option("bt_chunks", chunks)
        dec.set_option("bt_warm", warm)
        dec.set_option("bt_fast_rows", 1 if warm == 1 else 0)
        for algo in ("auto", "dense"):
            st, ll = dec.decode(E, lengths=lens_d, algo=algo, out_dtype=torch.int32)
            check(st, ll, ref_s, ref_l, (case, chunks, warm, algo))
    dec.set_option("reset", 0)
