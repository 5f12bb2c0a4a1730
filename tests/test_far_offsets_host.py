"""Host tier of the far-offset tests (tests/far_offsets.py): the shape arithmetic against the library's own size queries, and the
proof that the expected values of constructions B and C equal ONE plain oracle run -- at marks scaled down to 2^16 (C) and 2^18 (B) elements, on
every plan the GPU tier uses, float32 and float16, and the float64 family against tests/f64_ref.py.  No GPU."""
import os

import numpy as np
import pytest

from oracle import viterbi_oracle as vo
from tests import f64_ref, far_offsets as fo
from tests.common import f32_bits

SMALL = 1 << 16                     # the scaled-down mark: element 65536, byte 131072
PLANS_C = ("tonet361", "jdc722", "durrieu722", "msnet321")
PLANS_F64 = ("tonet361", "jdc722")


@pytest.fixture(scope="module")
def lib():
    from viterbi_spl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _params(golden, name):
    return golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]


def test_marks():
    assert fo.mark_elements(4) == [1 << 30, 1 << 31] and fo.mark_elements(2) == [1 << 31] and fo.mark_elements(8) == [1 << 29, 1 << 31]
    assert fo.mark_rows(361, 4) == [(1 << 30) // 361, (1 << 31) // 361]
    n = fo.rows_past([(361, 4), (384, 4)])
    assert (n - 1) * 361 <= 1 << 31 < n * 361 + 361 and n * 361 > 1 << 31 and n * 384 * 4 > 1 << 32
    assert fo.rows_past([(722, 2)]) * 722 > 1 << 31 and (fo.rows_past([(722, 2)]) - 1) * 722 <= 1 << 31


@pytest.mark.parametrize("name", fo.PLANS_A)
def test_history_rows_come_from_the_size_queries(lib, golden, name):
    """The strides the constructions are sized by are the library's: one song of T frames costs T rows, and two songs start T rows
    apart.  What the header documents -- ceil((S + 2) / 4) * 4 floats for the workgroup kernels, 64 * ceil(S / 64) for the wave form
    -- is what the queries answer; a new layout moves the marks' rows with it instead of silently missing them."""
    A, pi = _params(golden, name)
    S = A.shape[0]
    plan = fo.create_plan(lib, A, pi)
    rows = fo.history_rows(lib, plan)
    lib.vit_plan_destroy(plan)
    assert "dense" in rows and rows["dense"] == ((S + 5) // 4 * 4, 4)
    if "wave" in rows:
        assert rows["wave"] == (64 * -(-S // 64), 4)
    if "f64" in rows:
        assert rows["f64"][1] == 8 and rows["f64"][0] >= S
    for name_, (r, i) in rows.items():
        assert r >= S, name_
        B, T = fo.shape_a(S, 2, (r, i))
        assert T * S > 1 << 31 and T * S * 2 > 1 << 32 and T * r * i > 1 << 32 and (T - 1) * S <= 1 << 31 and B in (2, 3)
        B, T = fo.shape_b(S, 4, (r, i))
        assert B % 8 == 0 and B * T * S > 1 << 31 and (B - 8) * T * S <= 1 << 31
        nb = fo.count_b_packed(S, 2, (r, i), fo.LENS_B)
        off = fo.packed_offsets(nb, fo.LENS_B)
        assert off[-1] * S > 1 << 31 and off[-9] * S <= 1 << 31
        picks = fo.straddlers(off, [(S, 2), (r, i)])
        assert picks[0] == 0 and picks[-1] == nb - 1 and len(picks) >= 3


def test_probe_rows():
    rows = fo.probe_rows(6_000_000, [(360, 4), (361, 4)], seed=1)
    assert rows[0] == 0 and rows[-1] == 5_999_999 and len(rows) > 4096
    for r in fo.mark_rows(360, 4) + fo.mark_rows(361, 4):
        assert r in rows and r - 32 in rows and r + 31 in rows


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("name", PLANS_C)
def test_piecewise_expectation_equals_the_plain_oracle(lib, golden, name, f16):
    """Construction C at the scaled-down mark: the expectation chained island by island (the survivor's score through the stretches
    by the one-state oracle) is, bit for bit, what one vo.decode_c run over the whole recording returns."""
    A, pi = _params(golden, name)
    S = A.shape[0]
    plan = fo.create_plan(lib, A, pi)
    rows = fo.history_rows(lib, plan)
    lib.vit_plan_destroy(plan)
    buffers = [(S, 2 if f16 else 4)] + sorted(set(rows.values()))
    for kind, seed in (("peaks", 3), ("dense", 4), ("ties", 5)):
        c = fo.recording_c(A, pi, f16, buffers, kind, seed, island=12, mark=SMALL)
        assert len(c["spans"]) >= 3 and c["spans"][0][0] == 0 and c["spans"][-1][1] == c["N"]
        E = np.empty((c["N"], S), np.float16 if f16 else np.float32)
        fo.fill_recording(E, c["k"], c["v"], c["spans"], c["islands"])
        assert np.isfinite(E).sum(axis=1).min() >= 1 and (np.isfinite(E).sum(axis=1) == 1).any()
        st, ll = vo.decode_c(A, pi, E.astype(np.float32)[None])
        assert np.array_equal(st[0], c["states"]), (name, kind)
        assert f32_bits(ll)[0] == f32_bits(c["loglik"]), (name, kind, ll, c["loglik"])
        inside = np.zeros(c["N"], bool)
        for s, e in c["spans"]:
            inside[s:e] = True
        assert np.all(c["states"][~inside] == c["k"])
        assert any(np.any(c["states"][s:e] != c["k"]) for s, e in c["spans"]), "the islands must leave the survivor's state"


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("name", PLANS_F64)
def test_piecewise_expectation_equals_the_float64_reference(lib, golden, name, f16):
    """The same for the float64 family: the chained expectation against tests/f64_ref.decode_f64 over the whole recording."""
    A, pi = _params(golden, name)
    S = A.shape[0]
    plan = fo.create_plan(lib, A, pi)
    rows = fo.history_rows(lib, plan)
    lib.vit_plan_destroy(plan)
    assert "f64" in rows
    c = fo.recording_c(A, pi, f16, [(S, 2 if f16 else 4), rows["f64"]], "peaks", 6, island=12, mark=SMALL, f64=True)
    E = np.empty((c["N"], S), np.float16 if f16 else np.float32)
    fo.fill_recording(E, c["k"], c["v"], c["spans"], c["islands"])
    st, d = f64_ref.decode_f64(A, pi, E.astype(np.float32))
    assert np.array_equal(st, c["states"])
    assert f64_ref.bits64(d[st[-1]]) == f64_ref.bits64(c["loglik"])


SMALL_B = 1 << 18                  # construction B's scaled-down mark: three periods of eight 40-frame recordings at 361 states
LENS_SMALL = (40, 39, 37, 1, 38, 40, 21, 27)
CASES_B = [("tonet361", False), ("tonet361", True), ("msnet321", False), ("msnet321", True), ("jdc722", True), ("jdc722", False),
           ("durrieu722", True)]                                   # every plan and storage type of tests/test_gpu_far_offsets_b.py


def _whole_batch(p, S, dtype):
    """The packed batch of fo.packed_batch_b as ONE padded [B, 40, S] batch with lengths: what a plain oracle run takes."""
    off = p["off"]
    B = p["B"]
    rows = np.tile(p["period"], (B // 8, 1))
    assert rows.shape[0] == off[-1]
    lens = np.diff(off)
    E = np.zeros((B, int(lens.max()), S), dtype)
    for b in range(B):
        E[b, :lens[b]] = rows[off[b]:off[b + 1]]
    return E, lens


def _tiled_equals(p, states, loglik, lens, bits):
    """What the GPU tier asserts, on the plain run's output: the recordings picked one by one, then the whole batch against the tiled
    expectation."""
    B, off = p["B"], p["off"]
    packed = np.concatenate([states[b, :lens[b]] for b in range(B)])
    for b in p["picks"]:
        assert np.array_equal(packed[off[b]:off[b + 1]], p["ref_s"][b % 8, :lens[b]]), b
    assert np.array_equal(packed.reshape(B // 8, -1), np.tile(p["want"], (B // 8, 1)))
    assert np.array_equal(bits(loglik).reshape(B // 8, 8), np.tile(bits(p["ref_l"]), (B // 8, 1)))


@pytest.mark.parametrize("name,f16", CASES_B, ids=[f"{n}-{'f16' if h else 'f32'}" for n, h in CASES_B])
def test_tiled_expectation_equals_the_plain_oracle(lib, golden, name, f16):
    """Construction B at a scaled-down mark, through the helpers the GPU tier uses (count_b_packed, packed_offsets, straddlers, the
    concatenated `want`): the expectation tiled from the oracle's decode of the 8 distinct recordings equals one plain oracle run
    over every recording of the batch, for the packed history row and the workgroup one."""
    A, pi = _params(golden, name)
    S = A.shape[0]
    plan = fo.create_plan(lib, A, pi)
    rows = fo.history_rows(lib, plan)
    lib.vit_plan_destroy(plan)
    base = fo.base_songs(S, 40, f16, seed=9)
    for hist in sorted({rows["packed"], rows["dense"]}):
        p = fo.packed_batch_b(A, pi, base, LENS_SMALL, hist, f16, mark=SMALL_B)
        assert p["B"] >= 16 and p["B"] % 8 == 0 and len(p["picks"]) >= 3 and p["picks"][0] == 0 and p["picks"][-1] == p["B"] - 1
        assert (p["off"][-9] * S <= max(fo.mark_elements(2 if f16 else 4, SMALL_B))
                or p["off"][-9] * hist[0] <= max(fo.mark_elements(hist[1], SMALL_B))), "eight recordings fewer do not reach the marks"
        E, lens = _whole_batch(p, S, base.dtype)
        st, ll = vo.decode_c(A, pi, E.astype(np.float32), lengths=lens)
        _tiled_equals(p, st, ll, lens, f32_bits)
    B, T = fo.shape_b(S, 2 if f16 else 4, rows["dense"], T=40, mark=SMALL_B)          # the padded batches: B songs of T frames
    assert B % 8 == 0 and B * T * S > SMALL_B and (B - 8) * T * S <= max(SMALL_B, 2 * SMALL_B // (2 if f16 else 4))


@pytest.mark.parametrize("name,f16", [("tonet361", False), ("jdc722", True), ("msnet321", True)], ids=["tonet361-f32", "jdc722-f16", "msnet321-f16"])
def test_tiled_expectation_equals_the_float64_reference(lib, golden, name, f16):
    """The same for the float64 packed decodes: tests/f64_ref.py on the 8 recordings, tiled, against tests/f64_ref.py on every
    recording of the batch."""
    A, pi = _params(golden, name)
    S = A.shape[0]
    plan = fo.create_plan(lib, A, pi)
    rows = fo.history_rows(lib, plan)
    lib.vit_plan_destroy(plan)
    base = fo.base_songs(S, 40, f16, seed=10)
    p = fo.packed_batch_b(A, pi, base, LENS_SMALL, rows["f64_packed"], f16, f64=True, mark=SMALL_B)
    E, lens = _whole_batch(p, S, base.dtype)
    st, ll = f64_ref.decode_f64_batch(A, pi, E.astype(np.float32), lens)
    _tiled_equals(p, st.astype(np.int32), ll, lens, f64_ref.bits64)
