"""Value edges on the GPU: every kernel family decodes -inf entries, songs that die (a whole -inf emission frame, starvation through
a -inf matrix floor, a -inf prior, float32 overflow), absorbed matrix entries, signed zeros and the float16 edge values (+-0,
subnormals, the smallest normal, -65504, -inf) to the oracle's bits.  The oracle's answer for a dead song: a frame whose delta row
is all -inf resolves every back-pointer to state 0, the terminal state is 0, the log-likelihood -inf (0xff800000).

The inputs are those of tests/test_value_edges_host.py (tests/common.py edge_cases); each one's premise is asserted on the oracle's
output before a kernel result is looked at, the oracle runs once per input and its result is shared by every kernel form.  Every
test asserts through dec.info / forward_family / history_mode that the family it names is the one that runs."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests import common as cm
from tests.test_plan_host import _banded_matrix
from viterbi_spl_amd import ViterbiDecoder, _lib

pytestmark = pytest.mark.gpu

T_SHORT, T_MID, T_LONG = 70, 130, 260       # 722-state grids | the other families | where the back-trace is cut into chunks
HALF = {"tonet361": 14, "msnet321": 12, "jdc722": 40, "imm722w": 56, "jdc721": 40}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _golden(golden, name, inf_floor=False):
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    return (cm.inf_floor_sibling(A) if inf_floor else A), pi


def _band(S, half, extras=(), dense_rows=(), seed=0):
    rng = np.random.default_rng(1000 * S + half + seed)
    return (_banded_matrix(S, half, rng, extras=extras, dense_rows=dense_rows, floor=-np.inf, quant=2),
            -(rng.integers(0, 8, S) / 2).astype(np.float32))


class Case:
    """One input with the oracle's answer (computed once, premise asserted), its tensors on the GPU and its decoder."""

    def __init__(self, dev, name, A, pi, E32, E16, lens, premise, by_value):
        self.name, self.A, self.pi, self.by_value, self.S = name, A, pi, by_value, A.shape[0]
        self.lens_h = np.asarray(lens, np.int64)
        self.ref_s, self.ref_l = vo.decode_c(A, pi, E32, lengths=self.lens_h)
        premise(self.ref_s, self.ref_l)                      # on the oracle alone, before any kernel runs
        self.ref_s.setflags(write=False)
        self.ref_l.setflags(write=False)
        self.E = torch.from_numpy(E16 if E16 is not None else E32).to(dev)
        self.lens = torch.from_numpy(self.lens_h).to(dev)
        self.B, self.T = E32.shape[:2]
        self.dec = ViterbiDecoder(A, pi, dev)

    def check(self, st, ll, tag):
        st, ll = st.cpu().numpy(), ll.cpu().numpy()
        assert not np.isnan(ll).any(), (self.name, tag, ll)
        for b in range(self.B):
            n = int(self.lens_h[b])
            assert np.all((st[b, :n] >= 0) & (st[b, :n] < self.S)), (self.name, tag, b, st[b, :n].min(), st[b, :n].max())
        bad = np.argwhere(st != self.ref_s)
        assert bad.size == 0, (self.name, tag, "first differing (song, frame)", bad[:4].tolist())
        if self.by_value:                                    # +0 and -0 are the same maximum
            assert np.array_equal(ll, self.ref_l), (self.name, tag, ll, self.ref_l)
        else:
            assert np.array_equal(cm.f32_bits(ll), cm.f32_bits(self.ref_l)), (self.name, tag, ll, self.ref_l)

    def run(self, algo, options, tag=None):
        """One padded decode under the forced options, compared with the oracle; the options are reset afterwards."""
        try:
            for k, v in options.items():
                self.dec.set_option(k, v)
            st, ll = self.dec.decode(self.E, lengths=self.lens, algo=algo, out_dtype=torch.int32)
        finally:
            self.dec.set_option("reset", 0)
        self.check(st, ll, tag or (algo, options))

    def packed(self, order):
        """The songs `order` without padding -> (emissions [sum T_b, S], host offsets)."""
        ln = self.lens_h[list(order)]
        off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
        return torch.cat([self.E[b, :int(self.lens_h[b])] for b in order], dim=0).contiguous(), off

    def check_packed(self, sp, lp, order, off, tag):
        B, T = len(order), self.T
        st = torch.full((self.B, T), -1, dtype=torch.int32, device=sp.device)
        ll = torch.zeros(self.B, dtype=torch.float32, device=sp.device)
        assert sorted(order) == list(range(self.B))
        for k, b in enumerate(order):
            st[b, :int(self.lens_h[b])] = sp[int(off[k]):int(off[k + 1])]
            ll[b] = lp[k]
        self.check(st, ll, tag)


def _cases(dev, seed, A, pi, T, half=None, f16=False, only=None):
    for name, A2, pi2, E32, E16, lens, premise, by_value in cm.edge_cases(seed, A, pi, T, half=half, f16=f16, only=only):
        yield Case(dev, name, A2, pi2, E32, E16, lens, premise, by_value)


def _expected_classes(A, half, f16):
    inf_floor = bool(np.isneginf(A).any())
    names = {"sparse_inf", "dead_frame0", "dead_frame1", "dead_prior", "dead_prior_all", "signed_zeros"}
    names |= {"fp16_edges", "fp16_edges_dead"} if f16 else {"overflow_dead", "absorbing"}
    names |= {"starved"} if inf_floor else set()
    names |= {"single_survivor"} if inf_floor and half else set()
    return names


F16 = pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])


# ------------------------------------------------------------------ workgroup form, 32-wide windows
@F16
@pytest.mark.parametrize("which", ["tonet361", "tonet361_inf", "band361", "band383"])
def test_workgroup_form_with_32_wide_windows(golden, dev, which, f16):
    """forward_form 1 (one target per lane), 2 (two targets), 3 (scan form), 6 (split windows) x backtrace_form 0 / 1 / 2 / 4."""
    if which.startswith("tonet"):
        A, pi = _golden(golden, "tonet361", which.endswith("_inf"))
        half = 14
    else:
        S = int(which[4:])
        A, pi = _band(S, 14, extras=(S - 1,) if S == 383 else ())
        half = 14
    seen = set()
    for c in _cases(dev, 11 + f16, A, pi, T_MID, half=half, f16=f16):
        info = c.dec.info
        assert info["banded_ok"] and info["floor_ok"] and info["group_window"] == 32 and info["n_dense_rows"] == 0, (c.name, info)
        assert c.dec.forward_family(c.B, "group") == "group" and c.dec.history_mode(c.B, c.T, "group") == "full"
        for form in (1, 2, 3, 6):
            for bt in (0, 1, 2, 4):
                c.run("group", {"forward_form": form, "backtrace_form": bt})
        seen.add(c.name)
    assert seen == _expected_classes(A, half, f16), seen


@F16
def test_scan_form_with_dense_rows(dev, f16):
    """Two dense rows: the plan has no floor form, the scan form runs and the generic back-trace decides the dense rows."""
    A, pi = _band(361, 10, extras=(360,), dense_rows=(7, 100))
    seen = set()
    for c in _cases(dev, 13 + f16, A, pi, T_MID, half=10, f16=f16):
        info = c.dec.info
        assert info["banded_ok"] and info["n_dense_rows"] == 2 and info["group_window"] == 32, (c.name, info)
        assert c.dec.forward_family(c.B, "group") == "group"
        for form in (0, 3):
            for bt in (0, 1, 2):
                c.run("group", {"forward_form": form, "backtrace_form": bt})
        with pytest.raises(_lib.ViterbiHipError):            # the lane back-trace needs a plan without dense rows
            c.run("group", {"backtrace_form": 4})
        seen.add(c.name)
    assert seen == _expected_classes(A, 10, f16), seen


# ------------------------------------------------------------------ wave form
@F16
@pytest.mark.parametrize("which", ["msnet321", "msnet321_inf", "tonet361", "tonet361_inf", "band383"])
def test_wave_form(golden, dev, which, f16):
    """wave_two 0 / 1 / 2 x wave_uniform 0-3 x wave_history 1 / 2 (a refusal where the plan has no half history), and the other
    back-trace forms behind the full history.  dead_frame0 / dead_frame1 kill songs at even and at odd frames: the half history
    rebuilds odd rows, a dead one included."""
    if which.startswith("band"):
        A, pi = _band(383, 14)
        half = 14
    else:
        A, pi = _golden(golden, which.split("_")[0], which.endswith("_inf"))
        half = HALF[which.split("_")[0]]
    seen = set()
    for c in _cases(dev, 17 + f16, A, pi, T_MID, half=half, f16=f16):
        dec = c.dec
        assert dec.info["wave_ok"], (c.name, dec.info)
        assert dec.forward_family(c.B, "wave") == "wave"
        dec.set_option("wave_history", 2)
        half_ok = dec.history_mode(c.B, c.T, "wave") == "half"
        dec.set_option("reset", 0)
        assert dec.history_mode(c.B, c.T, "wave") == "full"
        for two in (0, 1, 2):
            for uni in (0, 1, 2, 3):
                for hist in (1, 2):
                    opts = {"wave_two": two, "wave_uniform": uni, "wave_history": hist}
                    if hist == 2 and not half_ok:
                        with pytest.raises(_lib.ViterbiHipError):
                            c.run("wave", opts)
                        continue
                    c.run("wave", opts)
        for bt in (1, 2, 4):
            c.run("wave", {"backtrace_form": bt, "wave_history": 1})
        seen.add(c.name)
    assert seen == _expected_classes(A, half, f16), seen


# ------------------------------------------------------------------ 722-state floor kernels
@F16
@pytest.mark.parametrize("which", ["jdc722", "jdc722_inf", "imm722w", "imm722w_inf", "jdc721", "jdc721_inf"])
def test_floor_kernels_of_the_722_state_grids(golden, dev, which, f16):
    """W = 84 (jdc) / 128 (imm): forward_form 0 / 1 / 2 x backtrace_form 0 / 1 / 2 / 4."""
    name = which.split("_")[0]
    A, pi = _golden(golden, name, which.endswith("_inf"))
    seen = set()
    for c in _cases(dev, 19 + f16, A, pi, T_SHORT, half=HALF[name], f16=f16):
        info = c.dec.info
        assert info["banded_ok"] and info["floor_ok"] and not info["wave_ok"] and info["n_dense_rows"] == 0, (c.name, info)
        assert info["group_window"] == (128 if name == "imm722w" else 84), (c.name, info)
        assert c.dec.forward_family(c.B, "banded") == "group"
        for form in (0, 1, 2):
            for bt in (0, 1, 2, 4):
                c.run("banded", {"forward_form": form, "backtrace_form": bt})
        seen.add(c.name)
    assert seen == _expected_classes(A, HALF[name], f16), seen


# ------------------------------------------------------------------ step kernels
@F16
def test_step_kernels(golden, dev, f16):
    """The Durrieu matrix stays finite: the edges are in the emissions and the prior.  step_form 0 / 3, the plain dense kernel beside."""
    A, pi = _golden(golden, "durrieu722")
    seen = set()
    for c in _cases(dev, 23 + f16, A, pi, T_SHORT, f16=f16):
        info = c.dec.info
        assert not info["banded_ok"] and info["step_ok"], (c.name, info)
        assert c.dec.forward_family(c.B, "auto") == "dense" and c.dec.forward_family(c.B, "dense") == "dense"
        for algo, form in (("auto", 0), ("auto", 3), ("dense", 0)):
            c.run(algo, {"step_form": form})
        seen.add(c.name)
    assert seen == _expected_classes(A, None, f16), seen


# ------------------------------------------------------------------ dense kernels
@F16
@pytest.mark.parametrize("S", [33, 97, 200, 361, 369])
def test_dense_kernels(dev, S, f16):
    """Every size class of the dense kernels, both forms, on a matrix with random -inf entries, one all -inf row and one all -inf
    column; songs per workgroup 0 / 4 / 8 at S = 97."""
    rng = np.random.default_rng(S)
    A = cm.dense_with_inf(rng, S)
    pi = -(rng.integers(0, 32, S) / 4).astype(np.float32)
    assert np.isneginf(A).all(axis=1).sum() == 1 and np.isneginf(A).all(axis=0).sum() == 1
    seen = set()
    for c in _cases(dev, 29 + f16, A, pi, T_SHORT, f16=f16):
        info = c.dec.info
        assert not info["banded_ok"] and not info["step_ok"], (c.name, info)
        assert c.dec.forward_family(c.B, "auto") == "dense"
        for form in (0, 1):
            for ns in ((0, 4, 8) if S == 97 else (0,)):
                c.run("auto", {"dense_form": form, "dense_songs": ns})
        seen.add(c.name)
    assert seen == _expected_classes(A, None, f16), seen


# ------------------------------------------------------------------ the time-parallel back-trace
CHUNKINGS = ((0, -1, 0), (7, 0, 0), (32, 1, 1))              # (bt_chunks, bt_warm, bt_fast_rows)


def _chunk_deaths(T):
    """Deaths inside a chunk, on a chunk's first frame and on its last, for 7 and for 32 chunks of a full-length song (chunk c of C
    covers frames (T - 1) c / C .. (T - 1) (c + 1) / C - 1).  A dead tail is where every guess coalesces trivially; the frame before
    the death is where it must not."""
    L = T - 1
    first7, first32 = L * 2 // 7, L * 8 // 32
    td = (first7, first7 - 1, first7 + 16, first32, L * 9 // 32 - 1, 200, 1, T - 1)
    deaths = {b: t for b, t in enumerate(td)}
    lens = np.asarray([T] * 8 + [1, 2, T, T - 1], np.int64)
    return deaths, lens


@F16
@pytest.mark.parametrize("which", ["tonet361_group", "tonet361_wave", "tonet361_inf_wave", "jdc722_inf", "imm722w", "scan361", "durrieu722", "dense97"])
def test_chunked_backtrace_over_dead_songs(golden, dev, which, f16):
    T = T_LONG
    deaths, lens = _chunk_deaths(T)
    assert (T - 1) * 2 // 7 == 74 and (T - 1) * 8 // 32 == 64 and (T - 1) * 9 // 32 - 1 == 71
    rng = np.random.default_rng(31 + f16)
    if which == "scan361":
        A, pi = _band(361, 10, extras=(360,), dense_rows=(7, 100))
    elif which == "dense97":
        A = cm.dense_with_inf(rng, 97)
        pi = -(rng.integers(0, 32, 97) / 4).astype(np.float32)
    else:
        A, pi = _golden(golden, which.split("_")[0], "_inf" in which)
    S = A.shape[0]
    algo = "wave" if which.endswith("wave") else ("group" if which.endswith("group") or which == "scan361" else "auto")
    E32 = cm.dead_frame(rng, cm.EDGE_B, T, S, deaths)
    if f16:
        E32b, E16 = cm.fp16_edges(rng, cm.EDGE_B, T, S, deaths=deaths)
        inputs = [("dead_frame", E32, E32.astype(np.float16)), ("fp16_edges_dead", E32b, E16)]
    else:
        inputs = [("dead_frame", E32, None)]
    for name, e32, e16 in inputs:
        c = Case(dev, name, A, pi, e32, e16, lens, lambda s, l: cm.premise_dead(s, l, lens, deaths), False)
        info = c.dec.info
        fam = c.dec.forward_family(c.B, algo)
        assert fam == {"wave": "wave", "group": "group"}.get(algo, "group" if info["banded_ok"] else "dense"), (which, fam, info)
        full_lane = info["banded_ok"] and info["n_dense_rows"] == 0
        hists = (1, 2) if algo == "wave" else (0,)
        for hist in hists:
            for chunks, warm, fast in CHUNKINGS:
                for bt in ((0, 1, 2, 4) if info["banded_ok"] else (0,)):
                    if (bt == 4 and not full_lane) or (hist == 2 and bt != 0):
                        continue                              # (the lane form: plans without dense rows; the half history has one back-trace)
                    opts = {"bt_chunks": chunks, "bt_warm": warm, "bt_fast_rows": fast, "backtrace_form": bt}
                    if algo == "wave":
                        opts["wave_history"] = hist
                    c.run(algo, opts)
        if algo == "wave":
            c.dec.set_option("wave_history", 2)
            assert c.dec.history_mode(c.B, c.T, "wave") == "half"
            c.dec.set_option("reset", 0)


# ------------------------------------------------------------------ bounded and ragged entry points
PACK_ORDER = (9, 0, 10, 1, 7, 2, 8, 3, 4, 5, 6, 11)          # live, dead, live, dead, ...: a dead song between two live ones
K_SEG = 64


def _entry_cases(dev, golden, name, f16, inf_floor=False):
    """dead_frame0 / dead_frame1 (deaths at K - 1, K, K + 1 of the 64-frame segments among them), sparse_inf and the float16 edges."""
    A, pi = _golden(golden, name, inf_floor)
    only = {"sparse_inf", "dead_frame", "dead_prior", "fp16_edges"}
    cases = list(_cases(dev, 37 + f16, A, pi, T_MID, f16=f16, only=only))
    want = {"sparse_inf", "dead_frame0", "dead_frame1", "dead_prior", "dead_prior_all"} | ({"fp16_edges", "fp16_edges_dead"} if f16 else set())
    assert {c.name for c in cases} == want
    return cases


@F16
@pytest.mark.parametrize("name", ["tonet361", "jdc722", "durrieu722"])
def test_checkpointed_decode(golden, dev, name, f16):
    """decode_checkpointed with segments of 64 frames: songs die on a segment's last frame, on its first and on its second."""
    for c in _entry_cases(dev, golden, name, f16):
        info = c.dec.info
        assert {"tonet361": info["wave_ok"], "jdc722": info["floor_ok"] and not info["wave_ok"], "durrieu722": info["step_ok"]}[name], info
        assert c.dec.workspace_bytes_checkpointed(c.B, c.T, K_SEG) > 0
        st, ll = c.dec.decode_checkpointed(c.E, segment_frames=K_SEG, lengths=c.lens, out_dtype=torch.int32)
        c.check(st, ll, ("checkpointed", K_SEG))


@F16
@pytest.mark.parametrize("name", ["tonet361", "tonet361_inf", "msnet321"])
def test_packed_decodes_of_wave_form_plans(golden, dev, name, f16):
    for c in _entry_cases(dev, golden, name.split("_")[0], f16, name.endswith("_inf")):
        assert c.dec.info["wave_ok"]
        Ep, off = c.packed(PACK_ORDER)
        assert c.dec.workspace_bytes_packed(c.B, int(off[-1])) > 0 and c.dec.workspace_bytes_packed_checkpointed(off, K_SEG) > 0
        sp, lp = c.dec.decode_packed(Ep, off, out_dtype=torch.int32)
        c.check_packed(sp, lp, PACK_ORDER, off, "packed")
        sp, lp = c.dec.decode_packed_checkpointed(Ep, off, segment_frames=K_SEG, out_dtype=torch.int32)
        c.check_packed(sp, lp, PACK_ORDER, off, "packed checkpointed")


@F16
@pytest.mark.parametrize("name", ["jdc722", "jdc722_inf", "imm722w", "durrieu722"])
def test_packed_decodes_of_the_722_state_plans(golden, dev, name, f16):
    for c in _entry_cases(dev, golden, name.split("_")[0], f16, name.endswith("_inf")):
        assert not c.dec.info["wave_ok"] and (c.dec.info["floor_ok"] or c.dec.info["step_ok"])
        Ep, off = c.packed(PACK_ORDER)
        assert c.dec.workspace_bytes_packed(c.B, int(off[-1])) > 0 and c.dec.workspace_bytes_packed_bounded(off, K_SEG) > 0
        sp, lp = c.dec.decode_packed(Ep, off, out_dtype=torch.int32)
        c.check_packed(sp, lp, PACK_ORDER, off, "packed")
        sp, lp = c.dec.decode_packed_bounded(Ep, off, segment_frames=K_SEG, out_dtype=torch.int32)
        c.check_packed(sp, lp, PACK_ORDER, off, "packed bounded")
