"""Where the decodes and the builders write: every output between guards, over poisoned buffers, through the raw C ABI.

The parity tests take their outputs from ViterbiDecoder.decode: `states` and `loglik` from torch.empty (the block the previous, correct,
decode just freed) and the workspace from a cache that keeps the largest buffer ever needed.  A frame that is never written, a store one
element past an end, or a repair pass that trusts what `states` held before the call all pass there.  Here every case runs with
* the workspace an Arena (tests/guarded.py) of exactly the bytes the library's own size query returns for that call,
* `states` and `loglik` Arenas of exactly their sizes, `states` one element past a 256-byte boundary and holding wrong states,
* the emissions (logits) in an Arena one element past a 256-byte boundary, NaN patterns all around them,
twice: in the workspace filled with 0xFF over `states` = "shifted", then at once in the SAME workspace on emissions of another seed and
another T over `states` = "neighbour" (another decode's path).  The second call is told the size its own query returns; the bytes of
the arena behind that size must come out of it unchanged.  Every comparison is by bits against the CPU oracle (tests/f64_ref.py for
the float64 decodes), or against the same call's un-guarded output for the builders.  No tolerance anywhere.

Shapes: B = 4, T = 403 (odd: the half history keeps (T + 1) / 2 rows; T % 4 == 3 and 402 % 4 == 2 reach the tails of the 4-wide state
stores), lengths (403, 402, 131, 1): 131 ends inside a chunk and inside a 64-frame tile, one frame is the degenerate song.  bt_chunks 5
and bt_warm 8 are set in every case, so several chunks per song exist.  With the peak emissions of the sweep every guess has coalesced
after eight frames (a host replay of the chunk scheme finds no repair for 120 seeds), so the verify pass is put under test by
test_repair_pass_under_poison: the same chunking over synth.emissions_dense, with the premise chunks_repaired > 0 asserted through
vit_backtrace_counters for every back-trace kernel that counts (sparse, half, lane; the whole-row and the lazy kernel count nothing).

Out of reach: overruns BETWEEN the regions inside a workspace (the history is followed by 256-byte padding, the timing scratch, the
counters and the tables).  Only the first and the last byte of a workspace are fenced."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests import f64_ref
from tests import guarded as gd
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED = 0, -1, -5
B, K = 4, 64
RUNS = ((403, (403, 402, 131, 1), 41), (257, (257, 256, 131, 1), 42))      # (T, lengths, seed) of the first and the second call
SEED_NEIGHBOUR = 43
AUTO, DENSE, BANDED = _lib.ALGO["auto"], _lib.ALGO["dense"], _lib.ALGO["banded"]
FAM_STEP, FAM_GROUP, FAM_WAVE = 1, 2, 3
CHUNKING = (("bt_chunks", 5), ("bt_warm", 8))
GEN = {"peaks": synth.emissions_peaks, "dense": synth.emissions_dense}
WAVE_PLANS, GRID_PLANS, STEP_PLANS, DENSE_PLANS = ("tonet361", "msnet321"), ("jdc722", "jdc721", "imm722w"), ("durrieu722", "durrieu721"), ("dense97", "dense361")
ALL_PLANS = WAVE_PLANS + GRID_PLANS + STEP_PLANS + DENSE_PLANS
DTYPES = (False, True)                                   # fp16 storage?
DT_ID = {False: "f32", True: "f16"}

TALLY = collections.defaultdict(lambda: [0, 0])         # plan -> [cases run, cases the library refused]
SWEEP_REPAIRS = collections.Counter()                    # plan -> chunks_repaired over the whole sweep on peak emissions
REPAIRS = {}                                             # (plan, back-trace kernel) -> chunks_repaired of the two calls on dense emissions


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


class Run:
    """The inputs of one call and the oracle's answer: emissions padded and packed, each in an arena one element past a 256-byte boundary."""

    def __init__(self, A, pi, dev, kind, f16, T, lens, seed):
        S = A.shape[0]
        dt = torch.float16 if f16 else torch.float32
        item = 2 if f16 else 4
        E = GEN[kind](B, T, S, seed=seed, dtype=dt, device=dev)
        self.T, self.S, self.f16, self.dt = T, S, f16, _lib.VIT_F16 if f16 else _lib.VIT_F32
        self.lens_h = np.asarray(lens, np.int64)
        self.lens = torch.from_numpy(self.lens_h).to(dev)
        self.off = np.concatenate([[0], np.cumsum(self.lens_h)]).astype(np.int64)
        self.N = int(self.off[-1])
        self.E = gd.Arena(B * T * S * item, dev, lead=item)
        self.E.store(E)
        self.Ep = gd.Arena(self.N * S * item, dev, lead=item)
        self.Ep.store(torch.cat([E[b, :int(n)] for b, n in enumerate(lens)], dim=0).contiguous())
        self.Eh = E.float().cpu().numpy()
        self.ref_s, self.ref_l = vo.decode_c(A, pi, self.Eh, lengths=self.lens_h)
        self._ref64 = None
        self.A, self.pi = A, pi

    def ref64(self):
        if self._ref64 is None:
            s, l = f64_ref.decode_f64_batch(self.A, self.pi, self.Eh, self.lens_h)
            self._ref64 = (s.astype(np.int32), l)
        return self._ref64

    def packed(self, states):
        return np.concatenate([states[b, :int(n)] for b, n in enumerate(self.lens_h)]).astype(np.int32)


class Plan:
    def __init__(self, golden, dev, name):
        self.lib, self.name, self.dev = _lib.load(), name, dev
        self.A, self.pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
        self.dec = ViterbiDecoder(self.A, self.pi, dev)
        self.p, self.S = self.dec._plan, self.dec.S
        self._data = {}

    def data(self, f16, kind="peaks"):
        """(first call, second call, the neighbour path of the second call's songs), computed once and never modified."""
        key = (f16, kind)
        if key not in self._data:
            r1, r2 = (Run(self.A, self.pi, self.dev, kind, f16, T, lens, seed) for T, lens, seed in RUNS)
            T2, lens2, _ = RUNS[1]
            nb = GEN[kind](B, T2, self.S, seed=SEED_NEIGHBOUR, dtype=torch.float16 if f16 else torch.float32).float().numpy()
            nb_s, _ = vo.decode_c(self.A, self.pi, nb, lengths=np.asarray(lens2, np.int64))
            self._data[key] = (r1, r2, nb_s)
        return self._data[key]

    def options(self, opts):
        assert self.lib.vit_plan_set_option(self.p, b"reset", 0) == OK
        for key, value in tuple(opts):
            assert self.lib.vit_plan_set_option(self.p, key.encode(), value) == OK, (key, value)

    def family(self, algo):
        return self.lib.vit_forward_family(self.p, B, algo)

    def counters(self, ws, T):
        off, n = ctypes.c_size_t(), ctypes.c_int32()
        assert self.lib.vit_backtrace_counters(self.p, B, T, ws.ptr, ctypes.byref(off), ctypes.byref(n)) == OK
        ct = ws.payload[off.value:off.value + B * n.value * 4].view(torch.int32).view(B, n.value).sum(dim=0).cpu().tolist()
        return dict(zip(ViterbiDecoder.COUNTERS, ct))


@pytest.fixture(scope="module")
def plans(golden, dev):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Plan(golden, dev, name)
        return made[name]
    yield get
    for name in ALL_PLANS:
        if name in TALLY:
            print(f"[bounds] {name}: {TALLY[name][0]} cases ran, {TALLY[name][1]} refused; chunks repaired on peak emissions: {SWEEP_REPAIRS[name]}")
    for key, v in sorted(REPAIRS.items()):
        print(f"[bounds] chunks_repaired {key}: {v}")
    for pl in made.values():
        pl.options(())


# ----------------------------------------------------------------------------------------------------------------------------------
# one guarded pair of calls
# ----------------------------------------------------------------------------------------------------------------------------------
PACKED = ("packed", "packed_checkpointed", "packed_bounded", "f64_packed")
F64 = ("f64", "f64_checkpointed", "f64_packed")


def _need(pl, entry, r, algo):
    """The library's own size query for the call."""
    lib, p = pl.lib, pl.p
    return int({"decode": lambda: lib.vit_workspace_bytes_for(p, B, r.T, algo),
                "split": lambda: lib.vit_workspace_bytes_for(p, B, r.T, algo),
                "checkpointed": lambda: lib.vit_workspace_bytes_checkpointed(p, B, r.T, K),
                "f64": lambda: lib.vit_workspace_bytes_f64(p, B, r.T),
                "f64_checkpointed": lambda: lib.vit_workspace_bytes_f64_checkpointed(p, B, r.T, K),
                "packed": lambda: lib.vit_workspace_bytes_packed(p, B, r.N),
                "packed_checkpointed": lambda: lib.vit_workspace_bytes_packed_checkpointed(p, B, r.off.ctypes.data, K),
                "packed_bounded": lambda: lib.vit_workspace_bytes_packed_bounded(p, B, r.off.ctypes.data, K),
                "f64_packed": lambda: lib.vit_workspace_bytes_f64_packed(p, B, r.N)}[entry]())


def _call(pl, entry, r, algo, ws, ws_bytes, st, ll, poison, ref_l):
    lib, p = pl.lib, pl.p
    e, ep, ln = r.E.ptr, r.Ep.ptr, r.lens.data_ptr()
    if entry == "decode":
        return lib.vit_decode(p, e, r.dt, B, r.T, ln, ws.ptr, ws_bytes, st.ptr, ll.ptr, algo, None)
    if entry == "split":
        rc = lib.vit_forward(p, e, r.dt, B, r.T, ln, ws.ptr, ws_bytes, ll.ptr, algo, None)
        if rc != OK:
            return rc
        torch.cuda.synchronize()
        # the forward pass writes the log-likelihoods and not one byte of `states`
        assert np.array_equal(st.view(torch.int32, (B, r.T)).cpu().numpy(), poison), "vit_forward wrote into states"
        gd.assert_intact(st, "states after vit_forward")
        got = ll.view(torch.float32, (B,)).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(ref_l, np.float32).view(np.uint32)), ("loglik after vit_forward", got, ref_l)
        return lib.vit_backtrace_checked(p, e, r.dt, B, r.T, ln, ws.ptr, ws_bytes, st.ptr, algo, None)
    if entry == "checkpointed":
        return lib.vit_decode_checkpointed(p, e, r.dt, B, r.T, ln, ws.ptr, ws_bytes, st.ptr, ll.ptr, K, None)
    if entry == "f64":
        return lib.vit_decode_f64(p, e, r.dt, B, r.T, ln, ws.ptr, ws_bytes, st.ptr, ll.ptr, None)
    if entry == "f64_checkpointed":
        return lib.vit_decode_f64_checkpointed(p, e, r.dt, B, r.T, ln, ws.ptr, ws_bytes, st.ptr, ll.ptr, K, None)
    if entry == "packed":
        return lib.vit_decode_packed(p, ep, r.dt, B, r.off.ctypes.data, ws.ptr, ws_bytes, st.ptr, ll.ptr, None)
    if entry == "f64_packed":
        return lib.vit_decode_f64_packed(p, ep, r.dt, B, r.off.ctypes.data, ws.ptr, ws_bytes, st.ptr, ll.ptr, None)
    fn = {"packed_checkpointed": lib.vit_decode_packed_checkpointed, "packed_bounded": lib.vit_decode_packed_bounded}[entry]
    return fn(p, ep, r.dt, B, r.off.ctypes.data, ws.ptr, ws_bytes, st.ptr, ll.ptr, K, None)


def guarded_pair(pl, entry, f16, opts=(), algo=BANDED, family=None, kind="peaks", kinds=("shifted", "neighbour"), what=None):
    """Both calls of one case (module docstring) -> "ran" with the counters of each call, or "refused": the library answered
    VIT_EUNSUPPORTED (a size of 0 included) and wrote nothing."""
    dev = pl.dev
    r1, r2, nb_s = pl.data(f16, kind)
    packed, f64 = entry in PACKED, entry in F64
    ws, counted = None, []
    try:
        pl.options(CHUNKING + tuple(opts))
        if family is not None:
            assert pl.family(algo) == family, (pl.name, opts, "forward family", pl.family(algo), family)
        for r, poison_kind in zip((r1, r2), kinds):
            need = _need(pl, entry, r, algo)
            ref_s, ref_l = r.ref64() if f64 and need > 0 else (r.ref_s, r.ref_l)   # (a call that will be refused: any poison serves)
            poison = gd.poison_states(ref_s, pl.S, poison_kind, nb_s if poison_kind == "neighbour" else None)
            if packed:
                poison = r.packed(poison)
            st = gd.Arena(poison.size * 4, dev, lead=4)
            st.store(poison)
            ll = gd.Arena(B * (8 if f64 else 4), dev)
            if ws is None:                                                       # the first call: the arena is exactly its size
                ws = gd.Arena(need if need > 0 else int(pl.lib.vit_workspace_bytes(pl.p, B, r.T)), dev)
                kept = None
            else:                                                                # the second: what lies behind ITS size stays as it is
                assert 0 < need <= ws.nbytes, (need, ws.nbytes)
                kept = ws.payload[need:].clone()
            rc = _call(pl, entry, r, algo, ws, need if need > 0 else ws.nbytes, st, ll, poison, ref_l)
            torch.cuda.synchronize()
            if rc == EUNSUPPORTED and r is r1:
                assert np.array_equal(st.view(torch.int32, poison.shape).cpu().numpy(), poison), (pl.name, entry, opts, "a refused call wrote into states")
                assert ll.poisoned(), (pl.name, entry, opts, "a refused call wrote into loglik")
                assert ws.poisoned(), (pl.name, entry, opts, "a refused call wrote into the workspace")
                for a, n in ((st, "states"), (ll, "loglik"), (ws, "workspace")):
                    gd.assert_intact(a, n)
                TALLY[pl.name][1] += 1
                return "refused", []
            assert need > 0, (pl.name, entry, opts, "the size query says unsupported, the call returned", rc)
            assert rc == OK, (pl.name, entry, opts, poison_kind, "status", rc)
            try:
                gd.assert_decode_outputs(st, ll, ref_s, ref_l, r.lens_h, r.T, offsets=r.off if packed else None)
                gd.assert_intact(ws, "workspace")
                gd.assert_intact(r.Ep if packed else r.E, "emissions")
                if kept is not None:
                    assert torch.equal(ws.payload[need:], kept), f"the call wrote behind the {need} workspace bytes it was given"
            except AssertionError as e:
                raise AssertionError(f"{pl.name} {entry} {DT_ID[f16]} {dict(opts)} T={r.T} states={poison_kind}: {e}") from None
            if entry in ("decode", "split"):
                counted.append(pl.counters(ws, r.T))
        TALLY[pl.name][0] += 1
        if kind == "peaks":
            SWEEP_REPAIRS[pl.name] += sum(c["chunks_repaired"] for c in counted)
        elif what is not None:
            REPAIRS[(pl.name, what)] = [c["chunks_repaired"] for c in counted]
        return "ran", counted
    finally:
        pl.options(())


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. vit_decode over the kernel forms vit_plan_set_option reaches
# ----------------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("decode", "split")       # vit_decode | vit_forward, then vit_backtrace_checked: the forward pass writes loglik and not one byte of
                                     # `states`, which stay fully poisoned until the second call and are fully written after it (_call)


def _fam(ff):
    return FAM_WAVE if ff == 4 else FAM_GROUP


@pytest.mark.parametrize("ff", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("f16", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("name", WAVE_PLANS)
def test_forward_forms_by_backtrace_forms(plans, name, f16, entry, ff):
    for bt in (0, 1, 2, 4):
        guarded_pair(plans(name), entry, f16, (("forward_form", ff), ("backtrace_form", bt)), BANDED, _fam(ff))


WAVE_OPTIONS = {
    "floor_live_window": [(("forward_form", 6), ("floor_live_window", v)) for v in (0, 1)],
    "half_history": [(("forward_form", 4), ("wave_history", 2), ("bt_block_waves", v)) for v in (0, 8)],
    "wave_uniform": [(("forward_form", 4), ("wave_uniform", v)) for v in (0, 1, 2, 3)],
    "wave_two": [(("forward_form", 4), ("wave_two", v)) for v in (1, 2, 5, 6)],
    "win_shift": [(("forward_form", 1), ("win_shift", v)) for v in (0, 1, 2, 3)],
}


@pytest.mark.parametrize("group", list(WAVE_OPTIONS))
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("f16", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("name", WAVE_PLANS)
def test_wave_plan_options(plans, name, f16, entry, group):
    pl = plans(name)
    for opts in WAVE_OPTIONS[group]:
        ff = dict(opts)["forward_form"]
        outcome, _ = guarded_pair(pl, entry, f16, opts, BANDED, _fam(ff))
        if group == "half_history" and outcome == "ran":                         # premise: the half history really ran
            pl.options(opts)
            half = int(pl.lib.vit_workspace_bytes_for(pl.p, B, 403, BANDED))
            pl.options(())
            full = int(pl.lib.vit_workspace_bytes_for(pl.p, B, 403, _lib.ALGO["wave"]))
            assert 0 < 3 * half < 2 * full, (half, full)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("f16", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("name", GRID_PLANS)
def test_grid_plans(plans, name, f16, entry):
    pl = plans(name)
    for bt in (0, 2, 4):
        guarded_pair(pl, entry, f16, (("backtrace_form", bt),), BANDED, FAM_GROUP)
    for ws in (0, 1, 2, 3):
        guarded_pair(pl, entry, f16, (("win_shift", ws),), BANDED, FAM_GROUP)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("f16", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("name", STEP_PLANS)
def test_step_plans(plans, name, f16, entry):
    pl = plans(name)
    assert pl.dec.info["step_ok"] and not pl.dec.info["banded_ok"]
    for sf in (0, 3):
        guarded_pair(pl, entry, f16, (("step_form", sf),), AUTO, FAM_STEP)
    guarded_pair(pl, entry, f16, (), DENSE, FAM_STEP)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("f16", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("name", DENSE_PLANS)
def test_dense_plans(plans, name, f16, entry):
    pl = plans(name)
    assert not pl.dec.info["banded_ok"] and not pl.dec.info["step_ok"]
    for df in (0, 1):
        for ns in (0, 1, 3):
            guarded_pair(pl, entry, f16, (("dense_form", df), ("dense_songs", ns)), AUTO, FAM_STEP)
        guarded_pair(pl, entry, f16, (("dense_form", df), ("dense_one_thread", 1)), AUTO, FAM_STEP)


@pytest.mark.parametrize("name", ALL_PLANS)
def test_sentinel_on_the_default_form(plans, name):
    outcome, _ = guarded_pair(plans(name), "decode", False, (), AUTO, kinds=("sentinel",))
    assert outcome == "ran"


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. the verify-and-repair pass over poisoned states
# ----------------------------------------------------------------------------------------------------------------------------------
REPAIR_CASES = [(name, what, opts) for name in WAVE_PLANS for what, opts in (
                    ("sparse-wave", (("forward_form", 4), ("backtrace_form", 0))), ("sparse-group", (("forward_form", 1), ("backtrace_form", 0))),
                    ("lane-wave", (("forward_form", 4), ("backtrace_form", 4))), ("lane-group", (("forward_form", 1), ("backtrace_form", 4))),
                    ("half", (("forward_form", 4), ("wave_history", 2))), ("rows", (("forward_form", 4), ("backtrace_form", 2))),
                    ("lazy", (("forward_form", 4), ("backtrace_form", 1))))]
REPAIR_CASES += [(name, what, opts) for name in GRID_PLANS for what, opts in (
                    ("sparse-group", (("backtrace_form", 0),)), ("lane-group", (("backtrace_form", 4),)), ("rows", (("backtrace_form", 2),)))]
COUNTING = ("sparse-wave", "sparse-group", "lane-wave", "lane-group", "half")


@pytest.mark.parametrize("case", REPAIR_CASES, ids=[f"{c[0]}-{c[1]}" for c in REPAIR_CASES])
def test_repair_pass_under_poison(plans, case):
    """Dense i.i.d. emissions: eight warm-up frames do not coalesce every guess, so MODE 1 of the back-trace re-chases chunks -- over
    states that hold wrong states ("shifted") and another decode's path ("neighbour").  Premise, for the kernels that count: at least
    one of the two calls reports chunks_repaired > 0."""
    name, what, opts = case
    outcome, counted = guarded_pair(plans(name), "decode", False, opts, BANDED, kind="dense", what=what)
    assert outcome == "ran"
    repaired = [c["chunks_repaired"] for c in counted]
    print(f"[bounds] {name} {what}: chunks_repaired {repaired}")
    if what in COUNTING:
        assert sum(repaired) > 0, (name, what, "premise: the verify pass had nothing to repair", counted)


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. the other entry points
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16", DTYPES, ids=DT_ID.get)
def test_checkpointed_on_a_wave_plan(plans, f16):
    assert guarded_pair(plans("tonet361"), "checkpointed", f16)[0] == "ran"


@pytest.mark.parametrize("f16", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("name", ["tonet361", "jdc722", "durrieu722"])
def test_packed(plans, name, f16):
    assert guarded_pair(plans(name), "packed", f16)[0] == "ran"


@pytest.mark.parametrize("entry", ["f64", "f64_packed", "f64_checkpointed", "packed_checkpointed", "packed_bounded"])
def test_newer_entry_points_over_poisoned_outputs(plans, entry):
    """Their own tests fence the workspace; `states` and `loglik` between guards and over poison is what they lacked."""
    assert guarded_pair(plans("tonet361"), entry, False)[0] == "ran"


@pytest.mark.parametrize("name", ["dense97", "dense361", "durrieu722"])
def test_unserved_plans_are_refused_untouched(plans, name):
    """Size 0 and VIT_EUNSUPPORTED, and not one byte of the poisoned buffers changes."""
    pl = plans(name)
    for entry in (("packed", "checkpointed") if name != "durrieu722" else ()) + ("packed_checkpointed", "f64", "f64_packed", "f64_checkpointed"):
        assert guarded_pair(pl, entry, False)[0] == "refused", (name, entry)
    assert guarded_pair(pl, "decode", False, (("backtrace_form", 4),), AUTO)[0] == "refused", "the lane back-trace needs a banded plan"


def _logit_inputs(dev, mode, T, n_bins):
    cols = n_bins + 1 if mode == 1 else n_bins
    X = synth.pitch_logits(B, T, cols, seed=7 + mode + T, device=dev)
    arena = gd.Arena(B * T * cols * 4, dev, lead=4)
    arena.store(X)
    return X, arena


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_fused_logits(plans, dev, mode):
    """vit_decode_logits: states and loglik against the oracle on the un-fused builder's emissions, logE_out in an arena of its own
    against that builder's bytes inside every song and untouched past its end."""
    pl = plans("tonet361")
    lib, n_bins = pl.lib, pl.S - 1
    spw, thr, off, sc = (15 if mode == 1 else 5), (-0.75 if mode != 1 else 0.0), (1.386 if mode == 0 else 0.0), (2.0 if mode == 0 else 0.0)
    obs = _lib.ObsParams(mode, n_bins, spw, thr, off, sc, None)
    ws = None
    try:
        pl.options(CHUNKING)
        for (T, lens, _), poison_kind in zip(RUNS, ("shifted", "sentinel")):
            lens_h = np.asarray(lens, np.int64)
            lens_d = torch.from_numpy(lens_h).to(dev)
            X, Xa = _logit_inputs(dev, mode, T, n_bins)
            built = torch.empty((B, T, pl.S), dtype=torch.float32, device=dev)
            n = B * T
            rc = {0: lambda: lib.vit_obs_shaun(X.data_ptr(), n, n_bins, spw, thr, off, sc, built.data_ptr(), None),
                  1: lambda: lib.vit_obs_softmax(X.data_ptr(), n, n_bins, spw, built.data_ptr(), None),
                  2: lambda: lib.vit_obs_softmax_scaled(X.data_ptr(), n, n_bins, spw, thr, None, built.data_ptr(), None)}[mode]()
            assert rc == OK
            torch.cuda.synchronize()
            ref_s, ref_l = vo.decode_c(pl.A, pl.pi, built.cpu().numpy(), lengths=lens_h)
            poison = gd.poison_states(ref_s, pl.S, poison_kind)
            st = gd.Arena(B * T * 4, dev, lead=4)
            st.store(poison)
            ll, eo = gd.Arena(B * 4, dev), gd.Arena(B * T * pl.S * 4, dev, lead=4)
            need = int(lib.vit_workspace_bytes_logits(pl.p, ctypes.byref(obs), B, T))
            assert need > 0
            if ws is None:
                ws, kept = gd.Arena(need, dev), None
            else:
                assert need <= ws.nbytes
                kept = ws.payload[need:].clone()
            rc = lib.vit_decode_logits(pl.p, Xa.ptr, ctypes.byref(obs), B, T, lens_d.data_ptr(), ws.ptr, need, eo.ptr, st.ptr, ll.ptr, None)
            assert rc == OK
            torch.cuda.synchronize()
            gd.assert_decode_outputs(st, ll, ref_s, ref_l, lens_h, T)
            for a, what in ((ws, "workspace"), (Xa, "logits"), (eo, "logE_out")):
                gd.assert_intact(a, what)
            if kept is not None:
                assert torch.equal(ws.payload[need:], kept), "the call wrote behind the workspace bytes it was given"
            got = eo.view(torch.int32, (B, T, pl.S))
            want = built.view(torch.int32)
            for b, nb in enumerate(lens):
                assert torch.equal(got[b, :nb], want[b, :nb]), (mode, T, b, "logE_out differs from the builder's bytes")
                assert bool((got[b, nb:] == -1).all()), (mode, T, b, "logE_out was written past the song's end")
        TALLY["tonet361"][0] += 1
    finally:
        pl.options(())


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. builders and hand-off kernels: the bytes of the un-guarded call, between guards, over two different fills
# ----------------------------------------------------------------------------------------------------------------------------------
FILLS = (0xFF, 0xA5)            # the same bytes out over both: every byte of the output was written by the call


def _all_fill_elements(t, item, fill):
    """Elements of a uint8 tensor whose `item` bytes all hold the fill byte."""
    return (t.view(-1, item) == fill).all(dim=1)


def _check_output(arena, want, item, what):
    """The payload holds the un-guarded call's bytes, the arena is intact, and no element is left as the fill (beyond those whose right
    value is that very pattern)."""
    gd.assert_intact(arena, what)
    wb = want.contiguous().view(torch.uint8).view(-1)
    assert arena.nbytes == wb.numel(), (what, arena.nbytes, wb.numel())
    same = arena.payload == wb
    if not bool(same.all()):
        first = int(torch.nonzero(~same)[0, 0])
        raise AssertionError(f"{what}: differs from the un-guarded call at byte {first} (element {first // item}) of {wb.numel()}")
    left = _all_fill_elements(arena.payload, item, arena.fill) & ~_all_fill_elements(wb, item, arena.fill)
    assert not bool(left.any()), (what, "elements never written", int(left.sum()))


@pytest.mark.parametrize("n_bins", [320, 360, 721])
@pytest.mark.parametrize("n_frames", [1, 63, 257])
@pytest.mark.parametrize("builder", ["shaun", "softmax", "softmax_scaled"])
def test_emission_builders(dev, builder, n_frames, n_bins):
    lib = _lib.load()
    cols = n_bins + 1 if builder == "softmax" else n_bins
    spw = 15 if builder == "softmax" else 5
    X = synth.pitch_logits(1, n_frames, cols, seed=n_frames + n_bins, device=dev)[0].contiguous()
    prior = (torch.arange(n_bins + 1, dtype=torch.float32, device=dev) % 7 + 1) / 64

    def call(xp, op):
        if builder == "shaun":
            return lib.vit_obs_shaun(xp, n_frames, n_bins, spw, -0.75, 1.386, 2.0, op, None)
        if builder == "softmax":
            return lib.vit_obs_softmax(xp, n_frames, n_bins, spw, op, None)
        return lib.vit_obs_softmax_scaled(xp, n_frames, n_bins, spw, -0.75, prior.data_ptr(), op, None)

    want = torch.empty((n_frames, n_bins + 1), dtype=torch.float32, device=dev)
    assert call(X.data_ptr(), want.data_ptr()) == OK
    torch.cuda.synchronize()
    for fill in FILLS:
        Xa = gd.Arena(X.numel() * 4, dev, fill=fill, lead=4)
        Xa.store(X)
        out = gd.Arena(want.numel() * 4, dev, fill=fill, lead=4)
        assert call(Xa.ptr, out.ptr) == OK
        torch.cuda.synchronize()
        _check_output(out, want, 4, f"{builder} [{n_frames}, {n_bins}] fill {fill:#x}")
        gd.assert_intact(Xa, "logits")


@pytest.mark.parametrize("f16", DTYPES, ids=DT_ID.get)
def test_activations(dev, f16):
    """vit_obs_activations: three recordings of 1, 63 and 193 frames side by side, 721 bins, fp32 and fp16 rows; logE, the stats array
    and the input each in an arena of their own."""
    from viterbi_spl_amd import emissions as em
    lib = _lib.load()
    U, lens = 721, (1, 63, 193)
    N, nB = sum(lens), len(lens)
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=dev)
    H = synth.hf0_activations(U, N, seed=5, device=dev).contiguous()
    item, dt = (2, _lib.VIT_F16) if f16 else (4, _lib.VIT_F32)
    below, to = em.activation_clamp_constants()

    def call(hp, sp, op):
        return lib.vit_obs_activations(hp, N, U, nB, off.data_ptr(), N, float(below), float(to), sp, op, dt, None)

    want = torch.empty((N, U + 1), dtype=torch.float16 if f16 else torch.float32, device=dev)
    want_stats = torch.empty((nB, 4), dtype=torch.float32, device=dev)
    assert call(H.data_ptr(), want_stats.data_ptr(), want.data_ptr()) == OK
    torch.cuda.synchronize()
    for fill in FILLS:
        Ha = gd.Arena(H.numel() * 4, dev, fill=fill, lead=4)
        Ha.store(H)
        out = gd.Arena(want.numel() * item, dev, fill=fill, lead=item)
        stats = gd.Arena(nB * 16, dev, fill=fill, lead=4)
        assert call(Ha.ptr, stats.ptr, out.ptr) == OK
        torch.cuda.synchronize()
        _check_output(out, want, item, f"activations {DT_ID[f16]} fill {fill:#x}")
        _check_output(stats, want_stats, 4, f"activation stats fill {fill:#x}")
        gd.assert_intact(Ha, "hf0")


@pytest.mark.parametrize("n", [1, 255, 1027])
def test_voicing_kernels(dev, n):
    """vit_voicing_map and vit_voicing_notes: the uint8 array one byte past a 256-byte boundary, every output in its own arena, and
    each output of vit_voicing_notes left out (NULL) in turn."""
    lib = _lib.load()
    n_bins = 360
    states = ((torch.arange(n, dtype=torch.int64, device=dev) * 97) % 362 - 1).to(torch.int32)        # -1 (padding) .. 360 (unvoiced)
    notes = torch.linspace(30.0, 90.0, n_bins, device=dev)
    w_v, w_b = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    w_n, w_nv = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    assert lib.vit_voicing_notes(states.data_ptr(), n, n_bins, notes.data_ptr(), w_v.data_ptr(), w_b.data_ptr(), w_n.data_ptr(), w_nv.data_ptr(), None) == OK
    m_v, m_b = torch.empty_like(w_v), torch.empty_like(w_b)
    assert lib.vit_voicing_map(states.data_ptr(), n, n_bins, m_v.data_ptr(), m_b.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert torch.equal(m_v, w_v) and torch.equal(m_b, w_b)
    for fill in FILLS:
        sa = gd.Arena(n * 4, dev, fill=fill, lead=4)
        sa.store(states)
        v, b = gd.Arena(n, dev, fill=fill, lead=1), gd.Arena(n * 4, dev, fill=fill, lead=4)
        assert lib.vit_voicing_map(sa.ptr, n, n_bins, v.ptr, b.ptr, None) == OK
        torch.cuda.synchronize()
        _check_output(v, w_v, 1, f"voicing_map voiced n={n}")
        _check_output(b, w_b, 4, f"voicing_map bins n={n}")
        for skip in (None, 0, 1, 2, 3):
            outs = [gd.Arena(n, dev, fill=fill, lead=1)] + [gd.Arena(n * 4, dev, fill=fill, lead=4) for _ in range(3)]
            ptrs = [None if k == skip else a.ptr for k, a in enumerate(outs)]
            assert lib.vit_voicing_notes(sa.ptr, n, n_bins, notes.data_ptr(), *ptrs, None) == OK
            torch.cuda.synchronize()
            for k, (a, want, item) in enumerate(zip(outs, (w_v, w_b, w_n, w_nv), (1, 4, 4, 4))):
                if k == skip:
                    assert a.poisoned(), (n, skip, "an output that was not asked for was written")
                    gd.assert_intact(a, f"voicing_notes output {k} (NULL)")
                else:
                    _check_output(a, want, item, f"voicing_notes output {k} n={n} without {skip}")
        gd.assert_intact(sa, "states")


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. the written contract: element alignment
# ----------------------------------------------------------------------------------------------------------------------------------
def test_misaligned_workspace_is_refused(plans):
    """The one pointer with a stronger requirement than its element type: a workspace off a 256-byte boundary is VIT_EINVAL and
    nothing is written (the emissions, the logits and `states` run at element alignment in every case of this file)."""
    pl = plans("tonet361")
    r1, _, _ = pl.data(False)
    need = int(pl.lib.vit_workspace_bytes_for(pl.p, B, r1.T, BANDED))
    ws = gd.Arena(need, pl.dev, lead=16)
    poison = gd.poison_states(r1.ref_s, pl.S, "sentinel")
    st, ll = gd.Arena(B * r1.T * 4, pl.dev, lead=4), gd.Arena(B * 4, pl.dev)
    st.store(poison)
    assert pl.lib.vit_decode(pl.p, r1.E.ptr, r1.dt, B, r1.T, r1.lens.data_ptr(), ws.ptr, need, st.ptr, ll.ptr, BANDED, None) == EINVAL
    torch.cuda.synchronize()
    assert ws.poisoned() and ll.poisoned() and np.array_equal(st.view(torch.int32, (B, r1.T)).cpu().numpy(), poison)
