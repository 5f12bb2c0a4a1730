"""The seeded case table of the randomised parity tests (tests/test_random_cases_host.py, tests/test_gpu_random_parity.py,
scripts/fuzz_parity.py).  Host only: NumPy, the hash generators of viterbi_spl_amd.synth on the CPU, and tests/plan_replay.HostPlan.

case(seed, index) is a function of (seed, index) alone: its generator is ``np.random.default_rng([seed, index])``, so case (3, 41)
is the same arrays drawn alone, in a run, or after any other case.  One case = one transition matrix, one batch [B, T, S] with its
lengths and storage type, one emission kind, and for every entry point the options and arguments it is called with.

served(case) says which entry points the header promises for the case's plan, restated from csrc/kernels.hpp and csrc/capi.hip
(``*_applies``, ``ck_family``, ``pk_family``, ``pb_family``, ``st_family``, ``sc_served``) over HostPlan's fields and the predicates
tests/floor_grid.py already mirrors.  tests/test_random_cases_host.py holds it against the library's own size queries on the host.

TABLE is the committed table: (seed, N) pairs; the cases are case(seed, 0) .. case(seed, N - 1)."""
import os

import numpy as np
import torch

from tests import floor_grid as fg
from tests import inexact
from tests.common import FP16_EDGE_BITS, GEN, step_matrix
from tests.plan_replay import HostPlan
from viterbi_spl_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE = ((2, 112), (3, 112), (5, 112))
BLOCK = 4                                   # consecutive table indices per item of the GPU test

ENTRIES = ("decode", "checkpointed", "packed", "packed_checkpointed", "packed_bounded",
           "f64", "f64_checkpointed", "f64_packed", "f64_packed_checkpointed", "f64_packed_bounded",
           "logits", "logits_checkpointed", "stream", "commit", "ring")
F64_ENTRIES = ENTRIES[5:10]
CLASSES = ("wave", "floor_wg", "floor_small", "scan", "step", "dense_small", "dense_large")
KINDS = ("peaks", "dense", "ties", "scaled", "edges", "offgrid")
FAMILIES = ("band", "band_novoice", "band_edit", "dense", "logprob", "durrieu", "golden722", "structure", "step")
_FAMILY_WEIGHTS = (15, 2, 1, 2, 1, 1, 3, 2, 2)
GOLDEN_722 = ("jdc722", "jdc721", "imm722w", "durrieu722", "durrieu721")      # the reference's 722-state grids (tests/golden/params.npz)

BATCHES = (1, 2, 3, 5, 9, 17)
FRAMES = (1, 2, 3, 17, 64, 65, 129, 300, 601, 1100)
SEGMENTS = (64, 65, 100, 256, 2048)
COST_CAP = 2_000_000_000                    # B T S^2: the references of one case stay near a second
SESSION_B, SESSION_T = 2, 260               # a session takes the first recordings of the batch, cut at this many frames
LOOKBACKS = (8, 33, 100, 1 << 20)
CHUNK_SIZES = (1, 2, 3, 7, 16, 37, 64, 65, 100)

# option -> the values the header documents beside the default
OPTION_VALUES = {
    "bt_chunks": (2, 7, 32), "bt_warm": (0, 1, 16, 64), "bt_fast_rows": (1,), "bt_block_waves": (8, 4), "wave_two": (1, 2, 5, 6),
    "wave_uniform": (1, 2, 3), "win_shift": (0, 1, 2, 3), "floor_live_window": (1,), "step_form": (3,), "dense_form": (1,),
    "f64_units_per_cu": (1, 2, 3, 4),
}
LANE_CHUNKS = (1, 3, 64, 100, 256)          # "backtrace_form" 4 takes up to 256 chunks per song


_params = None


def _golden_params():
    global _params
    if _params is None:
        _params = np.load(os.path.join(ROOT, "tests", "golden", "params.npz"))
    return _params


# ---------------------------------------------------------------------------------------------------------------------
# The draws
# ---------------------------------------------------------------------------------------------------------------------
def _matrix(rng):
    """-> (family, name, logA_T, log_pi)"""
    fam = str(rng.choice(FAMILIES, p=np.asarray(_FAMILY_WEIGHTS) / sum(_FAMILY_WEIGHTS)))
    if fam == "golden722":
        name = str(rng.choice(GOLDEN_722))
        p = _golden_params()
        return fam, name, np.ascontiguousarray(p[f"{name}_logA_T"], np.float32), np.ascontiguousarray(p[f"{name}_log_pi"], np.float32)
    if fam == "durrieu":
        n = int(rng.choice([705, 721, 740, 767]))
        la = np.require(np.log(synth.durrieu_transition(n, 20)).astype(np.float32).T, np.float32, ["C"])
        lp = np.log(np.full(n + 1, 1.0 / (n + 1))).astype(np.float32)
        return fam, f"durrieu{n + 1}", la, lp
    if fam == "step":                           # tests/common.step_matrix: the Durrieu geometry (served) or another one (decode only)
        n, bw, kb = [(705, 20, 9), (768, 20, 9), (721, 20, 9), (128, 4, 15)][int(rng.integers(4))]
        la = step_matrix(n, bw, kb, rng, zero_top=bool(rng.integers(2)))
        lp = -(rng.integers(0, 8, n + 1) / 2).astype(np.float32)
        return fam, f"step{n}_{bw}_{kb}", la, lp
    if fam == "dense":
        S = int(rng.choice([rng.integers(2, 200), rng.integers(129, 257), rng.integers(257, 369), rng.integers(369, 420), rng.integers(369, 420), rng.integers(369, 420)]))
        la = synth.dense_random_log_transition(S, seed=int(rng.integers(1 << 20)))
        lp = synth.dense_random_log_transition(S, seed=int(rng.integers(1 << 20)))[0].copy()
        return fam, f"dense{S}", la, lp
    if fam == "logprob":                        # log of normalised random probabilities: no sum of the recursion is exact
        S = int(rng.choice([rng.integers(2, 200), rng.integers(369, 420)]))
        return fam, f"logprob{S}", inexact.logprob_matrix(S, rng), inexact.logprob_prior(S, rng)
    if fam == "structure":                      # tests/floor_grid.random_banded_structure, drawn from this case's generator
        from tests.test_plan_host import _banded_matrix
        S = int(rng.choice([rng.integers(70, 400), rng.integers(257, 384), 128, 256]))
        half = int(rng.integers(1, 15))
        extras = sorted(set(int(x) for x in rng.integers(0, S, int(rng.integers(0, 3)))))
        dense_rows = sorted(set(int(x) for x in rng.integers(0, S, int(rng.choice([0, 0, 1, 2])))))
        floor = [-50.0, -3.0, -np.inf][int(rng.integers(3))]
        la = _banded_matrix(S, half, rng, extras, dense_rows, floor=floor, quant=2)
        lp = -(rng.integers(0, 8, S) / 2).astype(np.float32)
        return fam, f"structure{S}_h{half}_x{len(extras)}_r{len(dense_rows)}_f{floor}", la, lp
    n = int(rng.choice([rng.integers(100, 300), rng.integers(300, 383), 320, 360, 320, 360, rng.integers(400, 760), 720, 721]))
    if fam == "band_novoice":                   # (no extra column: S = n; S = 64 k leaves the floor kernel no idle slot -- scan form only)
        n = int(rng.choice([rng.integers(100, 300), 128, 256, 320, 384, 512]))
    dmax = int(rng.integers(1, 8)) if n < 100 else int(rng.choice([rng.integers(2, 15), 12, 14, 14, rng.integers(15, 60)]))
    dmax = min(dmax, n // 3)
    A = synth.tonet_transition(n, dmax)
    pi = synth.floored_prior(n + 1)
    if fam == "band_novoice":                   # voiced block only: no extra column
        A = A[:n, :n] / A[:n, :n].sum(axis=1, keepdims=True)
        pi = pi[:n] / pi[:n].sum()
    la, lp = synth.log_params(A, pi)
    if fam == "band_edit" and la.shape[0] > 64:   # a few far entries in a few rows: dense-row outliers or wider windows
        for _ in range(int(rng.integers(1, 4))):
            j, i = int(rng.integers(la.shape[0])), int(rng.integers(la.shape[0]))
            la[j, i] = np.float32(-1.0 - rng.integers(0, 2000) / 256.0)
    return fam, f"{fam}{la.shape[0]}_d{dmax}", la, lp


def _edges(rng, B, T, S, f16):
    """Emission kind "edges": a coarse grid sprinkled with -inf (float16 storage: with the float16 edge values), and with
    probability 1/4 one song killed by a whole -inf frame at a random position."""
    e = (-(rng.integers(0, 96, (B, T, S)) / 8)).astype(np.float16)
    if f16:
        u = e.view(np.uint16).copy()
        pick = rng.random((B, T, S)) < 0.3
        u[pick] = np.asarray(FP16_EDGE_BITS, np.uint16)[rng.integers(0, len(FP16_EDGE_BITS), int(pick.sum()))]
        e = u.view(np.float16)
    else:
        e = e.astype(np.float32)
        e[rng.random((B, T, S)) < 0.2] = -np.inf
    if rng.random() < 0.25:
        e[int(rng.integers(B)), int(rng.integers(T)), :] = -np.inf
    return np.ascontiguousarray(e)


def _emissions(rng, kind, B, T, S, f16):
    """-> (float32 values as the oracle sees them, the float16 array that is stored or None)"""
    if kind == "edges":
        e = _edges(rng, B, T, S, f16)
        return (e.astype(np.float32), e) if f16 else (e, None)
    if kind == "offgrid":
        # few levels: the running sums of neighbouring states differ by the offsets alone, so candidates tie within an ulp
        # and a common depth per frame: the path on paper is the same, the sums grow and with them the ulp they round to
        base = -(rng.integers(0, int(rng.choice([8, 24])), (B, T, S)) / 2).astype(np.float32) - np.float32(rng.choice([0.0, 8.0, 40.0]))
        return inexact.stored(inexact.off_grid_emissions(base, rng), f16)
    e = GEN[kind](B, T, S, seed=int(rng.integers(1 << 20)), dtype=torch.float16 if f16 else torch.float32).numpy()
    return (e.astype(np.float32), e) if f16 else (e, None)


def _pick(rng, key, p=0.5):
    """A documented non-default value of option `key` with probability p, else None (the default)."""
    vals = OPTION_VALUES[key]
    v = vals[int(rng.integers(len(vals)))]
    return int(v) if rng.random() < p else None


def _opts(rng, keys, p=0.5):
    out = {}
    for k in keys:
        v = _pick(rng, k, p)
        if v is not None:
            out[k] = v
    return out


def _schedule(rng, lens):
    """An append schedule over recordings of `lens` frames: [(n, counts)], every recording takes a frame of the first append, later
    ones may sit an append out or take fewer rows than it holds; no append is empty for everybody."""
    lens = np.asarray(lens, np.int64)
    pos = np.zeros_like(lens)
    out = []
    while (pos < lens).any():
        n = int(rng.choice(CHUNK_SIZES))
        left = lens - pos
        cnt = np.minimum(n, left)
        if out:
            u = rng.random(len(lens))
            cnt = np.where(u < 0.15, 0, np.where(u < 0.3, rng.integers(0, n + 1, len(lens)), n))
            cnt = np.minimum(cnt, left)
            if cnt.max() == 0:
                cnt = np.minimum(n, left)
        out.append((n, cnt.astype(np.int64)))
        pos = pos + cnt
        if len(out) >= 8:                      # the rest in one append each of 100 rows
            while (pos < lens).any():
                cnt = np.minimum(100, lens - pos)
                out.append((100, cnt.astype(np.int64)))
                pos = pos + cnt
    return out


def plan_class(hp):
    """One of CLASSES, read from the host plan."""
    if hp.ok:
        if hp.wave_ok:
            return "wave"
        if hp.n_dense == 0 and fg.floor_packed_applies(hp.S, hp.W, hp.floor_ok, hp.n_dense):
            return "floor_wg" if hp.S >= 384 else "floor_small"
        return "scan"
    if hp.step_ok:
        return "step"
    return "dense_small" if hp.S <= 368 else "dense_large"


def fused_mode_ok(hp):
    """The plan side of kernels.hpp fused_logits_applies: six states per lane, half-width 14, one extra column, the last state."""
    return bool(hp.ok and hp.wave_ok and hp.wave_npl == 6 and hp.wave_dk == 14 and hp.n_extras == 1 and hp.extras == [hp.S - 1] and
                hp.S in (321, 361))


def case(seed, index):
    """Everything case (seed, index) is: see the module docstring."""
    rng = np.random.default_rng([int(seed), int(index)])
    family, name, A, pi = _matrix(rng)
    S = A.shape[0]
    hp = HostPlan(A, pi)
    B = int(rng.choice(BATCHES))
    T = int(rng.choice(FRAMES))
    while B * T * S * S > COST_CAP:             # the longest shape under the cap: first fewer frames, then fewer songs
        if T > 64:
            T = max(t for t in FRAMES if t < T)
        else:
            B = max(b for b in BATCHES if b < B)
    kinds = KINDS if S >= 8 else ("dense", "ties", "edges", "offgrid")
    kind = str(rng.choice(kinds))
    f16 = bool(rng.integers(2))
    E32, E16 = _emissions(rng, kind, B, T, S, f16)
    lens = np.where(rng.random(B) < 0.5, T, rng.integers(1, T + 1, B)).astype(np.int64)
    if rng.random() < 0.2:
        lens[:] = T
    c = dict(seed=int(seed), index=int(index), family=family, name=name, A=A, pi=pi, hp=hp, S=S, B=B, T=T, lens=lens, f16=f16, kind=kind,
             E32=E32, E16=E16, cls=plan_class(hp))

    # decode: the forms the plan allows, each with its own options
    forms = [("auto", 0)]
    if hp.ok:
        forms += [("group", 0), ("group", 2)]
        if hp.n_dense == 0:
            forms += [("group", 4)]
        if hp.wave_ok:
            forms += [("wave", 0), ("wave", 2), ("wave", 4), ("wave-half", 0)]
    if S <= 400 or rng.random() < 0.3:
        forms += [("dense", 0)]
    wave = bool(hp.ok and hp.wave_ok)
    form_keys = {"auto": ("bt_fast_rows",) if hp.ok else (("step_form",) if hp.step_ok else ()),
                 "group": ("bt_fast_rows", "win_shift") + (("floor_live_window",) if hp.floor_ok else ()),
                 "wave": ("bt_fast_rows", "wave_two", "wave_uniform"), "wave-half": ("bt_fast_rows", "wave_uniform", "bt_block_waves"),
                 "dense": ("dense_form",)}
    decode_forms = []
    for algo, btf in forms:
        o = _opts(rng, form_keys[algo], 0.4)
        if btf:
            o["backtrace_form"] = btf
        if algo != "dense" and (hp.ok or algo != "auto") and rng.random() < 0.5:
            o["bt_chunks"] = int(rng.choice(LANE_CHUNKS)) if btf == 4 else int(rng.choice(OPTION_VALUES["bt_chunks"]))
            o["bt_warm"] = int(rng.choice(OPTION_VALUES["bt_warm"]))
        decode_forms.append((algo, o))
    c["decode_forms"] = decode_forms
    c["K"] = {e: int(rng.choice(SEGMENTS)) for e in ENTRIES}
    c["options"] = {
        "checkpointed": _opts(rng, ("bt_fast_rows", "wave_two") if wave else ("bt_fast_rows", "bt_warm", "win_shift")),
        "packed": _opts(rng, () if wave else ("bt_warm", "win_shift")),
        "packed_checkpointed": _opts(rng, ("wave_uniform", "wave_two", "bt_fast_rows")),
        "packed_bounded": _opts(rng, ("wave_uniform", "wave_two", "bt_fast_rows") if wave else ("bt_fast_rows", "bt_warm", "win_shift")),
        "f64": _opts(rng, ("bt_chunks", "bt_warm")),
        "f64_checkpointed": _opts(rng, ("bt_chunks", "bt_warm")),
        "f64_packed": _opts(rng, ("bt_warm",)),
        "f64_packed_checkpointed": _opts(rng, ("bt_chunks", "bt_warm", "f64_units_per_cu")),
        "f64_packed_bounded": _opts(rng, ("bt_chunks", "bt_warm", "f64_units_per_cu")),
        "logits": _opts(rng, ("bt_chunks", "bt_warm", "bt_fast_rows", "bt_block_waves")),
        "logits_checkpointed": _opts(rng, ("bt_fast_rows",)),
        "stream": _opts(rng, ("bt_chunks", "bt_warm", "bt_fast_rows", "win_shift")),
        "commit": _opts(rng, ("win_shift",)),
        "ring": _opts(rng, ("win_shift",)),
    }
    # the fused decodes take "wave_uniform" 2 / 3 on the 361-state grid and 3 on the 321-state one ("wave_uniform" 1 is refused)
    if rng.random() < 0.4:
        u = int(rng.choice((2, 3) if S == 361 else (3,)))
        c["options"]["logits"]["wave_uniform"] = u
        c["options"]["logits_checkpointed"]["wave_uniform"] = u
    if rng.random() < 0.3:
        c["options"]["logits"]["backtrace_form"] = int(rng.choice((2, 4)))
    if rng.random() < 0.3:
        c["options"]["stream"]["backtrace_form"] = 4
    # max_workspace_bytes: a rung (the segment length whose size the budget is placed at) and the side of it
    c["budget"] = {e: (int(rng.choice((64, 128, 256, 1024))), bool(rng.integers(2))) for e in ("decode", "packed", "f64", "logits")}
    # the fused decodes: builder geometry and logits
    c["obs_mode"] = int(rng.integers(3))
    c["logits_seed"] = int(rng.integers(1 << 20))
    # sessions
    Bs = min(B, SESSION_B)
    slens = np.minimum(lens[:Bs], SESSION_T)
    c["session"] = dict(B=Bs, lens=slens, schedule=_schedule(rng, slens), schedule_commit=_schedule(rng, slens),
                        cadence=int(rng.integers(1, 4)), lookback=int(rng.choice(LOOKBACKS)), lookback_ring=int(rng.choice(LOOKBACKS[2:])),
                        cap_extra=int(rng.integers(0, 9)))
    return c


def case_arrays(c):
    """Every array of a case, in a fixed order (for common.sha)."""
    out = [c["A"], c["pi"], c["E32"], c["lens"], np.asarray([c["B"], c["T"], c["S"], int(c["f16"])], np.int64)]
    if c["E16"] is not None:
        out.append(c["E16"].view(np.uint16))
    for key in ("schedule", "schedule_commit"):
        for n, cnt in c["session"][key]:
            out += [np.asarray([n], np.int64), cnt]
    scal = [c["K"][e] for e in ENTRIES] + [c["obs_mode"], c["logits_seed"], c["session"]["cadence"], c["session"]["lookback"],
                                           c["session"]["lookback_ring"], c["session"]["cap_extra"]]
    for e in sorted(c["budget"]):
        scal += [c["budget"][e][0], int(c["budget"][e][1])]
    text = repr((c["family"], c["name"], c["kind"], c["decode_forms"], sorted((e, sorted(o.items())) for e, o in c["options"].items())))
    return out + [np.asarray(scal, np.int64), np.frombuffer(text.encode(), np.uint8)]


def case_id(c):
    return f"({c['seed']}, {c['index']}) {c['name']} {c['cls']} B{c['B']} T{c['T']} {c['kind']} {'f16' if c['f16'] else 'f32'}"


def table():
    """[(seed, index)] of the committed table, in order."""
    return [(s, i) for s, n in TABLE for i in range(n)]


def blocks():
    t = table()
    return [t[k:k + BLOCK] for k in range(0, len(t), BLOCK)]


# ---------------------------------------------------------------------------------------------------------------------
# Which entry points serve a plan
# ---------------------------------------------------------------------------------------------------------------------
def _sparse_applies(S, W, SD, n_dense):
    """backtrace_sparse.hip sparse_backtrace_applies over history rows of SD floats with a frame maximum."""
    kc = (W + 4 + 1 + 63) // 64
    span = {1: 64, 2: 128}.get(kc, 160)
    return n_dense == 0 and kc <= 3 and W + 32 <= span and SD >= span and SD % 4 == 0 and (S + 63) // 64 <= 12


def served_plan(hp):
    """{entry: bool} for a host plan (the fused entries: for a builder geometry of the reference)."""
    S, W = hp.S, hp.W
    nd = hp.n_dense if hp.ok else 0
    width_ok = W in fg.WIDTHS
    lane = nd == 0 and width_ok and W <= S                                                 # capi.hip ck_lane_applies
    sparse_g = _sparse_applies(S, W, (S + 5) // 4 * 4, nd)                                # ck_sparse_applies(kFamGroup)
    sparse_w = hp.wave_ok and _sparse_applies(S, W, 64 * hp.wave_npl, nd)                 # ck_sparse_applies(kFamWave)
    step = bool(hp.step_ok and hp.step_bw == 20 and hp.step_kb == 9 and 704 < S - 1 <= 768)   # capi.hip step_applies
    wave = bool(hp.ok and hp.wave_ok)
    packed_wg = bool(hp.ok) and fg.floor_packed_applies(S, W, hp.floor_ok, nd)
    ckpt_wg = packed_wg and fg.floor_ckpt_pair(W, fg.waves_for(S))
    if wave:
        ck, pk, pc, pb = sparse_w, True, sparse_w, sparse_w
    elif hp.ok:
        ck, pk, pc, pb = ckpt_wg and (sparse_g or lane), packed_wg and W <= S, False, ckpt_wg and W <= S and sparse_g
    else:
        ck, pk, pc, pb = step, step, False, step
    f64 = bool(hp.ok and hp.floor_ok and nd == 0 and width_ok and W <= S and fg.waves_for(S) > 0)
    st = (packed_wg and (sparse_g or lane)) if hp.ok else step                            # capi.hip st_family
    sc = bool(hp.ok) and st and lane                                                       # capi.hip sc_served
    lg = fused_mode_ok(hp)
    out = {"decode": True, "checkpointed": ck, "packed": pk, "packed_checkpointed": pc, "packed_bounded": pb,
           "logits": lg, "logits_checkpointed": lg and ck, "stream": st, "commit": sc, "ring": sc}
    out.update({e: f64 for e in F64_ENTRIES})
    return {e: bool(out[e]) for e in ENTRIES}


def served(c):
    """The set of entry points the header says serve this case's plan."""
    return {e for e, ok in served_plan(c["hp"]).items() if ok}


def group_ok(hp):
    """capi.hip resolve_family: the banded workgroup family (algo "group") exists for the plan."""
    nwt = fg.waves_for(hp.S)
    scan = nwt > 0 and ((hp.W <= 32 and nwt <= 12) or (hp.W == 64 and nwt <= 6))
    return bool(hp.ok and (scan or (hp.floor_ok and hp.S < nwt * 64 and fg.floor_form_instantiated(hp.W, nwt))))


def honoured(c):
    """{entry: the options the case sets for an entry point that serves it}.  case() draws for every call only options the header
    lists as honoured for the plan's kind, so this is what the coverage condition of the host tier counts; decode: the union over
    its forms ("wave_history" 2 is the half-history form)."""
    sv = served(c)
    out = {e: dict(c["options"][e]) for e in ENTRIES if e in c["options"] and e in sv}
    d = {}
    for algo, o in c["decode_forms"]:
        d.update(o)
        if algo == "wave-half":
            d["wave_history"] = 2
    out["decode"] = d
    return out
