"""CPU tier of the randomised parity test: the committed table of tests/random_cases.py is held to the conditions that keep
tests/test_gpu_random_parity.py from being empty or one-sided.  Nothing here touches a GPU; the library is asked size queries only,
of plans that were never uploaded.

The mutant checks run on a fixed subset (the NumPy recursions take about a second per 2 10^8 candidate sums, several minutes for
the whole table): per plan class the first MUTANT_CASES cases of the table, in table order, with at least 17 frames and
T S^2 <= MUTANT_COST, their first MUTANT_SONGS songs; and the cases of MUTANT_FOUND with as many of their songs as keep
songs T S^2 <= MUTANT_FOUND_COST.  The back-trace mutant needs two candidates one ulp apart that the emission add rounds together,
on the path: a few steps in a hundred thousand.  MUTANT_FOUND lists one case per class in which a scan of the whole table with that
mutant alone found it visible."""
import ctypes
import os
from collections import Counter, defaultdict

import numpy as np
import pytest

from tests import f64_ref
from tests import inexact
from tests import random_cases as rc
from tests import random_check as ck
from tests.common import sha

MUTANT_CASES, MUTANT_COST, MUTANT_SONGS = 4, 60_000_000, 2
MUTANT_FOUND = ((3, 106), (2, 104), (2, 29), (3, 109), (3, 14), (3, 70), (5, 92))
MUTANT_FOUND_COST = 1_100_000_000

# entry points that at least three cases of a class must be served by (with both storage types and a ragged batch among them) ...
_BANDED_ALL = ("decode", "checkpointed", "packed", "packed_bounded", "stream", "commit", "ring") + rc.F64_ENTRIES
MUST_SERVE = {
    "wave": _BANDED_ALL + ("packed_checkpointed", "logits", "logits_checkpointed"),
    "floor_wg": _BANDED_ALL,
    "floor_small": ("decode", "packed", "stream", "commit", "ring") + rc.F64_ENTRIES,
    "scan": ("decode",),
    "step": ("decode", "checkpointed", "packed", "packed_bounded", "stream"),
    "dense_small": ("decode",),
    "dense_large": ("decode",),
}
# ... and entry points that refuse at least one case of a class
MUST_REFUSE = {
    "wave": ("logits", "logits_checkpointed"),
    "floor_wg": ("packed_checkpointed", "logits", "logits_checkpointed"),
    "floor_small": ("checkpointed", "packed_checkpointed", "packed_bounded", "logits", "logits_checkpointed"),
    "scan": tuple(e for e in rc.ENTRIES if e not in ("decode",) + rc.F64_ENTRIES),
    "step": ("packed_checkpointed", "commit", "ring", "logits", "logits_checkpointed") + rc.F64_ENTRIES,
    "dense_small": rc.ENTRIES[1:],
    "dense_large": rc.ENTRIES[1:],
}
ALL_OPTIONS = tuple(rc.OPTION_VALUES) + ("backtrace_form", "wave_history")


@pytest.fixture(scope="module")
def cases():
    return [rc.case(s, i) for s, i in rc.table()]


@pytest.fixture(scope="module")
def refs(cases):
    return [ck.host_references(c) for c in cases]


@pytest.fixture(scope="module")
def lib():
    from viterbi_spl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _served_cells(cases, refs):
    """(class, entry) -> the cases an entry point serves; a ring session counts where the case has a ring size."""
    cells = defaultdict(list)
    refused = Counter()
    for c, r in zip(cases, refs):
        sv = rc.served(c)
        for e in rc.ENTRIES:
            if e in sv and not (e == "ring" and r["ring"] is None):
                cells[(c["cls"], e)].append(c)
            elif e not in sv:
                refused[(c["cls"], e)] += 1
    return cells, refused


def test_reproducible(cases):
    """case(s, i) drawn again, alone and after other cases, is the same bytes."""
    picks = [(3, 41)] + rc.table()[::23]
    first = {p: sha(*rc.case_arrays(rc.case(*p))) for p in picks}
    for p in reversed(picks):
        rc.case(1, 0)
        assert sha(*rc.case_arrays(rc.case(*p))) == first[p], p
    by_id = {(c["seed"], c["index"]): c for c in cases}
    for p in picks:
        assert sha(*rc.case_arrays(by_id[p])) == first[p], ("drawn in a run", p)


def test_served_is_what_the_size_queries_answer(cases, lib):
    """served() against the library: every size query on the host, of a plan that was never uploaded."""
    from viterbi_spl_amd import _lib
    off = np.asarray([0, 100, 300], np.int64)
    for c in cases:
        plan = ctypes.c_void_p()
        assert lib.vit_plan_create(c["A"].ctypes.data, c["pi"].ctypes.data, c["S"], ctypes.byref(plan)) == 0
        got = {"decode"}
        for mode, spw in ((0, 5), (1, 15), (2, 5)):
            obs = _lib.ObsParams(mode, c["S"] - 1, spw, 0.0, 0.0, 2.0, None)
            lg = lib.vit_workspace_bytes_logits(plan, ctypes.byref(obs), 2, 200) > 0
            lgc = lib.vit_workspace_bytes_logits_checkpointed(plan, ctypes.byref(obs), 2, 200, 64) > 0
            assert lg == ("logits" in rc.served(c)) and lgc == ("logits_checkpointed" in rc.served(c)), (rc.case_id(c), mode)
        answers = {
            "checkpointed": lib.vit_workspace_bytes_checkpointed(plan, 2, 200, 64), "packed": lib.vit_workspace_bytes_packed(plan, 2, 300),
            "packed_checkpointed": lib.vit_workspace_bytes_packed_checkpointed(plan, 2, off.ctypes.data, 64),
            "packed_bounded": lib.vit_workspace_bytes_packed_bounded(plan, 2, off.ctypes.data, 64),
            "f64": lib.vit_workspace_bytes_f64(plan, 2, 200), "f64_checkpointed": lib.vit_workspace_bytes_f64_checkpointed(plan, 2, 200, 64),
            "f64_packed": lib.vit_workspace_bytes_f64_packed(plan, 2, 300),
            "f64_packed_checkpointed": lib.vit_workspace_bytes_f64_packed_checkpointed(plan, 2, off.ctypes.data, 64),
            "f64_packed_bounded": lib.vit_workspace_bytes_f64_packed_checkpointed(plan, 2, off.ctypes.data, 64),
            "stream": lib.vit_workspace_bytes_stream(plan, 2, 200), "commit": lib.vit_workspace_bytes_stream_commit(plan, 2),
            "ring": lib.vit_workspace_bytes_stream_ring(plan, 2, 128),
        }
        lib.vit_plan_destroy(plan)
        got |= {e for e, n in answers.items() if n > 0} | {e for e in ("logits", "logits_checkpointed") if e in rc.served(c) and lg}
        assert got == rc.served(c), (rc.case_id(c), sorted(got ^ rc.served(c)))


def test_every_cell_is_covered(cases, refs):
    cells, refused = _served_cells(cases, refs)
    for cls in rc.CLASSES:
        for e in MUST_SERVE[cls]:
            assert len(cells[(cls, e)]) >= 3, (cls, e, len(cells[(cls, e)]))
        for e in MUST_REFUSE[cls]:
            assert refused[(cls, e)] >= 1, (cls, e)
    for (cls, e), got in cells.items():                      # a served cell outside MUST_SERVE holds to the same conditions
        assert len(got) >= 3, (cls, e, len(got))
        assert {c["f16"] for c in got} == {False, True}, (cls, e, "one storage type only")
        assert any((c["lens"] < c["T"]).any() for c in got), (cls, e, "no ragged batch")


def test_every_option_is_set(cases):
    """Every option takes a non-default value in at least three cases of an entry point that honours it."""
    count = Counter()
    for c in cases:
        for e, o in rc.honoured(c).items():
            for k, v in o.items():
                assert k in ALL_OPTIONS and (k in ("backtrace_form", "wave_history") or v in rc.OPTION_VALUES[k] or
                                             (k == "bt_chunks" and v in rc.LANE_CHUNKS)), (k, v)
                count[k] += 1
    for k in ALL_OPTIONS:
        assert count[k] >= 3, (k, count[k])
    units = sum(1 for c in cases if "f64_units_per_cu" in rc.honoured(c).get("f64_packed_checkpointed", {}))
    assert units >= 3, units


def test_every_kind_in_every_class(cases):
    seen = {(c["cls"], c["kind"]) for c in cases}
    missing = [(cls, k) for cls in rc.CLASSES for k in rc.KINDS if (cls, k) not in seen]
    assert not missing, missing


def test_not_one_sided(cases):
    only_decode = sum(1 for c in cases if rc.served(c) == {"decode"})
    assert 4 * only_decode <= len(cases), (only_decode, len(cases))


def mutant_subset(cases):
    """{class: the cases the mutants run on} (see the module docstring)."""
    out = defaultdict(list)
    for c in cases:
        found = (c["seed"], c["index"]) in MUTANT_FOUND
        if found:
            songs = max(1, min(c["B"], MUTANT_FOUND_COST // (c["T"] * c["S"] ** 2)))
            out[c["cls"]].append((c, songs))
        elif c["T"] >= 17 and c["T"] * c["S"] ** 2 <= MUTANT_COST and sum(1 for _, n in out[c["cls"]] if n == MUTANT_SONGS) < MUTANT_CASES:
            out[c["cls"]].append((c, MUTANT_SONGS))
    return out


def mutant_kills(c, songs=MUTANT_SONGS):
    """-> {mutant: it changes the states or the log-likelihood bits of one of the case's first songs}"""
    A, pi = c["A"], c["pi"]
    kills = Counter()
    f64_served = "f64" in rc.served(c)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(min(c["B"], songs)):
            E = c["E32"][b, :int(c["lens"][b])]
            rows = inexact.forward_reference(A, pi, E)
            path, ll = inexact.backtrace_reference(A, rows)
            mp, ml = inexact.backtrace_reference(A, inexact.forward_reassociated(A, pi, E))
            kills["forward_reassociated"] |= bool(np.any(mp != path)) or np.float32(ml).tobytes() != np.float32(ll).tobytes()
            kills["backtrace_reassociated"] |= bool(np.any(inexact.backtrace_reassociated(A, rows, E) != path))
            hp_, hl = ck.backtrace_highest(A, rows)
            kills["argmax_highest"] |= bool(np.any(hp_ != path)) or np.float32(hl).tobytes() != np.float32(ll).tobytes()
            if f64_served:
                s64, d64 = f64_ref.decode_f64(A, pi, E)
                m64, l64 = ck.decode_f64_in_float32(A, pi, E)
                kills["f64_in_float32"] |= bool(np.any(m64 != s64)) or np.float64(l64).tobytes() != np.float64(d64[s64[-1]]).tobytes()
    return kills


def test_mutants_are_visible(cases):
    """In every plan class each float32 mutant changes a case of the subset, and the float64 mutant one of every class the float64
    decodes serve: a table on which a wrong tie rule or a re-associated sum cannot be seen is not accepted."""
    sub = mutant_subset(cases)
    report = {}
    for cls in rc.CLASSES:
        total = Counter()
        for c, songs in sub[cls]:
            for m, k in mutant_kills(c, songs).items():
                total[m] += int(k)
        report[cls] = dict(total)
        for m in ("forward_reassociated", "backtrace_reassociated", "argmax_highest"):
            assert total[m] >= 1, (cls, m, "kills no case of", [rc.case_id(c) for c, _ in sub[cls]])
        if any("f64" in rc.served(c) for c in cases if c["cls"] == cls):
            assert total["f64_in_float32"] >= 1, (cls, "f64_in_float32")
    print("mutant kills per class:", report)


def test_block_premise(cases, refs):
    """Of the songs of a block with at least 17 frames and a finite log-likelihood, at least half have a path that changes state
    (from the reference alone; the GPU test asserts the same on the block it runs)."""
    by_id = {(c["seed"], c["index"]): (c, r) for c, r in zip(cases, refs)}
    for block in rc.blocks():
        n = moving = 0
        for p in block:
            c, r = by_id[p]
            a, m = ck.paths_change(r["f32"][0], r["f32"][1], c["lens"])
            n, moving = n + a, moving + m
        assert 2 * moving >= n, (block, moving, n)
