"""CPU tier of the inexact-sum tests: the reason tests/test_gpu_inexact.py can fail.

The decoder promises the reference's bits, and its kernels keep float32 delta rows only: the back-traces and the half history's
rebuilt frames recompute "the same fl32 sums, lowest index attaining the max".  That depends on the association
fl(fl(d + A) + E) -- but only where a sum rounds.  On the dyadic grids of the geometry tests none does: a forward pass computed
as d + fl(A + E) and a back-trace that compares after the emission add return the same bits there
(test_mutants_are_invisible_on_the_dyadic_original asserts exactly that, next to the twin on which both show).

For every case of tests/inexact_cases.py (the per-case figures are in that module's docstring; by family, the share of candidate
sums that round: wave 0.53 - 0.94, path 0.63 - 0.81, banded 0.53 - 0.81, sparse 0.54 - 0.77, dense 0.91 - 1.00 (S = 1: 0, by construction), wide 0.51, step
0.64 - 0.90):

  * the premises, on the reference recursion alone (tests/inexact.py): at least half of the candidate sums round, the forward
    mutant changes a state or a log-likelihood bit, and per structure the back-trace mutant changes a state in some case;
  * the NumPy restatement the premises are measured on equals oracle.viterbi_oracle.decode_c bit for bit;
  * the plan analysis classifies the twin like the dyadic original (tests/plan_replay.HostPlan);
  * the host replays of the kernels' arithmetic (replay_banded, its floor and pair forms, replay_wave, replay_step,
    replay_dense_image) give decode_c's delta row, states and log-likelihood bit for bit."""
import numpy as np
import pytest

from oracle import viterbi_oracle as vo
from tests import inexact as ix
from tests import inexact_cases as ic
from tests.plan_replay import HostPlan, replay_banded, replay_dense_image, replay_step, replay_wave

PLAN_FIELDS = ("ok", "S", "SP", "W", "max_window", "extras", "dense_rows", "pair_ok", "floor_ok", "floor_all_ok", "wave_ok", "wave_npl",
               "wave_d", "wave_dk", "step_ok", "step_bw", "step_kb")


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _replayed_songs(c):
    """The full-length song and, where the batch has one, the mid-length song."""
    return (0, 2) if c.B >= 3 else (0,)


@pytest.mark.parametrize("cid", ic.IDS)
def test_premises(cid):
    """At least half of the candidate sums of the reference recursion round and the forward mutant is visible -- except with one
    state, where the only log-probability is log(1) = 0 and every sum is exact."""
    c = ic.case(cid)
    rounds, visible, changed = ic.premises(cid)
    print(f"{cid}: {rounds:.3f} of the candidate sums round, forward mutant visible: {visible}, back-trace mutant: {changed} states")
    if c.S == 1:
        assert rounds == 0.0 and not visible and changed == 0
        return
    assert rounds >= 0.5, (cid, rounds)
    assert visible, (cid, "d + fl(A + E) decodes the same states and log-likelihood bits: pick another seed (inexact_cases.RESEED)")
    assert len(np.unique(c.lens)) >= min(c.B, 3) and c.lens.max() == c.T and (c.B < 2 or c.lens.min() == 1)


def test_backtrace_mutant_shows_in_every_structure():
    """Per family and structure, at least one case on which an arg-max taken after the emission add changes a state."""
    seen = {}
    for cid in ic.IDS:
        c = ic.case(cid)
        seen.setdefault((c.family, c.structure), []).append(ic.premises(cid)[2])
    assert len(seen) == 3 + 5 + 3 + 1 + 1 + 1 + 1
    missing = [k for k, v in seen.items() if not any(n > 0 for n in v)]
    assert not missing, (missing, "pick another seed (inexact_cases.RESEED)")


@pytest.mark.parametrize("cid", ("path0", "wave4", "banded1"))
def test_mutants_are_invisible_on_the_dyadic_original(cid):
    """The dyadic original next to its twin: on the original no candidate sum rounds, the reassociated forward pass returns the
    same states and log-likelihood bits and the reassociated back-trace the same path -- the geometry tests cannot tell the mutants
    from the kernels.  On the twin they can."""
    c = ic.case(cid)
    assert ix.premise_rounds(c.A0, c.pi0, c.E0, c.lens) == 0.0
    visible, changed, _ = ix.premise_mutants(c.A0, c.pi0, c.E0, c.lens)
    assert not visible and changed == 0
    rounds, visible, _ = ic.premises(cid)
    assert rounds >= 0.5 and visible
    structure = [ic.premises(k)[2] for k in ic.IDS if (ic.case(k).family, ic.case(k).structure) == (c.family, c.structure)]
    assert any(n > 0 for n in structure)


@pytest.mark.parametrize("cid", ic.IDS)
def test_restatement_equals_the_oracle(cid):
    """tests/inexact.py forward_reference + backtrace_reference, which the premises are measured on, against decode_c."""
    c = ic.case(cid)
    ref_s, ref_l, ref_d = ic.oracle(cid)
    _, _, (st, ll) = ix.premise_mutants(c.A, c.pi, c.E[:4], c.lens[:4])
    for b, s in enumerate(st):
        assert np.array_equal(s, ref_s[b, :c.lens[b]]), (cid, b)
    assert np.array_equal(_bits(ll), _bits(ref_l[:4])), cid
    n = int(c.lens[0])
    assert np.array_equal(_bits(ix.forward_reference(c.A, c.pi, c.E[0, :n])[-1]), _bits(ref_d[0])), cid


@pytest.mark.parametrize("cid", [k for k in ic.IDS if ic.FAMILY[k] != "dense"])
def test_plan_classifies_the_twin_like_the_original(cid):
    """off_grid keeps every equality and the order of the values: the same flags, windows, extra columns, dense rows and step
    bands, row by row."""
    c = ic.case(cid)
    twin, orig = HostPlan(c.A, c.pi), HostPlan(c.A0, c.pi0)
    for f in PLAN_FIELDS:
        assert getattr(twin, f) == getattr(orig, f), (cid, f, getattr(twin, f), getattr(orig, f))
    assert np.array_equal(twin.lo, orig.lo) and np.array_equal(twin.kind, orig.kind) and np.array_equal(twin.lo2, orig.lo2), cid
    assert twin.ok == (c.family != "step") and twin.step_ok == (c.family == "step"), (cid, twin.ok, twin.step_ok)
    if c.family == "step":
        assert (twin.step_bw, twin.step_kb) == (c.bw, c.kb)
    if c.family == "wave":
        assert twin.wave_ok == (c.S + len(c.extras) < 384) and twin.extras == c.extras, (cid, twin.wave_ok, twin.extras)
    if c.family == "path":
        assert (twin.floor_ok, twin.n_dense > 0) == {"floor+lean_affine": (True, False), "floor+lean_table": (True, False),
                                                     "scan+lean": (False, False), "scan+generic": (False, True),
                                                     "scan(full waves)+lean": (True, False)}[c.name], (cid, twin.floor_ok, twin.n_dense)


@pytest.mark.parametrize("cid", ic.IDS)
def test_host_replay_is_bit_exact(cid):
    """The kernels' arithmetic, replayed on the host from the plan image, on inputs whose sums round."""
    c = ic.case(cid)
    ref_s, ref_l, ref_d = ic.oracle(cid)
    plan = HostPlan(c.A, c.pi)
    ran = set()
    for b in _replayed_songs(c):
        n = int(c.lens[b])
        E, want_s, want_l, want_d = c.E[b, :n], ref_s[b, :n], ref_l[b], ref_d[b]

        def same(st, ll, delta, what):
            ran.add(what)
            assert np.array_equal(st, want_s), (cid, b, what, "states")
            assert np.array_equal(_bits(delta), _bits(want_d)), (cid, b, what, "delta")
            assert _bits(ll) == _bits(want_l), (cid, b, what, "log-likelihood")

        if plan.ok:
            same(*replay_banded(plan, E), "scan")
            if plan.floor_ok:
                same(*replay_banded(plan, E, floor=True), "floor")
                if plan.pair_ok:
                    same(*replay_banded(plan, E, floor=True, pair=True), "pair")
            if plan.wave_ok:
                _, delta = replay_wave(plan, E)
                ran.add("wave")
                assert np.array_equal(_bits(delta), _bits(want_d)), (cid, b, "wave", "delta")
        elif plan.step_ok:
            st, ll, rows = replay_step(plan, E)
            same(st, ll, rows[-1], "step")
        # the packed matrix the dense kernels read, for every plan
        A_img = plan.A4[:, :c.S, :].transpose(1, 0, 2).reshape(c.S, -1)[:, :c.S]
        assert np.array_equal(_bits(A_img), _bits(c.A)), cid
        if c.S <= 400 or not plan.step_ok:
            st, ll = replay_dense_image(plan, E)
            same(st, ll, vo.decode_numpy(A_img, plan.log_pi[:c.S], E, return_delta=True)[2], "dense")
    want = {"wave": {"scan", "floor", "wave", "dense"}, "dense": {"dense"}, "step": {"step"}, "wide": {"scan", "floor", "dense"}}.get(c.family)
    if want is not None and not (c.family == "wave" and not plan.wave_ok):
        assert want <= ran, (cid, ran)
