"""Value edges on the host: -inf entries, songs that die (a whole -inf emission frame, starvation through a -inf matrix floor, a
-inf prior, float32 overflow), absorbed matrix entries, signed zeros and the float16 edge values go through the host replay of
every banded decomposition (tests/plan_replay.py: scan form, floor form, pair form, wave form, the dense image) and must give what
the oracle gives, bit for bit.  The oracle's answer for a dead song: a frame whose delta row is all -inf resolves every
back-pointer to state 0, the terminal state is 0 and the log-likelihood is -inf.

Every input's premise (tests/common.py premise_*) is asserted on the oracle's output before a replay result is looked at.  The
same builders feed tests/test_gpu_value_edges.py."""
import numpy as np
import pytest

from oracle import viterbi_oracle as vo
from tests import common as cm
from tests.plan_replay import HostPlan, replay_banded, replay_dense_image, replay_wave
from tests.test_plan_host import _banded_matrix

T_HOST = 70
GOLDEN = {"tonet361": 14, "msnet321": 12, "jdc722": 40, "imm722w": 56}        # name -> half-width of its band


def _matrix(golden, name):
    """-> (logA_T, log_pi, band half-width or None)."""
    p = golden["params"]
    if name in GOLDEN:
        return p[f"{name}_logA_T"], p[f"{name}_log_pi"], GOLDEN[name]
    if name.endswith("_inf") and name[:-4] in GOLDEN:          # log(A) without tiny: the floor log(0 + tiny) becomes log(0)
        A = cm.inf_floor_sibling(p[f"{name[:-4]}_logA_T"])
        assert np.isneginf(A).sum() > A.size // 2
        return A, p[f"{name[:-4]}_log_pi"], GOLDEN[name[:-4]]
    rng = np.random.default_rng(len(name))
    if name.startswith("band"):                                # band<S>_<half>: -inf floor, no extra column
        S, half = (int(v) for v in name[4:].split("_"))
        return _banded_matrix(S, half, rng, floor=-np.inf, quant=2), -(rng.integers(0, 8, S) / 2).astype(np.float32), half
    if name == "scan361":                                      # dense rows: the scan form and the generic back-trace
        return (_banded_matrix(361, 10, rng, extras=(360,), dense_rows=(7, 100), floor=-np.inf, quant=2),
                -(rng.integers(0, 8, 361) / 2).astype(np.float32), 10)
    assert name == "dense97"
    return cm.dense_with_inf(rng, 97), -(rng.integers(0, 32, 97) / 4).astype(np.float32), None


def _equal(got, want, by_value):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.array_equal(got, want) if by_value else got.tobytes() == want.tobytes()


def check_replays(A, pi, E, lens, ref_s, ref_l, ref_d, by_value, tag, plan=None, dense_image=False, songs=None):
    """Every replay the plan offers against the oracle's states, log-likelihoods and final delta rows.  -> the forms that ran."""
    plan = plan or HostPlan(A, pi)
    ran = set()
    for b in (range(E.shape[0]) if songs is None else songs):
        n = int(lens[b])
        e, want_s = E[b, :n], ref_s[b, :n]
        forms = []
        if plan.ok:
            forms.append(("scan", {}))
            if plan.floor_ok:
                forms.append(("floor", {"floor": True}))
            if plan.floor_ok and plan.pair_ok:
                forms.append(("pair", {"floor": True, "pair": True}))
        for form, kw in forms:
            with np.errstate(over="ignore"):
                st, ll, delta = replay_banded(plan, e, **kw)
            assert not np.isnan(delta).any(), (tag, form, b)
            assert np.array_equal(st, want_s), (tag, form, b, np.nonzero(st != want_s)[0][:8])
            assert _equal(delta, ref_d[b], by_value), (tag, form, b)
            assert _equal(ll, ref_l[b], by_value), (tag, form, b, ll, ref_l[b])
            ran.add(form)
        if plan.ok and plan.wave_ok and plan.floor_all_ok:
            with np.errstate(over="ignore"):
                hist, delta = replay_wave(plan, e)
            assert _equal(delta, ref_d[b], by_value), (tag, "wave", b)
            assert _equal(hist[-1, 0], np.max(ref_d[b]), by_value), (tag, "wave: frame maximum", b)
            ran.add("wave")
        if dense_image and b < 4:
            with np.errstate(over="ignore"):
                st, ll = replay_dense_image(plan, e)
            assert np.array_equal(st, want_s), (tag, "dense image", b)
            assert _equal(ll, ref_l[b], by_value), (tag, "dense image", b)
            ran.add("dense")
    return ran


MATRICES = ["tonet361", "tonet361_inf", "msnet321", "msnet321_inf", "jdc722", "jdc722_inf", "imm722w", "imm722w_inf",
            "band361_14", "band722_40", "scan361", "dense97"]


@pytest.mark.parametrize("name", MATRICES)
def test_value_edges_through_the_host_replays(golden, name):
    A, pi, half = _matrix(golden, name)
    S = A.shape[0]
    want_forms = {"dense97": {"dense"}, "scan361": {"scan"}}.get(name, {"scan", "floor", "pair"} | ({"wave"} if S < 384 else set()))
    classes = set()
    # the replay is a Python loop per frame: the 722-state grids replay eight of a batch's twelve songs (every dead one among them)
    songs = None if S < 400 else (0, 2, 3, 5, 6, 7, 8, 11)
    for f16 in (False, True):       # (float16 storage is a matter of the values alone here: its pass runs the float16 classes only)
        only = {"fp16_edges"} if f16 else None
        for cname, A2, pi2, E, E16, lens, premise, by_value in cm.edge_cases(S + f16, A, pi, T_HOST, half=half, f16=f16, only=only):
            ref_s, ref_l, ref_d = vo.decode_c(A2, pi2, E, lengths=lens, return_delta=True)
            premise(ref_s, ref_l)
            plan = HostPlan(A2, pi2)
            ran = check_replays(A2, pi2, E, lens, ref_s, ref_l, ref_d, by_value, (name, cname, f16), plan, dense_image=S < 100, songs=songs)
            assert ran == want_forms, (name, cname, ran)
            classes.add(cname)
    always = {"sparse_inf", "dead_frame0", "dead_frame1", "dead_prior", "dead_prior_all", "overflow_dead", "absorbing", "signed_zeros",
              "fp16_edges", "fp16_edges_dead"}
    inf_floor = bool(np.isneginf(A).any())
    assert classes == always | ({"starved"} if inf_floor else set()) | ({"single_survivor"} if inf_floor and half else set()), classes


@pytest.mark.parametrize("name", ["jdc722_inf", "imm722w_inf", "band722_40"])
def test_single_survivor_enters_window_sources_beyond_the_64th(golden, name):
    """W = 84 / 128: the lone finite source of a window sits beyond its 64th position at least ten times (what
    test_generic_backtrace_with_windows_wider_than_a_wave asserts for its own input)."""
    A, pi, half = _matrix(golden, name)
    plan = HostPlan(A, pi)
    assert plan.W in (84, 128)
    (_, A2, pi2, E, _, lens, premise, _), = cm.edge_cases(5, A, pi, 130, half=half, only={"single_survivor"})
    ref_s, ref_l = vo.decode_c(A2, pi2, E, lengths=lens)
    premise(ref_s, ref_l)
    pos = cm.window_positions(ref_s, lens, plan.lo[:plan.S])
    assert pos.min() >= 0 and pos.max() < plan.W and np.sum(pos >= 64) >= 10, (pos.min(), pos.max(), np.sum(pos >= 64))


@pytest.mark.parametrize("name", ["tonet361_inf", "msnet321_inf", "band361_14"])
def test_single_survivor_enters_both_sides_of_the_split_window(golden, name):
    """The split-window kernel joins sources 0..15 and 16..31 of a window: both 15 and 16 are entered."""
    A, pi, half = _matrix(golden, name)
    plan = HostPlan(A, pi)
    assert plan.W == 32
    (_, A2, pi2, E, _, lens, premise, _), = cm.edge_cases(5, A, pi, 130, half=half, only={"single_survivor"})
    ref_s, ref_l = vo.decode_c(A2, pi2, E, lengths=lens)
    premise(ref_s, ref_l)
    pos = cm.window_positions(ref_s, lens, plan.lo[:plan.S])
    assert {15, 16} <= set(pos.tolist()), sorted(set(pos.tolist()))


def test_dense_matrix_has_an_unreachable_target_and_a_dead_end_source():
    A = cm.dense_with_inf(np.random.default_rng(1), 97)
    assert np.isneginf(A).all(axis=1).sum() == 1 and np.isneginf(A).all(axis=0).sum() == 1
    assert 0.2 < np.isneginf(A).mean() < 0.45
