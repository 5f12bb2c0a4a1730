"""The oracle against the goldens generated from the imported reference (CPU only)."""
import numpy as np
import pytest

from oracle import viterbi_oracle as vo
from tests.common import case_emissions, case_params, sha


def test_golden_inputs_regenerate_bit_exactly(golden):
    for c in golden["manifest"]["log_cases"]:
        if c["T"] > 1000:
            continue
        logA_T, log_pi = case_params(golden, c)
        logE = case_emissions(c).numpy()
        assert sha(logA_T, log_pi, logE) == c["sha256"], c


def test_c_oracle_matches_reference_goldens(golden):
    for c in golden["manifest"]["log_cases"]:
        logA_T, log_pi = case_params(golden, c)
        logE = case_emissions(c).numpy()
        states, ll, delta = vo.decode_c(logA_T, log_pi, logE, return_delta=True)
        k = c["index"]
        assert np.array_equal(states, golden["data"][f"c{k}_states"].astype(np.int32)), c
        assert delta.tobytes() == golden["data"][f"c{k}_delta"].tobytes(), c
        assert np.float32(ll) == np.float32(c["loglik"])


def test_numpy_oracle_matches_reference_goldens(golden):
    for c in golden["manifest"]["log_cases"]:
        if c["T"] > 1000:
            continue
        logA_T, log_pi = case_params(golden, c)
        logE = case_emissions(c).numpy()
        states, ll, delta = vo.decode_numpy(logA_T, log_pi, logE, return_delta=True)
        k = c["index"]
        assert states.dtype == np.int64
        assert np.array_equal(states, golden["data"][f"c{k}_states"].astype(np.int64)), c
        assert delta.tobytes() == golden["data"][f"c{k}_delta"].tobytes()


def test_prob_domain_wrapper_matches_reference_goldens(golden):
    A, pi = golden["params"]["msnet321_A"], golden["params"]["msnet321_pi"]
    for c in golden["manifest"]["prob_cases"]:
        k = c["index"]
        got = vo.decode_probs_numpy(A, pi, golden["data"][f"p{k}_probs_st"])
        assert np.array_equal(got, golden["data"][f"p{k}_states"].astype(np.int64))


def test_batched_ragged_and_threads(golden):
    c = next(c for c in golden["manifest"]["log_cases"] if c["params"] == "tonet361" and c["kind"] == "dense" and c["T"] == 1000)
    logA_T, log_pi = case_params(golden, c)
    from viterbi_spl_amd import synth
    E = synth.emissions_dense(5, 300, 361, seed=9).numpy()
    lengths = np.array([300, 1, 2, 177, 299], np.int64)
    st, ll = vo.decode_c(logA_T, log_pi, E, lengths=lengths, threads=3)
    for b in range(5):
        s1, l1 = vo.decode_c(logA_T, log_pi, E[b, : lengths[b]])
        assert np.array_equal(st[b, : lengths[b]], s1)
        assert np.all(st[b, lengths[b]:] == -1)
        assert ll[b] == l1


def test_tie_break_is_lowest_index():
    S, T = 8, 5
    logA_T = np.zeros((S, S), np.float32)
    log_pi = np.zeros(S, np.float32)
    logE = np.zeros((T, S), np.float32)
    st, ll = vo.decode_c(logA_T, log_pi, logE)
    assert np.all(st == 0) and ll == 0.0
    st2, _ = vo.decode_numpy(logA_T, log_pi, logE)
    assert np.all(st2 == 0)


def test_minus_inf_entries():
    rng = np.random.default_rng(0)
    S, T = 33, 40
    logA_T = (-rng.integers(0, 64, (S, S)) / 8).astype(np.float32)
    logA_T[rng.random((S, S)) < 0.5] = -np.inf
    np.fill_diagonal(logA_T, 0.0)
    log_pi = np.full(S, -np.inf, np.float32)
    log_pi[3] = 0
    logE = (-rng.integers(0, 64, (T, S)) / 8).astype(np.float32)
    a, la = vo.decode_c(logA_T, log_pi, logE)
    b, lb = vo.decode_numpy(logA_T, log_pi, logE)
    assert np.array_equal(a, b) and la == lb and np.isfinite(la)


def test_observation_oracle_matches_reference_goldens():
    """Emission builders: the NumPy restatement equals the reference's own outputs."""
    import os
    from oracle import observation_oracle as oo
    from tests.common import logits_case
    og = np.load(os.path.join(os.path.dirname(__file__), "golden", "obs_goldens.npz"))
    for k in range(3):
        seed, n = og[f"shaun{k}_seed"]
        got = oo.shaun_observation_probs(logits_case(int(seed), int(n), 360))
        assert np.array_equal(np.ascontiguousarray(got.T), og[f"shaun{k}_probs"])
        seed, n = og[f"softmax{k}_seed"]
        got = oo.softmax_observation_probs(logits_case(int(seed), int(n), 361))
        assert np.array_equal(got, og[f"softmax{k}_probs"])


def test_c_oracle_matches_family_b_goldens_at_full_length():
    """The S = 361 production entry points' goldens (tests/golden/make_familyB_golden.py: the reference's own
    Viterbi.viterbi_librosa_fn / SoftMaxViterbi.viterbi_librosa_fn at T = 30000): inputs regenerate bit for bit, and the C
    restatement - fed log(p + tiny) computed as the reference does - returns the reference's states."""
    import json
    import os
    from tests.golden import make_familyB_golden as mk
    from viterbi_spl_amd import synth
    gdir = os.path.dirname(mk.__file__)
    man = json.load(open(os.path.join(gdir, "familyB_manifest.json")))
    gold = np.load(os.path.join(gdir, "familyB_goldens.npz"))
    A, pi = synth.tonet_transition(360, 14), synth.floored_prior(361)
    assert mk.sha(A, pi) == man["sha256_params"]
    P = mk.inputs(man["seed"], man["T"])
    assert mk.sha(P) == man["sha256_probs_st"]
    logA_T, log_pi = vo.log_params_from_probs(A, pi)
    logE = np.require(np.log(P.T + vo.TINY32), np.float32, ["C"])
    states, _ = vo.decode_c(logA_T, log_pi, logE)
    assert np.array_equal(states, gold["states_B"].astype(np.int32)) and np.array_equal(gold["states_B"], gold["states_C"])
    assert int(np.sum(states == 360)) == man["unvoiced_frames"]


def test_observation_oracle_matches_reference_goldens_at_the_range_edge():
    """The emission-builder restatements at the float32 range edge of exp (tests/golden/obs_range_goldens.npz: the reference's own
    builders on tests.common.range_edge_logits): spans whose e^-d is subnormal stay subnormal, bit for bit."""
    import os
    from oracle import observation_oracle as oo
    from tests.common import RANGE_SPANS, range_edge_logits
    og = np.load(os.path.join(os.path.dirname(__file__), "golden", "obs_range_goldens.npz"))
    assert tuple(og["spans"]) == RANGE_SPANS
    prior = np.load(os.path.join(os.path.dirname(__file__), "golden", "params.npz"))["msnet321_pi"]
    tiny = np.finfo(np.float32).tiny
    for name in ("shaun", "softmax", "scaled", "unscaled"):
        U, spw, *tops = (int(a) for a in og[f"{name}_args"])
        if name == "shaun":
            got = np.ascontiguousarray(oo.shaun_observation_probs(range_edge_logits(U, spw, tops), 0.32, spw=spw).T)
        elif name == "softmax":
            got = oo.softmax_observation_probs(range_edge_logits(U, spw, tops, unvoiced_column=True), spw=spw)
        else:
            got = oo.softmax_scaled_observation_probs(range_edge_logits(U, spw, tops), np.float32(0.5), prior, scaled=name == "scaled", spw=spw)
        want = og[f"{name}_probs"]
        assert got.tobytes() == want.tobytes(), name
        assert np.any((want > 0) & (want < tiny)), name                  # the subnormal band is populated
