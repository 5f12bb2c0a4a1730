"""Host tier of imm's activation front-end (``vit_obs_activations``, csrc/activations.hip; ``reference_api.ImmViterbi``): the
adapter's parameters and its host ``process_HF0_fn`` against what the reference produced (tests/golden/make_imm_goldens.py), the
host-derived clamp constants, and the new entry point's declaration and argument checks.  No GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from tests.common import sha
from viterbi_spl_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "viterbi_hip.h")
VIT_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from viterbi_spl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module")
def imm():
    with open(os.path.join(HERE, "golden", "imm_manifest.json")) as fh:
        man = json.load(fh)
    return {"manifest": man, "data": np.load(os.path.join(HERE, "golden", "imm_goldens.npz"))}


def case_input(man, case):
    x = synth.hf0_activations(man["U"], case["T"], seed=case["seed"], denormal_min=case["denormal_min"]).numpy()
    assert sha(x) == case["sha256_hf0"], "synth.hf0_activations no longer regenerates the golden input"
    return x


@pytest.mark.parametrize("n_bins", [721, 720])
def test_parameters_equal_the_reference(imm, n_bins):
    """``np.log(A.T)`` without tiny, the uniform prior logged in float64 then cast: the reference's bits."""
    from viterbi_spl_amd import ImmViterbi
    man = imm["manifest"]
    v = ImmViterbi(man["bins_per_semitone"], n_bins)
    rec = man["params"][f"{man['bins_per_semitone']}_{n_bins}"]
    assert v.log_transition_matrix_T.dtype == np.float32 and v.log_transition_matrix_T.flags["C_CONTIGUOUS"]
    assert v.log_transition_matrix_T.shape == (n_bins + 1, n_bins + 1)
    assert sha(v.log_transition_matrix_T) == rec["sha256_log_transition_matrix_T"]
    assert v.log_prob_init.dtype == np.float32 and sha(v.log_prob_init) == rec["sha256_log_prob_init"]
    assert v.log_prob_init[0] == np.float32(np.log(1.0 / (n_bins + 1)))


def test_process_hf0_byte_for_byte(imm):
    """t, _min and every byte of the output, the clamp case (a subnormal smallest positive entry) and the zeros included.  The
    goldens hold what the reference returned under the NumPy named in the manifest (its clamp case is float64 under NumPy >= 2)."""
    from viterbi_spl_amd import ImmViterbi
    man = imm["manifest"]
    assert np.__version__.split(".")[0] == man["numpy"].split(".")[0], "the clamp case's dtype follows NumPy's promotion rules"
    v = ImmViterbi(man["bins_per_semitone"], man["U"])
    seen = set()
    for case in man["cases"]:
        x = case_input(man, case)
        out = v.process_HF0_fn(x)
        assert out.shape == (man["U"] + 1, case["T"]) and str(out.dtype) == case["out_dtype"]
        mp = x[x > 0].min()
        assert int(mp.view(np.uint32)) == case["min_positive_bits"]
        clamped = bool(np.log(mp) < -87)
        assert clamped == case["clamped"] == case["denormal_min"]
        t = np.exp(-87) if clamped else mp
        assert float(t).hex() == case["t_hex"]
        assert float(out[-1, 0]).hex() == case["min_hex"] and np.all(out[-1] == out[-1, 0]) and out[-1, 0] == out[:-1].min()
        assert sha(out) == case["sha256_out"], case["name"]
        assert case["zeros"] == int(np.sum(x == 0))
        seen.add((clamped, case["zeros"] > 0))
    assert (True, True) in seen and (False, True) in seen
    assert sorted(c["T"] for c in man["cases"])[:4] == [1, 2, 63, 257] and [c["T"] for c in man["cases"]].count(600) == 3


def test_golden_states_are_the_oracle_decode(imm):
    """The committed states are the float32 log-domain decode of the host front-end's output: ties the goldens to the CPU oracle."""
    from oracle import viterbi_oracle as vo
    from viterbi_spl_amd import ImmViterbi
    man = imm["manifest"]
    v = ImmViterbi(man["bins_per_semitone"], man["U"])
    for case in man["cases"]:
        out = np.asarray(v.process_HF0_fn(case_input(man, case)), np.float32)
        states, _ = vo.decode_c(v.log_transition_matrix_T, v.log_prob_init, np.ascontiguousarray(out.T)[None])
        assert np.array_equal(states[0], imm["data"][f"states_{case['name']}"]), case["name"]


def test_clamp_constants_classify_like_numpy():
    """Every float32 within 64 ulp of the threshold: ``x < clamp_below`` (a compare of bit patterns, positive floats) is
    ``np.log(x) < -87``; clamp_to is float32(exp(-87))."""
    from viterbi_spl_amd.emissions import activation_clamp_constants
    below, to = activation_clamp_constants()
    assert below.dtype == np.float32 and to.dtype == np.float32
    assert to == np.float32(np.exp(-87)) and to.view(np.uint32) == 0x00B33687
    b0 = int(below.view(np.uint32))
    bits = np.arange(b0 - 64, b0 + 65, dtype=np.uint32)
    x = bits.view(np.float32)
    assert np.array_equal(bits < b0, np.log(x) < -87)
    assert np.array_equal(bits < b0, np.asarray([np.log(v) < -87 for v in x]))         # scalar calls, as the reference makes them
    # the planted subnormal of the synthetic recordings is clamped, the ordinary smallest entries are not
    assert np.uint32(0x200).view(np.float32) < below < np.float32(2.0 ** -40)


def test_declared_and_exported(lib):
    from viterbi_spl_amd import _lib
    import viterbi_spl_amd
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bvit_obs_activations\s*\(", src), "vit_obs_activations is not declared in viterbi_hip.h"
    assert "imm/tf_imm.py:70-88" in open(HEADER).read()
    assert "vit_obs_activations" in _lib.EXPORTS and hasattr(lib, "vit_obs_activations")
    assert lib.vit_abi_version() == 4
    for name in ("ImmViterbi", "activation_log_emissions"):
        assert hasattr(viterbi_spl_amd, name)
    assert callable(synth.hf0_activations)


def test_bad_arguments_are_rejected(lib):
    """VIT_EINVAL before anything is enqueued: null pointers, ld < total_frames, n_bins out of range, a bad dtype, no recording,
    fewer frames than recordings."""
    p = ctypes.c_void_p(256 * 1024)          # never dereferenced: every call below is refused on its arguments

    def call(hf0=p, ld=100, n_bins=721, B=2, off=p, total=100, stats=p, out=p, dt=0):
        return lib.vit_obs_activations(hf0, ld, n_bins, B, off, total, 1e-38, 1.6e-38, stats, out, dt, None)

    for kw in ({"hf0": None}, {"off": None}, {"stats": None}, {"out": None}, {"ld": 99}, {"n_bins": 0}, {"n_bins": 1024},
               {"n_bins": -3}, {"dt": 2}, {"dt": -1}, {"B": 0}, {"B": 101}, {"total": 0, "ld": 0}):
        assert call(**kw) == VIT_EINVAL, kw


def test_synthetic_activations():
    """What the synthetic recordings promise: non-negative finite values, a share of exact zeros, a positive entry in every
    frame, a wide dynamic range, the same bits for the same seed -- and with denormal_min one subnormal smallest entry."""
    x = synth.hf0_activations(65, 129, seed=5).numpy()
    assert x.dtype == np.float32 and x.shape == (65, 129) and np.isfinite(x).all() and (x >= 0).all()
    assert 0.05 < np.mean(x == 0) < 0.2 and (x.max(axis=0) >= 16).all()
    assert x[x > 0].min() >= np.float32(2.0 ** -40) and x.max() / x[x > 0].min() > 1e12
    assert np.array_equal(x, synth.hf0_activations(65, 129, seed=5).numpy())
    assert not np.array_equal(x, synth.hf0_activations(65, 129, seed=6).numpy())
    d = synth.hf0_activations(65, 129, seed=5, denormal_min=True).numpy()
    tiny = np.finfo(np.float32).tiny
    assert int(np.sum((d > 0) & (d < tiny))) == 1 and int(np.sum(d != x)) == 1
    assert synth.hf0_activations(1, 3, seed=1).shape == (1, 3)
