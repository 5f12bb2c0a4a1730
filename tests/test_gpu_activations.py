"""GPU tests of imm's activation front-end (``vit_obs_activations``, csrc/activations.hip) and of ``reference_api.ImmViterbi``.

Shapes: U = 721 (the reference's grid) and U in {1, 5, 64, 65} (one bin, fewer bins than a store group, one tile exactly, one tile
and one bin); recordings of 1, 2, 63, 64, 65, 129 and 600 frames in ONE packed call -- every 64-frame tile but the last ones of the
long recording straddles a boundary -- and the same recordings alone; the activations are a column slice of a wider buffer
(row stride > frames, a base that is not 16-byte aligned), whose other columns hold values smaller than any inside.

The recordings are crafted so that a tile that attributes one column to the neighbouring recording changes a statistic: each
recording's unique smallest positive value sits in its last (variant 0) or first (variant 1) column, and the column next to it
across the boundary holds a value that is smaller than it but larger than that neighbour's own minimum.  Variant 0 has no zeros
(the overall minimum is that same value) and ends with a recording whose minimum is subnormal (the clamp); in variant 1 the
even recordings hold exactly one zero, in a boundary column."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests.common import sha
from viterbi_spl_amd import ImmViterbi, _lib, synth
from viterbi_spl_amd.emissions import activation_log_emissions

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = (1, 2, 63, 64, 65, 129, 600)
SHAPES = [(721, 0), (721, 1), (1, 0), (1, 1), (5, 0), (5, 1), (64, 0), (64, 1), (65, 0), (65, 1)]
# Largest distance, in float32 ulp, between the device's log(hf0 + t) and NumPy's float32 log over every input of this file,
# measured on the MI355X (the test prints it): 4 ulp over 3 114 694 values (1 ulp where HF0 == 0; NumPy 2.2.6, ROCm's logf).
# Both are a few ulp from the true value, so the bound is not derived: the assert allows twice the measured maximum, because
# the inputs sample the range thinly.
MEASURED_MAX_ULP = 4
ULP_BOUND = 2 * MEASURED_MAX_ULP


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def f32(e):
    return np.float32(2.0) ** np.float32(e)


def crafted(U, variant):
    """Host activations of the seven recordings, [U, T_b] float32 each."""
    recs = []
    ua, ub = 0, U - 1
    for b, T in enumerate(LENGTHS):
        x = synth.hf0_activations(U, T, seed=300 + 10 * variant + b).numpy().copy()
        x[x == 0] = f32(-20)
        if variant == 0:           # decreasing chain: m_b in the last column, s_b in the first; m_{b+1} < s_{b+1} < m_b
            m, s = f32(-(60 + 2 * b)), f32(-(59 + 2 * b))
            if b == len(LENGTHS) - 1:
                m = np.uint32(0x200).view(np.float32)            # a subnormal minimum: this recording is clamped
            if U > 1:
                x[ub, 0] = s
            x[ua, T - 1] = m
        else:                      # increasing chain: m_b in the first column, s_b in the last; m_b < s_b < m_{b+1}
            m, s = f32(-(80 - 2 * b)), f32(-(79 - 2 * b))
            if U > 1:
                x[ub, T - 1] = s
                if b % 2 == 0:
                    x[U // 2, 0 if b % 4 == 0 else T - 1] = 0.0   # the recording's only zero (U // 2 is ua or ub only for U = 1)
            x[ua, 0] = m
        recs.append(np.ascontiguousarray(x, np.float32))
    return recs


def host_front_end(x):
    """``process_HF0_fn`` in float32 (what the reference computes under NumPy 1.x, where the clamp case stays float32):
    (min positive, min, t, log(x + t) [U, T], _min)."""
    mp = x[x > 0].min()
    t = mp
    if np.log(t) < -87:
        t = np.float32(np.exp(-87))
    e = np.log(x + t)
    assert e.dtype == np.float32
    return mp, x.min(), np.float32(t), e, e.min()


def ulp_distance(a, b):
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16}[a.dtype.itemsize])


_CACHE = {}


def built(dev, U, variant):
    """Everything the checks of one (U, variant) need, computed once: the packed call on a slice of a wider buffer (fp32 with
    statistics, fp16), the per-recording calls, and the host reference."""
    k = (U, variant)
    if k in _CACHE:
        return _CACHE[k]
    recs = crafted(U, variant)
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    N = int(off[-1])
    lead, ld = (3, N + 13) if variant == 0 else (1, N + 16)        # row stride not / a multiple of four floats; base misaligned
    wide = torch.full((U, ld), float(f32(-100)), dtype=torch.float32, device=dev)
    hf0 = wide[:, lead:lead + N]
    hf0.copy_(torch.from_numpy(np.concatenate(recs, axis=1)))
    assert hf0.stride(0) == ld and hf0.data_ptr() % 16 != 0
    E32, stats = activation_log_emissions(hf0, offsets=off, return_stats=True)
    E16 = activation_log_emissions(hf0, offsets=torch.from_numpy(off).to(dev), dtype=torch.float16)     # device-resident offsets
    alone32, alone16, alone_stats = [], [], []
    for x in recs:
        xd = torch.from_numpy(x).to(dev)
        e, s = activation_log_emissions(xd, return_stats=True)
        alone32.append(e.cpu().numpy())
        alone_stats.append(s.cpu().numpy())
        alone16.append(activation_log_emissions(xd, dtype=torch.float16).cpu().numpy())
    torch.cuda.synchronize()
    assert torch.equal(wide[:, :lead], torch.full_like(wide[:, :lead], float(f32(-100))))
    out = {"recs": recs, "off": off, "E32": E32.cpu().numpy(), "E16": E16.cpu().numpy(), "E32_half": E32.to(torch.float16).cpu().numpy(),
           "stats": stats.cpu().numpy(), "alone32": alone32, "alone16": alone16, "alone_stats": alone_stats,
           "host": [host_front_end(x) for x in recs]}
    _CACHE[k] = out
    return out


@pytest.mark.parametrize("U,variant", SHAPES)
def test_statistics_are_the_hosts_bits(dev, U, variant):
    """(a) min positive, min and t per recording, bit for bit -- the subnormal minimum and its clamp included."""
    r = built(dev, U, variant)
    assert r["E32"].shape == (sum(LENGTHS), U + 1) and r["stats"].shape == (len(LENGTHS), 4)
    want = np.asarray([[h[0], h[1], h[2]] for h in r["host"]], np.float32)
    assert np.array_equal(bits(r["stats"][:, 0:3]), bits(want)), (r["stats"][:, 0:3], want)
    for b, s in enumerate(r["alone_stats"]):
        assert np.array_equal(bits(s[0, 0:3]), bits(want[b])), b
    if variant == 0:
        assert want[-1, 0] < np.finfo(np.float32).tiny and want[-1, 2] == np.float32(np.exp(-87))      # the clamped recording
        assert np.array_equal(want[:, 0], want[:, 1])                                                  # no zeros anywhere
    elif U > 1:
        assert np.array_equal(want[:, 1] == 0, np.arange(len(LENGTHS)) % 2 == 0)


@pytest.mark.parametrize("U,variant", SHAPES)
def test_unvoiced_column_is_the_written_minimum(dev, U, variant):
    """(b) column U is constant per recording and bit-equal to the minimum of that recording's other columns (and stats[:, 3])."""
    r = built(dev, U, variant)
    for name, E in (("float32", r["E32"]), ("float16", r["E16"])):
        for b in range(len(LENGTHS)):
            rows = E[r["off"][b]:r["off"][b + 1]]
            m = rows[:, :U].min()
            assert np.all(bits(rows[:, U]) == bits(m)), (name, b)
            if name == "float32":
                assert bits(r["stats"][b, 3]) == bits(m), b
    assert np.isfinite(r["E32"]).all() and np.isfinite(r["E16"].astype(np.float32)).all()


@pytest.mark.parametrize("U,variant", SHAPES)
def test_float16_is_the_rounded_float32(dev, U, variant):
    """(c) float16 storage = the float32 value rounded to nearest even."""
    r = built(dev, U, variant)
    assert r["E16"].dtype == np.float16
    assert np.array_equal(bits(r["E16"]), bits(r["E32_half"]))


@pytest.mark.parametrize("U,variant", SHAPES)
def test_packed_equals_each_recording_alone(dev, U, variant):
    """(d) one packed call on a strided, misaligned slice = a call per recording on its own contiguous tensor."""
    r = built(dev, U, variant)
    for b in range(len(LENGTHS)):
        sl = slice(r["off"][b], r["off"][b + 1])
        assert np.array_equal(bits(r["E32"][sl]), bits(r["alone32"][b])), b
        assert np.array_equal(bits(r["E16"][sl]), bits(r["alone16"][b])), b
        assert np.array_equal(bits(r["stats"][b]), bits(r["alone_stats"][b][0])), b


def test_agreement_with_the_host_function(dev):
    """(e) every value, the entries with HF0 == 0 and the unvoiced column included, within ULP_BOUND float32 ulp of the host's
    float32 ``process_HF0_fn`` -- over all inputs of this file: the crafted recordings and the seven golden cases."""
    worst, worst_zero, n = 0, 0, 0
    for U, variant in SHAPES:
        r = built(dev, U, variant)
        for b, (x, h) in enumerate(zip(r["recs"], r["host"])):
            rows = r["E32"][r["off"][b]:r["off"][b + 1]]
            d = ulp_distance(rows[:, :U], h[3].T)
            worst = max(worst, int(d.max()), int(ulp_distance(rows[:, U], np.full(len(rows), h[4], np.float32)).max()))
            if (x == 0).any():
                worst_zero = max(worst_zero, int(d[x.T == 0].max()))
            n += d.size
    man = json.load(open(os.path.join(HERE, "golden", "imm_manifest.json")))
    v = ImmViterbi(man["bins_per_semitone"], man["U"], device=dev)
    for case in man["cases"]:
        x = synth.hf0_activations(man["U"], case["T"], seed=case["seed"], denormal_min=case["denormal_min"]).numpy()
        host = v.process_HF0_fn(x)
        if host.dtype != np.float32:                 # the clamp case under NumPy >= 2: compare with the float32 computation
            h = host_front_end(x)
            host = np.concatenate([h[3], np.full((1, case["T"]), h[4], np.float32)])
        else:
            assert np.array_equal(host[:-1], host_front_end(x)[3])
        E = activation_log_emissions(torch.from_numpy(x).to(dev)).cpu().numpy()
        d = ulp_distance(E, host.T)
        worst = max(worst, int(d.max()))
        worst_zero = max(worst_zero, int(d[:, :-1][x.T == 0].max()))
        n += d.size
    print(f"activation front-end vs host process_HF0_fn: max {worst} ulp over {n} values ({worst_zero} ulp where HF0 == 0); bound {ULP_BOUND}")
    assert worst <= ULP_BOUND and worst_zero <= ULP_BOUND, (worst, worst_zero)


# ----------------------------------------------------------------------------------------------------------- paths
@pytest.fixture(scope="module")
def paths(dev):
    man = json.load(open(os.path.join(HERE, "golden", "imm_manifest.json")))
    gold = np.load(os.path.join(HERE, "golden", "imm_goldens.npz"))
    v = ImmViterbi(man["bins_per_semitone"], man["U"], device=dev)
    cases = [c for c in man["cases"] if c["T"] == 600]
    assert len(cases) == 3
    xs = [synth.hf0_activations(man["U"], c["T"], seed=c["seed"], denormal_min=c["denormal_min"], device=dev) for c in cases]
    for x, c in zip(xs, cases):
        assert sha(x.cpu().numpy()) == c["sha256_hf0"]                    # the generator gives the host's bits on the GPU
    return {"man": man, "gold": gold, "v": v, "cases": cases, "xs": xs, "alone": [v.decode_activations(x) for x in xs]}


def test_paths_are_the_oracles_decode_of_the_built_emissions(dev, paths):
    """(f) the decoder's own contract: the states of the GPU-built emissions are the oracle's decode of those same emissions, bit
    for bit -- float32 and float16 storage."""
    v = paths["v"]
    for dtype, name in ((torch.float32, "float32"), (torch.float16, "float16")):
        v16 = ImmViterbi(v.b, v.n_bins, device=dev, emission_dtype=name)
        for x, alone in zip(paths["xs"], paths["alone"]):
            E = activation_log_emissions(x, dtype=dtype)
            ref, _ = vo.decode_c(v.log_transition_matrix_T, v.log_prob_init, E.float().cpu().numpy()[None])
            got = v16.decode_activations(x)
            assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), ref[0])
            if dtype == torch.float32:
                assert torch.equal(got, alone)


def test_paths_against_the_host_exact_pipeline(dev, paths):
    """(f) against the golden states (the reference's ``process_HF0_fn`` + ``viterbi_librosa_fn``): the project's bar for a
    GPU-built front-end (test_gpu_parity.py::test_postprocessor_agreement_at_full_length) -- >= 99.9 % of the frames of every song
    equal, and every differing frame on a path whose exact score ties the reference path's to 1e-6 under the host's emissions."""
    v, man = paths["v"], paths["man"]
    logA_T, log_pi = v.log_transition_matrix_T, v.log_prob_init
    rates = []
    for x, c in zip(paths["xs"], paths["cases"]):
        ref = paths["gold"][f"states_{c['name']}"].astype(np.int64)
        got = v(x.cpu().numpy())                                             # the reference's call surface: NumPy in, NumPy out
        assert got.dtype == np.int64 and got.shape == (c["T"],)
        same = got == ref
        rates.append(float(same.mean()))
        if not same.all():
            logE = np.ascontiguousarray(v.process_HF0_fn(x.cpu().numpy()).T)
            T = c["T"]

            def score(s):
                return (float(log_pi[s[0]]) + logE[np.arange(T), s].astype(np.float64).sum() +
                        logA_T[s[1:], s[:-1]].astype(np.float64).sum())
            a, b = score(ref), score(got)
            assert abs(a - b) <= 1e-6 * abs(a), (c["name"], int((~same).sum()), a, b)
    print("imm HF0 -> path agreement with the host-exact pipeline:", rates)
    assert all(r >= 0.999 for r in rates), rates


def test_exact_entry_point_reproduces_the_goldens(dev, paths):
    """``viterbi_librosa_fn`` on the host front-end's output: the reference's states, every golden case (T = 1, 2, the clamp case)."""
    v, man = paths["v"], paths["man"]
    for c in man["cases"]:
        x = synth.hf0_activations(man["U"], c["T"], seed=c["seed"], denormal_min=c["denormal_min"]).numpy()
        st = v.viterbi_librosa_fn(np.asarray(v.process_HF0_fn(x), np.float32))
        assert st.dtype == np.int64 and np.array_equal(st, paths["gold"][f"states_{c['name']}"]), c["name"]


def test_recordings_in_one_pass(dev, paths):
    """``decode_activations_recordings`` -- one builder call, one packed decode -- equals ``decode_activations`` per recording:
    a list of recordings of different lengths, and the same as one concatenated buffer with offsets."""
    v = paths["v"]
    xs = [paths["xs"][0], paths["xs"][1][:, :65], paths["xs"][2][:, :1], paths["xs"][2]]
    want = [paths["alone"][0], v.decode_activations(xs[1]), v.decode_activations(xs[2]), paths["alone"][2]]
    got = v.decode_activations_recordings(xs)
    assert len(got) == 4
    for g, w in zip(got, want):
        assert g.dtype == torch.int64 and torch.equal(g, w)
    off = np.concatenate([[0], np.cumsum([x.shape[1] for x in xs])])
    got2 = v.decode_activations_recordings(torch.cat(xs, dim=1), off)
    for g, w in zip(got2, want):
        assert torch.equal(g, w)
