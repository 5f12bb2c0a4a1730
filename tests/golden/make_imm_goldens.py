"""Golden vectors for imm's decoder (the seventh "model output -> path" call surface), generated in the build container from the
reference's own class:

  * ``Viterbi.__init__(self, bins_per_semitone, n_bins)``   imm/tf_imm.py:51-68   (np.log(A.T) without tiny, uniform prior)
  * ``Viterbi.process_HF0_fn(self, HF0)``                    imm/tf_imm.py:70-88   (activations -> log-emissions)
  * ``Viterbi.viterbi_librosa_fn(self, log_HF0)``            imm/tf_imm.py:90-127  (the log-domain decode)

Only these three ``ast.FunctionDef`` nodes are compiled (the module itself needs TensorFlow, librosa, soundfile, matplotlib);
``imm/transition_matrix.py`` is loaded by file path; ``tf`` is a stub whose ``Tensor`` nothing is an instance of.  Commits data only:
seeds, the SHA-256 of the regenerated inputs, hashes of the reference's parameters, ``t`` / ``_min`` / a SHA-256 of
``process_HF0_fn``'s output per case, and the decoded states (uint16).

In the clamp case the reference adds ``np.exp(-87)``, a float64 scalar: under NumPy >= 2 its ``process_HF0_fn`` then returns a
float64 array, which its own ``viterbi_librosa_fn`` refuses (``assert log_HF0.dtype == np.float32``).  The manifest records the
dtype the reference returned; the states of such a case are the reference's decode of that output cast to float32 (``cast``).

    python tests/golden/make_imm_goldens.py        (REFERENCE_ROOT: where the reference repository lies)
"""
import ast
import hashlib
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")

from viterbi_spl_amd import synth                # noqa: E402

U, BPS = 721, 20
CASES = (
    {"name": "T1", "T": 1, "seed": 201, "denormal_min": False},
    {"name": "T2", "T": 2, "seed": 202, "denormal_min": False},
    {"name": "T63_clamp", "T": 63, "seed": 203, "denormal_min": True},
    {"name": "T257", "T": 257, "seed": 204, "denormal_min": False},
    {"name": "T600_a", "T": 600, "seed": 205, "denormal_min": False},
    {"name": "T600_b", "T": 600, "seed": 206, "denormal_min": False},
    {"name": "T600_c", "T": 600, "seed": 207, "denormal_min": False},
)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def case_input(case):
    return synth.hf0_activations(U, case["T"], seed=case["seed"], denormal_min=case["denormal_min"]).numpy()


def reference_class():
    """The reference's ``Viterbi`` with only the three methods, compiled from their AST nodes."""
    spec = importlib.util.spec_from_file_location("ref_imm_transition_matrix", f"{REF}/imm/transition_matrix.py")
    tm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tm)
    tf = types.SimpleNamespace(Tensor=type("Tensor", (), {}))
    tree = ast.parse(open(f"{REF}/imm/tf_imm.py").read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Viterbi")
    want = ("__init__", "process_HF0_fn", "viterbi_librosa_fn")
    cls.body = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert [n.name for n in cls.body] == list(want)
    ns = {"np": np, "tf": tf, "gen_transition_matrix_fn": tm.gen_transition_matrix_fn}
    exec(compile(ast.Module(body=[cls], type_ignores=[]), "ref_imm_Viterbi", "exec"), ns)
    return ns["Viterbi"]


def main():
    Viterbi = reference_class()
    params = {}
    for n_bins in (721, 720):
        v = Viterbi(BPS, n_bins)
        assert v.log_transition_matrix_T.dtype == np.float32 and v.log_prob_init.dtype == np.float32
        params[f"{BPS}_{n_bins}"] = {"sha256_log_transition_matrix_T": sha(v.log_transition_matrix_T),
                                    "sha256_log_prob_init": sha(v.log_prob_init)}
    vit = Viterbi(BPS, U)
    arrays, cases = {}, []
    for case in CASES:
        x = case_input(case)
        out = vit.process_HF0_fn(x)
        assert out.shape == (U + 1, case["T"])
        cast = out.dtype != np.float32
        states = vit.viterbi_librosa_fn(np.asarray(out, np.float32))
        assert states.dtype == np.int64 and states.shape == (case["T"],) and states.max() <= U
        mp = x[x > 0].min()
        rec = dict(case)
        rec.update({"sha256_hf0": sha(x), "zeros": int(np.sum(x == 0)), "min_positive_bits": int(mp.view(np.uint32)),
                    "clamped": bool(np.log(mp) < -87), "out_dtype": str(out.dtype), "cast": bool(cast),
                    "min": float(out[U, 0]), "min_hex": float(out[U, 0]).hex(), "sha256_out": sha(out),
                    "unvoiced_frames": int(np.sum(states == U))})
        # t as the reference holds it: the smallest positive entry, or exp(-87)
        t = np.exp(-87) if rec["clamped"] else mp
        rec["t"], rec["t_hex"] = float(t), float(t).hex()
        cases.append(rec)
        arrays[f"states_{case['name']}"] = states.astype(np.uint16)
        print(case["name"], "zeros", rec["zeros"], "clamped", rec["clamped"], out.dtype, "min", rec["min"], "unvoiced", rec["unvoiced_frames"])
    assert any(c["clamped"] for c in cases) and any(c["zeros"] for c in cases)
    np.savez_compressed(os.path.join(HERE, "imm_goldens.npz"), **arrays)
    with open(os.path.join(HERE, "imm_manifest.json"), "w") as fh:
        json.dump({"U": U, "bins_per_semitone": BPS, "numpy": np.__version__, "params": params, "cases": cases,
                   "inputs": "synth.hf0_activations(U, T, seed, denormal_min=...)",
                   "reference": ["imm/tf_imm.py:51-68", "imm/tf_imm.py:70-88", "imm/tf_imm.py:90-127", "imm/transition_matrix.py:3-27"]},
                  fh, indent=1)


if __name__ == "__main__":
    main()
