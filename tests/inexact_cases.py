"""The cases of tests/test_inexact_host.py and tests/test_gpu_inexact.py: the off-grid twins (tests/inexact.py) of the matrices the
geometry tests of tests/test_gpu_parity.py decode on dyadic grids, and log-probability inputs for the unstructured dense kernels.
NumPy only; every case is built once per session and never written to.

  family      cases                                                                      structures (for the back-trace premise)
  wave        wave0 .. wave9: floor_grid.wave_geometry, T = 131, B = 1 / 3 / 5 / 9 / 13   0, 1, 2 extra columns
  path        the five matrices of floor_grid.kernel_path_matrices, B = 6                 one each
  banded      banded0 .. banded7: floor_grid.random_banded_structure, B = 6               floor -50, -3, -inf
  sparse      the three floor_grid.SPARSE_GRID plans, B = 6                               one
  dense       S = 1 .. 369, T = 37, B = 3, fp32 and fp16; S = 97 with B = 9, 77, 131      one (unstructured)
  wide        floor_grid.few_wide_rows at S = 200, forced emissions, B = 4                one
  step        common.step_matrix with 1, 3, 9, 14 and 15 near bands, B = 4, both types    one

Premises, asserted by tests/test_inexact_host.py on the reference recursion alone: premise_rounds >= 0.5 and a visible forward
mutant in every case, a back-trace mutant that changes a state in at least one case of every structure.  RESEED holds the twin
seeds that were moved to get there (the first of 0, 1, 2, ... that meets them).  S = 1 is the one exception: its only
log-probability is log(1) = 0, every sum is exact, and the case stays for the kernel's sake.

Measured (share of candidate sums that round | forward mutant visible | states the back-trace mutant changes):
  wave0 0.867 yes 0                      wave1 0.943 yes 1                      wave2 0.870 yes 0
  wave3 0.780 yes 3                      wave4 0.533 yes 6                      wave5 0.615 yes 0
  wave6 0.810 yes 0                      wave7 0.870 yes 7                      wave8 0.829 yes 6
  wave9 0.804 yes 0                      path0 0.807 yes 1                      path1 0.626 yes 2
  path2 0.808 yes 2                      path3 0.779 yes 1                      path4 0.811 yes 1
  banded0 0.526 yes 5                    banded1 0.754 yes 1                    banded2 0.730 yes 0
  banded3 0.813 yes 0                    banded4 0.746 yes 0                    banded5 0.623 yes 17
  banded6 0.534 yes 0                    banded7 0.766 yes 0                    sparse0 0.770 yes 2
  sparse1 0.545 yes 1                    sparse2 0.537 yes 0                    dense1-f32 0.000 no 0
  dense1-f16 0.000 no 0                  dense2-f32 0.995 yes 0                 dense2-f16 0.986 yes 0
  dense33-f32 0.927 yes 0                dense33-f16 0.927 yes 0                dense63-f32 0.926 yes 0
  dense63-f16 0.926 yes 0                dense64-f32 0.924 yes 0                dense64-f16 0.924 yes 0
  dense65-f32 0.925 yes 0                dense65-f16 0.926 yes 0                dense97-f32 0.919 yes 0
  dense97-f16 0.919 yes 0                dense128-f32 0.919 yes 0               dense128-f16 0.919 yes 0
  dense129-f32 0.919 yes 0               dense129-f16 0.919 yes 0               dense200-f32 0.927 yes 0
  dense200-f16 0.927 yes 0               dense256-f32 0.932 yes 0               dense256-f16 0.932 yes 0
  dense257-f32 0.932 yes 0               dense257-f16 0.932 yes 0               dense361-f32 0.936 yes 0
  dense361-f16 0.936 yes 0               dense368-f32 0.935 yes 0               dense368-f16 0.935 yes 0
  dense369-f32 0.935 yes 0               dense369-f16 0.935 yes 0               dense97-B9 0.909 yes 0
  dense97-B77 0.910 yes 6                dense97-B131 0.907 yes 0               wide200 0.513 yes 3
  step-n128-bw4-kb1-f32 0.651 yes 1      step-n128-bw4-kb1-f16 0.730 yes 0      step-n400-bw5-kb3-f32 0.740 yes 0
  step-n400-bw5-kb3-f16 0.641 yes 0      step-n707-bw20-kb9-f32 0.662 yes 0     step-n707-bw20-kb9-f16 0.800 yes 0
  step-n1023-bw64-kb14-f32 0.900 yes 0   step-n1023-bw64-kb14-f16 0.726 yes 0   step-n128-bw4-kb15-f32 0.866 yes 0
  step-n128-bw4-kb15-f16 0.815 yes 0
"""
import functools
import types
import zlib

import numpy as np

from tests import floor_grid as fg
from tests import inexact as ix
from tests.common import emissions_jumps, step_matrix

T_BAND = 131
WAVE_B = (1, 3, 5, 9, 13)
DENSE_S = (1, 2, 33, 63, 64, 65, 97, 128, 129, 200, 256, 257, 361, 368, 369)
DENSE_T, DENSE_B = 37, 3
GROUPS_B, GROUPS_T = (9, 77, 131), 40
STEP_GEOMETRIES = ((128, 4, 1), (400, 5, 3), (707, 20, 9), (1023, 64, 14), (128, 4, 15))       # (n, bw, kb): one per near-band count
PATH_NAMES = ("floor+lean_affine", "floor+lean_table", "scan+lean", "scan+generic", "scan(full waves)+lean")

# case id -> the twin's seed index, where 0 misses a premise
RESEED = {"banded0": 5, "banded2": 1, "banded5": 10, "banded7": 1, "dense2": 1, "dense361": 3, "dense368": 2, "dense369": 1,
          "dense63": 2, "dense64": 1, "dense65": 1, "dense97": 4, "dense97-B77": 20, "path0": 2, "path1": 10, "path3": 40,
          "path4": 4, "sparse1": 1, "step-n128-bw4-kb1-f16": 1, "step-n128-bw4-kb1-f32": 6, "step-n400-bw5-kb3-f16": 59,
          "step-n707-bw20-kb9-f16": 2, "wide200": 11}


def _rng(cid, what):
    return np.random.default_rng([zlib.crc32(cid.encode()), what, RESEED.get(cid, 0)])


def _case(cid, family, structure, A, pi, E32, lens, f16, A0=None, pi0=None, E0=None, **meta):
    E, E16 = ix.stored(E32, f16)
    for x in (A, pi, E, A0, pi0, E0):
        if x is not None:
            x.setflags(write=False)
    return types.SimpleNamespace(id=cid, family=family, structure=structure, A=A, pi=pi, E=E, E16=E16, lens=np.asarray(lens, np.int64),
                                 f16=f16, A0=A0, pi0=pi0, E0=E0, S=A.shape[0], B=E.shape[0], T=E.shape[1], **meta)


def _twin(cid, family, structure, A0, pi0, E0, lens, f16, **meta):
    """The off-grid twin of (A0, pi0, E0): one map over the whole matrix, one over the prior, an offset per emission."""
    rng = _rng(cid, 1)
    A0, pi0, E0 = np.ascontiguousarray(A0, np.float32), np.ascontiguousarray(pi0, np.float32), np.ascontiguousarray(E0, np.float32)
    A, pi = ix.off_grid(A0, rng), ix.off_grid(pi0, rng)
    return _case(cid, family, structure, A, pi, ix.off_grid_emissions(E0, rng), lens, f16, A0=A0, pi0=pi0, E0=E0, **meta)


def _grid_emissions(rng, B, T, S, levels):
    return -(rng.integers(0, levels, (B, T, S)) / 2).astype(np.float32)


def _wave(seed):
    S, half, extras, A0, pi0, rng = fg.wave_geometry(seed)
    B = WAVE_B[seed % 5]
    return _twin(f"wave{seed}", "wave", f"{len(extras)} extras", A0, pi0, _grid_emissions(rng, B, T_BAND, S, 12), ix.ragged(B, T_BAND),
                 bool(seed & 1), seed=seed, half=half, extras=extras)


def _path(k):
    rng = np.random.default_rng(2024)
    mats = fg.kernel_path_matrices(rng)
    for i, name in enumerate(PATH_NAMES):                   # (the draws of the prior and the emissions follow the matrices, in order)
        A0 = mats[name]
        S = A0.shape[0]
        pi0 = -(rng.integers(0, 8, S) / 2).astype(np.float32)
        E0 = _grid_emissions(rng, 6, T_BAND, S, 6)
        if i == k:
            return _twin(f"path{k}", "path", name, A0, pi0, E0, ix.ragged(6, T_BAND), bool(k & 1), name=name)


def _banded(seed):
    S, half, extras, dense_rows, A0, pi0, rng = fg.random_banded_structure(seed)
    floor = ("floor -50", "floor -3", "floor -inf")[seed % 3]
    return _twin(f"banded{seed}", "banded", floor, A0, pi0, _grid_emissions(rng, 6, T_BAND, S, 6), ix.ragged(6, T_BAND), bool(seed & 1),
                 seed=seed, half=half, extras=extras, dense_rows=dense_rows)


def _sparse(k):
    (W, n), (S, half) = sorted(fg.SPARSE_GRID.items())[k]
    entry = (W, n, S, half, "sparse")
    A0, pi0 = fg.plan_params(entry)
    rng = _rng(f"sparse{k}", 0)
    return _twin(f"sparse{k}", "sparse", "sparse band", A0, pi0, _grid_emissions(rng, 6, T_BAND, S, 12), ix.ragged(6, T_BAND), bool(k & 1),
                 entry=entry, W=W)


def _dense(S, f16):
    rng = _rng(f"dense{S}", 0)                              # (one matrix and one batch per S: the fp16 case stores the same emissions)
    A, pi = ix.logprob_matrix(S, rng), ix.logprob_prior(S, rng)
    E = ix.logprob_emissions(DENSE_B, DENSE_T, S, rng)
    return _case(f"dense{S}-{'f16' if f16 else 'f32'}", "dense", "unstructured", A, pi, E, ix.ragged(DENSE_B, DENSE_T), f16)


def _groups(B):
    rng = _rng(f"dense97-B{B}", 0)
    A, pi = ix.logprob_matrix(97, rng), ix.logprob_prior(97, rng)
    return _case(f"dense97-B{B}", "dense", "unstructured", A, pi, ix.logprob_emissions(B, GROUPS_T, 97, rng), ix.ragged(B, GROUPS_T), False)


def _wide():
    rng = np.random.default_rng(4242)
    S = 200
    A0 = fg.few_wide_rows(S, rng, fg.WIDE_ROWS)
    pi0 = -(rng.integers(0, 8, S) / 2).astype(np.float32)
    E0 = fg.wide_row_emissions(rng, 4, T_BAND, S)
    return _twin("wide200", "wide", "few wide rows", A0, pi0, E0, [T_BAND, T_BAND - 1, 40, 1], False)


def _step(k, f16):
    n, bw, kb = STEP_GEOMETRIES[k]
    A0 = step_matrix(n, bw, kb, np.random.default_rng(1000 * n + 16 * bw + kb))
    pi0 = np.full(n + 1, np.float32(np.log(np.float32(1.0 / (n + 1)))), np.float32)
    E0 = emissions_jumps(4, T_BAND, n + 1, 100 + n, bw)
    return _twin(f"step-n{n}-bw{bw}-kb{kb}-{'f16' if f16 else 'f32'}", "step", "step", A0, pi0, E0, ix.ragged(4, T_BAND), f16, n=n, bw=bw, kb=kb)


_BUILDERS = {}
for _s in fg.WAVE_GEOMETRY_SEEDS:
    _BUILDERS[f"wave{_s}"] = functools.partial(_wave, _s)
for _k in range(len(PATH_NAMES)):
    _BUILDERS[f"path{_k}"] = functools.partial(_path, _k)
for _s in fg.RANDOM_BANDED_SEEDS:
    _BUILDERS[f"banded{_s}"] = functools.partial(_banded, _s)
for _k in range(len(fg.SPARSE_GRID)):
    _BUILDERS[f"sparse{_k}"] = functools.partial(_sparse, _k)
for _S in DENSE_S:
    for _f in (False, True):
        _BUILDERS[f"dense{_S}-{'f16' if _f else 'f32'}"] = functools.partial(_dense, _S, _f)
for _B in GROUPS_B:
    _BUILDERS[f"dense97-B{_B}"] = functools.partial(_groups, _B)
_BUILDERS["wide200"] = _wide
for _k, (_n, _bw, _kb) in enumerate(STEP_GEOMETRIES):
    for _f in (False, True):
        _BUILDERS[f"step-n{_n}-bw{_bw}-kb{_kb}-{'f16' if _f else 'f32'}"] = functools.partial(_step, _k, _f)

IDS = tuple(_BUILDERS)
FAMILY = {cid: ("dense" if cid.startswith("dense") else "step" if cid.startswith("step") else "wide" if cid.startswith("wide")
                else cid.rstrip("0123456789")) for cid in IDS}


def ids(family):
    return tuple(cid for cid in IDS if FAMILY[cid] == family)


@functools.lru_cache(maxsize=None)
def case(cid):
    return _BUILDERS[cid]()


@functools.lru_cache(maxsize=None)
def oracle(cid):
    """(states int32 [B, T], loglik float32 [B], last delta row [B, S]) of oracle.viterbi_oracle.decode_c."""
    from oracle import viterbi_oracle as vo
    c = case(cid)
    return vo.decode_c(c.A, c.pi, c.E, lengths=c.lens, return_delta=True)


@functools.lru_cache(maxsize=None)
def premises(cid):
    """(premise_rounds, forward mutant visible, states changed by the back-trace mutant) of the case, on the reference alone."""
    c = case(cid)
    visible, changed, _ = ix.premise_mutants(c.A, c.pi, c.E, c.lens)
    return ix.premise_rounds(c.A, c.pi, c.E, c.lens), visible, changed
