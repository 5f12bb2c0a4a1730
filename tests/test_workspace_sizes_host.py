"""Every workspace-size query of the library, for every named plan of tests/golden/params.npz and the scan-only variant of jdc722,
against the answers recorded in tests/golden/workspace_sizes.json (tests/golden/make_workspace_sizes.py): equal byte for byte, the
zeros of the refused queries included.  No GPU: a plan that was never uploaded assumes 256 compute units.  The file is a record of
what callers allocate today -- a change of the host layer that moves one of these numbers breaks their buffers."""
import json
import os

import pytest

from tests.golden import make_workspace_sizes as mk


@pytest.fixture(scope="module")
def lib():
    from viterbi_spl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module")
def recorded():
    with open(mk.OUT) as fh:
        return json.load(fh)


def test_every_plan_is_recorded(golden, recorded):
    assert sorted(recorded) == sorted(mk.plan_names(golden["params"]) + [mk.SCAN_ONLY])
    n = len(mk.SHAPES) * (1 + 2 * len(mk.ALGOS) + len(mk.SEGMENTS) + len(mk.BUILDERS)) + len(mk.LENGTHS) * (1 + 2 * len(mk.SEGMENTS))
    n += len(mk.SHAPES) * (1 + len(mk.SEGMENTS)) + len(mk.LENGTHS)                   # the float64 decodes: padded, checkpointed, packed
    n += len({B for B, _ in mk.SHAPES} | {len(lens) for lens in mk.LENGTHS})          # vit_packed_bounded_units
    assert all(len(v) == n for v in recorded.values())
    # the record is not a list of zeros: every family of queries answers for some plan, and refuses for some
    for prefix in ("bytes", "for", "checkpointed", "logits", "units", "packed", "packed_checkpointed", "packed_bounded", "f64", "f64_checkpointed",
                   "f64_packed"):
        vals = [v for plan in recorded.values() for k, v in plan.items() if k.split("|")[0] == prefix]
        assert any(v > 0 for v in vals), prefix
        assert prefix == "bytes" or any(v == 0 for v in vals), prefix


def _names():
    import numpy as np
    params = np.load(os.path.join(os.path.dirname(mk.OUT), "params.npz"))
    return mk.plan_names(params) + [mk.SCAN_ONLY]


@pytest.mark.parametrize("name", _names())
def test_sizes_are_the_recorded_ones(lib, golden, recorded, name):
    p = golden["params"]
    A, pi = mk.scan_only_jdc722(p) if name == mk.SCAN_ONLY else (p[f"{name}_logA_T"], p[f"{name}_log_pi"])
    got = mk.plan_sizes(lib, A, pi)
    assert sorted(got) == sorted(recorded[name])
    wrong = {k: (got[k], recorded[name][k]) for k in got if got[k] != recorded[name][k]}
    assert not wrong, f"{name}: (answer, recorded) {wrong}"
