"""The back-trace event counters of a few small, fixed decodes against the values recorded in tests/golden/bt_counters.json
(tests/golden/make_bt_counters.py): equal key by key.  The parity tests pin the decoded path; a chunk driver that fetches a tile or
repairs a chunk too many still decodes the right path, and only the counters show it.  The counters are integer sums of per-wave
counts, so they do not depend on the order in which the waves run.

The lean whole-row kernel (tonet361_form2) and the lazy kernel (durrieu722_lazy) count no events: their records are all zeros, and
for them the comparison pins only that they go on counting nothing, beside the parity check of the same decode."""
import json

import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests.golden import make_bt_counters as mk
from viterbi_spl_amd import ViterbiDecoder, _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def recorded():
    with open(mk.OUT) as fh:
        return json.load(fh)


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(mk.CASES)
    keys = sorted(f"{c}|{w}" for c, w in mk.CHUNKINGS)
    for name, rec in recorded.items():
        assert sorted(rec) == keys, name
        for ct in rec.values():
            assert sorted(ct) == sorted(ViterbiDecoder.COUNTERS), name
    # the record is not a list of zeros: every kernel family that counts fetched tiles, and seven chunks without a warm-up
    # leave wrong guesses to repair
    for name in ("tonet361_full_form0", "tonet361_half", "jdc722_form0"):
        assert all(ct["tiles_fetched"] >= sum(n - 1 for n in mk.LENGTHS) // 16 for ct in recorded[name].values()), name
    for k in ("chunks_repaired", "frames_repaired"):
        assert any(rec["7|0"][k] > 0 for rec in recorded.values()), k


@pytest.mark.parametrize("name", sorted(mk.CASES))
def test_counters_are_the_recorded_ones(golden, dev, recorded, name):
    plan = mk.CASES[name][0]
    A, pi = golden["params"][f"{plan}_logA_T"], golden["params"][f"{plan}_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    E, lens = mk.case_inputs(name, dev)
    ref_s, ref_l = vo.decode_c(A, pi, E.cpu().numpy(), lengths=lens.cpu().numpy())

    def check(st, ll, key):
        assert np.array_equal(st.cpu().numpy(), ref_s), (name, key)
        assert np.array_equal(ll.cpu().numpy(), ref_l), (name, key)

    got = mk.case_counters(dec, name, E, lens, check)
    print(name, json.dumps(got, sort_keys=True))
    assert sorted(got) == sorted(recorded[name])
    wrong = {(key, k): (got[key][k], recorded[name][key][k]) for key in got for k in got[key] if got[key][k] != recorded[name][key][k]}
    assert not wrong, f"{name}: (counted, recorded) {wrong}"
