"""Seeded randomised parity over every decode entry point: the committed table of tests/random_cases.py, in blocks of consecutive
indices, every case through tests/random_check.check_case -- each entry point against its reference bit for bit, the served set
against the size queries and the documented refusals, workspaces filled with 0xFF before each call, and one case per block with
its outputs between guards (tests/guarded.Arena).

A failure names (seed, index, entry point, options).  To rerun that case alone:

    from tests import random_cases as rc, random_check as ck
    c = rc.case(seed, index)
    ck.check_case(ViterbiDecoder(c["A"], c["pi"], dev), c, dev)

scripts/fuzz_parity.py walks the same code past the table's end."""
import pytest
import torch

from tests import random_cases as rc
from tests import random_check as ck
from viterbi_spl_amd import ViterbiDecoder, _lib

pytestmark = pytest.mark.gpu

BLOCKS = rc.blocks()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _block_id(block):
    return f"s{block[0][0]}-{block[0][1]}..{block[-1][1]}"


@pytest.mark.parametrize("block", BLOCKS, ids=[_block_id(b) for b in BLOCKS])
def test_block(dev, block):
    n = moving = 0
    for k, (seed, index) in enumerate(block):
        c = rc.case(seed, index)
        refs = ck.host_references(c)
        a, m = ck.paths_change(refs["f32"][0], refs["f32"][1], c["lens"])
        n, moving = n + a, moving + m
        dec = ViterbiDecoder(c["A"], c["pi"], dev)
        try:
            runs = ck.check_case(dec, c, dev, refs=refs, guarded=k == 0)
        except AssertionError:
            raise
        except BaseException as e:                       # not a mismatch: nothing more is started on a device that may have faulted
            pytest.exit(f"case ({seed}, {index}) {rc.case_id(c)}: {type(e).__name__}: {e}", returncode=3)
        assert runs >= len(c["decode_forms"]), (rc.case_id(c), runs)
    # the block's premise, from the reference alone: of the songs with at least 17 frames and a finite log-likelihood, at least half
    # have a path that changes state (tests/test_random_cases_host.py holds the table to it without a GPU)
    assert 2 * moving >= n, (block, moving, n)
