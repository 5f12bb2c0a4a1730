"""Host tier of the packed back-traces' chunk table (vit::packed_chunk_table in csrc/plan.cpp; vit_decode_packed's lane and lazy
branches and vit_decode_f64_packed call it), reached through the host-only plan library, against a few lines that restate the rule.
No GPU.  The constants are the callers' on a 256-unit device (a plan that was never uploaded)."""
import ctypes

import numpy as np
import pytest

from tests import plan_replay

N_CUS = 256
# (streams wanted at once, most chunks of a song, shortest chunk, rounded to nearest, capacity the layouts reserve beyond B)
LANE = (16 * 64 * N_CUS, 256, 4 * 64, True, 16 * 64 * N_CUS)      # one stream per lane: kLaneMaxChunks, 4 * kBtWarmSparse; pk_max_waves
WAVE = (8 * N_CUS, 32, 8 * 128, False, 8 * N_CUS)                 # one per wave (step plans, float64): kBtMaxChunks, 8 * kBtWarm
GUARD = -7


def _lists():
    rng = np.random.default_rng(20)
    out = [[1], [1, 2, 63, 64, 65, 700], [30000] + [10] * 50, [9000] * 3250]
    for k in range(20):                               # short and long songs mixed, one to a few thousand of them
        B = int(rng.integers(1, 4000 if k % 4 == 0 else 60))
        out.append(rng.integers(1, 30001 if k % 2 else 3000, size=B).tolist())
    return out


@pytest.fixture(scope="module")
def host():
    plan_replay._lib()                                # builds the host library where it is missing
    lib = ctypes.CDLL(plan_replay.LIB)
    lib.vph_packed_chunk_table.restype = ctypes.c_int
    lib.vph_packed_chunk_table.argtypes = [ctypes.c_void_p] + [ctypes.c_longlong] * 4 + [ctypes.c_int, ctypes.c_longlong] + [ctypes.c_void_p] * 3
    return lib


def _rule(lens, streams, cap, shortest, nearest):
    """chunks per song: about cf frames each, cf = max(ceil(N / streams), shortest, ceil(longest / cap))"""
    cf = max(-(-sum(lens) // streams), shortest, -(-max(lens) // cap))
    return [min(max((t + cf // 2) // cf if nearest else t // cf, 1), cap) for t in lens]


def _table(host, lens, form, capacity):
    streams, cap, shortest, nearest, _ = form
    off = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)
    B = len(lens)
    base = np.full(B + 1, GUARD, np.int32)
    waves = np.full(max(capacity, 0) + 64, GUARD, np.int32)
    largest = ctypes.c_longlong(GUARD)
    ok = host.vph_packed_chunk_table(off.ctypes.data, B, streams, cap, shortest, int(nearest), capacity, base.ctypes.data, waves.ctypes.data,
                                     ctypes.byref(largest))
    return ok, base, waves, largest.value


@pytest.mark.parametrize("form", [LANE, WAVE], ids=["lane-nearest", "wave-down"])
def test_chunk_table_is_the_rule(host, form):
    streams, cap, shortest, nearest, beyond = form
    some_split = False
    for lens in _lists():
        B, want = len(lens), _rule(lens, *form[:4])
        total, reserved = sum(want), B + beyond
        assert total <= reserved, "the rule itself leaves the capacity the layouts reserve: the inputs are wrong"
        ok, base, waves, largest = _table(host, lens, form, reserved)
        assert ok == 1
        assert base[0] == 0 and (np.diff(base) >= 1).all() and (np.diff(base) <= cap).all()       # increasing; 1 .. cap chunks a song
        assert np.diff(base).tolist() == want and base[B] == total <= reserved and largest == max(want)
        assert np.array_equal(waves[:total], np.repeat(np.arange(B, dtype=np.int32), want))         # wave_song[base[b] : base[b + 1]] == b
        assert (waves[total:] == GUARD).all()
        some_split |= max(want) > 1
        # a capacity one short of the total: failure, and nothing at or behind the capacity is written
        ok, base, waves, _ = _table(host, lens, form, total - 1)
        assert ok == 0 and (waves[total - 1:] == GUARD).all()
        ok, _, waves, _ = _table(host, lens, form, total)                                           # exactly enough
        assert ok == 1 and (waves[total:] == GUARD).all()
    assert some_split, "no list of the set takes more than one chunk a song"
