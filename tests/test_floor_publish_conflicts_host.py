"""Publication of a new delta row by the split floor kernel, replayed by the host library (vph_split_maps, vph_split_lds_conflicts;
the maps are the kernel's own constexpr functions in plan.hpp):

* every target's four copies land where the readers look: copy r of buffer b holds delta[i] at float b * BUF + r * DC + 4 + sh + i - r,
  which is where a lane whose window starts at delta[lo] with (lo + sh) % 4 == r reads from (floor_lds_check.hip replays the same
  against the layout); full waves write all four, the two lanes of a half-wave target two each, four between them;
* the frame-maximum slots: slots 0 .. 2 of a group together receive every non-extra target, slot 3 receives only column x, and the
  lanes of x's quad add into nothing that M is read from;
* the conflict cycles (what SQ_LDS_BANK_CONFLICT counts) of every LDS instruction of a frame per role and buffer: no other copy
  assignment the half waves can take without another instruction has fewer than the kernel's, for every role and both buffers.
  The figures themselves are printed (pytest -s) and recorded in DESIGN.md 7; the replay is a model, not a measurement."""
import ctypes

import numpy as np
import pytest

from tests import plan_replay

DC = 384 + 16
BUF = 4 * DC
GRIDS = ((361, 15, 29), (321, 13, 25), (361, 15, 32))      # states, window offset of the affine plan (lo_j = j - off), full-wave width
KINDS = ("slot quad read", "window b128", "window b32", "copy writes", "ds_max_f32", "slot reset")


@pytest.fixture(scope="module")
def lib():
    lib = plan_replay._lib()
    lib.vph_split_maps.restype = ctypes.c_int
    lib.vph_split_maps.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p]
    lib.vph_split_lds_conflicts.restype = ctypes.c_int
    lib.vph_split_lds_conflicts.argtypes = [ctypes.c_int] * 7 + [ctypes.c_void_p]
    return lib


def _maps(lib, S, off, wave, lane, b):
    out = np.zeros(9, np.int32)
    assert lib.vph_split_maps(S, off, wave, lane, b, out.ctypes.data) == 0
    return [int(v) for v in out]


def _conflicts(lib, S, off, WF, wave, rb, serial, assignment):
    out = np.zeros(6, np.int32)
    assert lib.vph_split_lds_conflicts(S, off, WF, wave, rb, serial, assignment, out.ctypes.data) == 0
    return [int(v) for v in out]


@pytest.mark.parametrize("S,off", [(361, 15), (321, 13)])
def test_four_copies_land_where_the_readers_look(lib, S, off):
    sh = off % 4
    for b in range(2):
        written = {}                                     # (target, copy) -> position
        for wave in range(8):
            for lane in range(64):
                m = _maps(lib, S, off, wave, lane, b)
                j, hh = m[0], m[1]
                copies = range(4) if wave < 4 else (2 * hh, 2 * hh + 1)
                pos = [p for p in m[4:8] if p >= 0]
                assert len(pos) == len(copies), (wave, lane, m)
                for r, p in zip(copies, pos):
                    assert p == b * BUF + r * DC + 4 + sh + j - r, (wave, lane, r, p)
                    assert written.setdefault((j, r), p) == p
        assert set(written) == {(j, r) for j in range(384) for r in range(4)}, "every target slot, four copies"
        # a reader's window start: 16-byte aligned, inside the copy that aligns it, and the float there is delta[lo] of that copy
        for wave in range(8):
            for lane in range(64):
                m = _maps(lib, S, off, wave, lane, b)
                j, hh, first = m[0], m[1], m[8]
                lo = min(max(j - off, 0), S - 32) if j < S else S - 32
                r = (lo + sh) % 4
                assert first % 4 == 0
                assert first == written[(lo + 16 * hh, r)], (wave, lane, j, lo, r)


@pytest.mark.parametrize("S,off", [(361, 15), (321, 13)])
def test_slots_of_the_frame_maximum(lib, S, off):
    x = S - 1
    into = {0: set(), 1: set(), 2: set(), 3: set()}
    for wave in range(8):
        quads = {}
        for lane in range(64):
            m = _maps(lib, S, off, wave, lane, 0)
            quads.setdefault(lane // 4, []).append(m[0])
        for lane in range(64):
            m = _maps(lib, S, off, wave, lane, 0)
            j = m[0]
            slot = m[3] if j == x else m[2]
            assert 0 <= slot < 16
            if slot < 4:
                # the lane adds the maximum over its quad
                into[slot] |= set(quads[lane // 4])
    assert into[3] == {x, x + 1, x + 2, x + 3} and all(j >= S for j in into[3] - {x}), "slot 3: column x and its idle quad mates only"
    m_slots = into[0] | into[1] | into[2]
    assert x not in m_slots
    assert {j for j in range(S) if j != x} <= m_slots, "M misses a non-extra target"


@pytest.mark.parametrize("S,off,WF", GRIDS)
def test_no_copy_assignment_has_fewer_conflict_cycles(lib, S, off, WF):
    for serial in (0, 1):
        totals = []
        for assignment in range(4):
            total = 0
            for rb in range(2):
                for wave in range(8):
                    now = _conflicts(lib, S, off, WF, wave, rb, serial, 0)
                    alt = _conflicts(lib, S, off, WF, wave, rb, serial, assignment)
                    assert sum(alt) >= sum(now), (S, WF, wave, rb, assignment, now, alt)
                    assert alt[:3] == now[:3] and alt[4:] == now[4:], "the assignment moves the copy writes only"
                    total += sum(alt)
                    if assignment == 0 and serial == 1 and rb == 0:
                        print(f"S {S} WF {WF} wave {wave}: " + ", ".join(f"{k} {v}" for k, v in zip(KINDS, now)))
            totals.append(total / 16)
        print(f"S {S} WF {WF}, ds_max_f32 lanes of one address {'serialised' if serial else 'combined'}: "
              f"extra LDS cycles per wave-frame by copy assignment {totals}")
        assert min(totals) == totals[0]


def test_conflict_replay_of_the_present_map(lib):
    """What the model gives for the headline kernel: the linear add-tid stores, the broadcast slot read and the reset are
    conflict-free; each half wave pays 4 cycles for its two-way copy writes; every wave's ds_max_f32 has three lanes on its busiest
    address in each 32-lane group."""
    for rb in range(2):
        for wave in range(8):
            c = _conflicts(lib, 361, 15, 29, wave, rb, 1, 0)
            assert c[0] == 0 and c[5] == 0
            assert c[3] == (0 if wave < 4 else 4)
            assert c[4] == 4
            assert _conflicts(lib, 361, 15, 29, wave, rb, 0, 0)[4] == 0
    assert lib.vph_split_lds_conflicts(400, 15, 29, 0, 0, 1, 0, None) == -1
