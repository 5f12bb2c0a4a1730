"""The split floor kernel's full-window waves store their four delta copies with ds_write_addtid_b32, whose byte address is
M0 + a 16-bit immediate + 4 * lane.  The host library replays the kernel's address rule (split_addtid_base / split_addtid_imm,
plan.hpp): for every full wave, lane, buffer, copy and win_shift the three terms must add up to the byte address of the float the
ds_write_b32 form writes -- wp[b * BUF + c * DC - c] with wp = dls + 4 + sh + j, what floor_lds_check.hip replays against the
readers -- and base and immediate must each fit the instruction's 16-bit fields."""
import ctypes
import itertools

import numpy as np

from tests import plan_replay

DC = 384 + 16            # FloorSplitLds: copy stride of the 384 state slots (banded_floor.inc)
BUF = 4 * DC             # floats per delta buffer
SEGMENT = 2 * BUF + 4 * 64 + 16 * 2   # two buffers, four slot groups, terminal scratch (FloorLds::end at W = 32)


def _addtid(lib, sh, wave, lane, b, c):
    out = np.zeros(3, np.int32)
    rc = lib.vph_split_addtid(sh, wave, lane, b, c, out.ctypes.data)
    return rc, int(out[0]), int(out[1]), int(out[2])


def _lib():
    lib = plan_replay._lib()
    lib.vph_split_addtid.restype = ctypes.c_int
    lib.vph_split_addtid.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p]
    return lib


def test_addtid_address_is_the_ds_write_b32_address():
    lib = _lib()
    seen = set()
    for sh, wave, b, c in itertools.product(range(4), range(4), range(2), range(4)):
        bases, imms = set(), set()
        for lane in range(64):
            rc, base, imm, pos = _addtid(lib, sh, wave, lane, b, c)
            assert rc == 0
            j = 64 * wave + lane
            # the ds_write_b32 form, by hand: own entry of copy 0, buffer b and copy c a constant further on
            assert pos == 4 + sh + j + b * BUF + c * DC - c, (sh, wave, lane, b, c)
            assert base + imm + 4 * lane == 4 * pos, (sh, wave, lane, b, c, base, imm, pos)
            assert 0 <= base < 65536 and 0 <= imm < 65536 and base + imm + 4 * lane + 4 <= 65536, (base, imm)
            # inside copy c of buffer b, and inside the segment
            assert b * BUF + c * DC <= pos < b * BUF + (c + 1) * DC and pos < SEGMENT, (sh, wave, lane, b, c, pos)
            bases.add(base)
            imms.add(imm)
            seen.add((sh, b, c, pos))
        assert len(bases) == 1 and len(imms) == 1, "base and immediate do not depend on the lane"
        assert base == 4 * (4 + sh + 64 * wave) and imm % 4 == 0
    # every (shift, buffer, copy) gets 256 distinct floats: no two lanes of the four waves write the same one
    assert len(seen) == 4 * 2 * 4 * 256


def test_immediate_depends_on_buffer_and_copy_only():
    lib = _lib()
    for b, c in itertools.product(range(2), range(4)):
        imms = {_addtid(lib, sh, wave, 0, b, c)[2] for sh in range(4) for wave in range(4)}
        assert imms == {4 * (b * BUF + c * DC - c)}
    for sh, wave in itertools.product(range(4), range(4)):
        assert {_addtid(lib, sh, wave, 0, b, c)[1] for b in range(2) for c in range(4)} == {4 * (4 + sh + 64 * wave)}


def test_arguments_out_of_range_are_refused():
    lib = _lib()
    for bad in ((4, 0, 0, 0, 0), (-1, 0, 0, 0, 0), (0, 4, 0, 0, 0), (0, 0, 64, 0, 0), (0, 0, 0, 2, 0), (0, 0, 0, 0, 4)):
        assert _addtid(lib, *bad)[0] == -1, bad
