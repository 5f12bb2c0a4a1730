"""The split floor kernel's frame loop, replayed on the CPU through the host plan library (vph_split_rounds, written with the
kernel's own round predicates split_round_interior / split_round_full / split_prefetch_row of plan.hpp).

Frames 1 .. Tb - 1 of a song run in rounds of PF unrolled frames and a tail of up to PF - 1.  Frame t requests the emission row
min(t + PF, Tb - 1).  The rounds all of whose requests stay inside the song ("interior") run a loop body that adds the constant
row offset and has no clamp, so for every song length:
  * the frames of all rounds and of the tail are exactly 1 .. Tb - 1, each once and in order;
  * frame t's request is row min(t + PF, Tb - 1) -- in an interior round that is what the UNCLAMPED sum must give, i.e. the body
    without a clamp never reads past row Tb - 1;
  * no frame of an interior round has a clamped row."""
import ctypes

import numpy as np
import pytest

from tests import plan_replay

INTERIOR, FULL, TAIL = 2, 1, 0
CAP = 256


def _lib():
    lib = plan_replay._lib()
    lib.vph_split_rounds.restype = ctypes.c_int
    lib.vph_split_rounds.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int]
    lib.vph_split_prefetch.restype = ctypes.c_int
    lib.vph_split_prefetch.argtypes = []
    return lib


def split_rounds(Tb, pf=0):
    """[(frame, requested emission row, class)] in loop order (pf = 0: the depth the kernel is instantiated with)."""
    lib = _lib()
    f, r, c = (np.full(CAP, -1, np.int32) for _ in range(3))
    n = lib.vph_split_rounds(Tb, pf, f.ctypes.data, r.ctypes.data, c.ctypes.data, CAP)
    assert 0 <= n <= CAP, (Tb, pf, n)
    return list(zip(f[:n].tolist(), r[:n].tolist(), c[:n].tolist()))


def round_classes(Tb, pf=0):
    """(interior rounds, clamped full rounds, tail frames) of a song of Tb frames."""
    PF = pf or _lib().vph_split_prefetch()
    cls = [c for _, _, c in split_rounds(Tb, pf)]
    assert cls.count(INTERIOR) % PF == 0 and cls.count(FULL) % PF == 0
    return cls.count(INTERIOR) // PF, cls.count(FULL) // PF, cls.count(TAIL)


def test_instantiated_depth():
    lib = _lib()
    assert lib.vph_split_prefetch() == 12           # the split kernel exists for W = 32 only: one prefetch depth
    assert split_rounds(50) == split_rounds(50, 12)


@pytest.mark.parametrize("PF", [4, 12])
def test_rounds_cover_the_song(PF):
    for Tb in range(1, 101):
        fr = split_rounds(Tb, PF)
        assert [f for f, _, _ in fr] == list(range(1, Tb)), (Tb, PF)
        for f, row, cls in fr:
            assert row == min(f + PF, Tb - 1), (Tb, PF, f, row, cls)
            if cls == INTERIOR:
                assert f + PF <= Tb - 1, (Tb, PF, f, "a clamped row in an interior round")
        # the classes come in loop order: interior rounds, clamped full rounds, the tail
        classes = [c for _, _, c in fr]
        assert classes == sorted(classes, reverse=True), (Tb, PF)
        ni, nf, nt = round_classes(Tb, PF)
        assert nt <= PF - 1 and ni * PF + nf * PF + nt == max(Tb - 1, 0)
        # every full round but the last is interior: nothing that could go without the clamp keeps it
        assert nf == (1 if Tb - 1 >= PF else 0) and ni == max((Tb - 1) // PF - 1, 0), (Tb, PF, ni, nf, nt)


def test_bad_arguments():
    lib = _lib()
    buf = np.zeros(4, np.int32)
    assert lib.vph_split_rounds(0, 12, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 4) == -1
    assert lib.vph_split_rounds(30, 5, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 4) == -1      # odd depth
    assert lib.vph_split_rounds(30, 12, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 4) == -1     # 29 frames, room for 4
