"""Guarded, poisoned buffers for the tests that ask where a call writes (tests/test_guarded_host.py, tests/test_gpu_bounds.py).  A plain
helper module: no fixtures, no GPU needed (an Arena lives on whatever device it is given; the host tier builds its arenas on the CPU).

* Arena: one uint8 tensor ``guard | pad to align | lead | payload | pad | guard`` filled with one byte.  The default 0xFF reads as NaN
  in float32 and float16 and as -1 in int32, so that whatever a kernel takes from outside its buffer poisons its result, and
  ``intact()`` finds every byte outside the payload that a call changed.
* poison_states: what a ``states`` buffer holds BEFORE a decode: a sentinel, valid-looking wrong states, or another decode's path.
* assert_decode_outputs: states and log-likelihoods against the oracle by bits, -1 past a song's end, both arenas intact; the
  message names the first offending (song, frame).

Only the first and the last byte of a buffer are fenced this way.  What a call does BETWEEN the regions inside its workspace is out
of reach of this harness."""
import numpy as np
import torch

FILL = 0xFF
GUARD = 1 << 16            # far more than any row prefetch of the kernels: a stray read stays inside the allocation
SENTINEL = -7
KINDS = ("sentinel", "shifted", "neighbour")


class Arena:
    """``nbytes`` of payload between two guards.  The payload starts ``lead`` bytes past an ``align``-byte boundary (lead = one
    element puts a tensor one element past a 256-byte boundary: element alignment and nothing more)."""

    def __init__(self, nbytes, device, fill=FILL, align=256, guard=GUARD, lead=0):
        nbytes, align, guard, lead = int(nbytes), int(align), int(guard), int(lead)
        assert nbytes >= 0 and align >= 1 and guard >= 0 and 0 <= lead and 0 <= fill <= 0xFF
        self.nbytes, self.fill, self.align, self.guard, self.lead = nbytes, int(fill), align, guard, lead
        self.buf = torch.full((guard + align + lead + nbytes + align + guard,), self.fill, dtype=torch.uint8, device=device)
        self.offset = guard + (-(self.buf.data_ptr() + guard)) % align + lead
        self.payload = self.buf[self.offset:self.offset + nbytes]
        assert self.payload.numel() == nbytes and (self.payload.data_ptr() - lead) % align == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.offset

    def view(self, dtype, shape):
        """The payload as a contiguous tensor of ``dtype`` and ``shape`` (it must fill the payload exactly)."""
        item = torch.empty((), dtype=dtype).element_size()
        assert self.ptr % item == 0, "the payload is not aligned for this element type"
        assert int(np.prod(shape, dtype=np.int64)) * item == self.nbytes, (tuple(shape), dtype, self.nbytes)
        return self.payload.view(dtype).view(tuple(shape))

    def store(self, array):
        """Copy a host array (or a tensor) of exactly the payload's size into the payload; returns the typed view."""
        t = array if isinstance(array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(array))
        v = self.view(t.dtype, tuple(t.shape))
        v.copy_(t)
        return v

    def poisoned(self):
        """True while every byte of the payload still holds the fill byte."""
        return bool((self.payload == self.fill).all())

    def intact(self):
        """(front_ok, back_ok, first_bad_offset): every byte outside the payload -- guards, pads and lead -- against the fill byte.
        first_bad_offset is relative to the payload's first byte (negative in front of it, >= nbytes behind it), None when intact."""
        front, back = self.buf[:self.offset], self.buf[self.offset + self.nbytes:]
        bad_f, bad_b = front != self.fill, back != self.fill
        front_ok, back_ok = not bool(bad_f.any()), not bool(bad_b.any())
        first = None
        if not front_ok:
            first = int(torch.nonzero(bad_f)[0, 0]) - self.offset
        elif not back_ok:
            first = self.nbytes + int(torch.nonzero(bad_b)[0, 0])
        return front_ok, back_ok, first


def assert_intact(arena, name):
    front_ok, back_ok, first = arena.intact()
    assert front_ok, f"{name}: bytes in front of the buffer were written (first at offset {first} from its start)"
    assert back_ok, f"{name}: bytes behind the buffer were written (first at offset {first}, the buffer holds {arena.nbytes} bytes)"


def _lengths_of(ref_states):
    ref = np.asarray(ref_states)
    assert ref.ndim == 2
    lens = (ref >= 0).sum(axis=1)
    for b, n in enumerate(lens):
        assert np.all(ref[b, :n] >= 0) and np.all(ref[b, n:] == -1), f"song {b}: the reference is not a path followed by -1"
    return lens


def poison_states(ref_states, S, kind, neighbour=None):
    """What ``states`` holds before a decode whose right answer is ``ref_states`` ([B, T] int32, -1 past a song's end) -> int32 [B, T].
    "sentinel": -7 everywhere.  "shifted": (ref + 1 + t % 3) % S -- valid-looking states, wrong at every frame.  "neighbour":
    ``neighbour``, the oracle's path of the same songs (the same lengths) under emissions of another seed -- a plausible, locally
    continuous, wrong path; past a song's end, where it would hold the right -1, it holds the sentinel."""
    ref = np.ascontiguousarray(ref_states, np.int32)
    assert ref.ndim == 2 and kind in KINDS, kind
    B, T = ref.shape
    if kind == "sentinel":
        out = np.full((B, T), SENTINEL, np.int32)
    elif kind == "shifted":
        out = ((ref.astype(np.int64) + 1 + (np.arange(T, dtype=np.int64) % 3)[None, :]) % S).astype(np.int32)
        assert np.all(out >= 0) and np.all(out < S)
    else:
        assert neighbour is not None, "the neighbour kind needs the other decode's path"
        nb = np.ascontiguousarray(neighbour, np.int32)
        lens = _lengths_of(ref)
        assert nb.shape == ref.shape and np.array_equal(_lengths_of(nb), lens), "the neighbour path is not one of the same songs"
        out = np.where(nb < 0, np.int32(SENTINEL), nb).astype(np.int32)
        for b, n in enumerate(lens):
            if n > 8:
                differ = int(np.sum(out[b, :n] != ref[b, :n]))
                assert 2 * differ >= n, f"song {b}: the neighbour path differs from the reference in only {differ} of {n} frames"
    if kind != "neighbour":
        assert np.all(out != ref), f"{kind}: the poison equals the right answer in {int(np.sum(out == ref))} entries"
    return out


def _bits(x):
    a = np.ascontiguousarray(x)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_decode_outputs(states_arena, loglik_arena, ref_s, ref_l, lens, T, offsets=None):
    """The outputs of one decode against the oracle.  Padded ([B, T] states; ``offsets`` None): bit equality on [b, :len_b], exactly -1
    on [b, len_b:T].  Packed (``offsets`` = B + 1 frame offsets, states [offsets[B]]; T is ignored): bit equality, no -1 anywhere.
    The log-likelihoods (float32, or float64 where ``ref_l`` is) by bits; both arenas intact.  Names the first offending (song,
    frame)."""
    lens = np.asarray(lens, np.int64)
    B = len(lens)
    ref_s = np.asarray(ref_s)
    ll_dtype = torch.float64 if np.asarray(ref_l).dtype == np.float64 else torch.float32
    ref_l = np.ascontiguousarray(ref_l, np.float64 if ll_dtype == torch.float64 else np.float32)
    assert_intact(states_arena, "states")
    assert_intact(loglik_arena, "loglik")
    if offsets is None:
        st = states_arena.view(torch.int32, (B, T)).cpu().numpy()
        rows = [(st[b], int(lens[b])) for b in range(B)]
    else:
        off = np.asarray(offsets, np.int64)
        assert off.shape == (B + 1,) and np.array_equal(np.diff(off), lens)
        st = states_arena.view(torch.int32, (int(off[-1]),)).cpu().numpy()
        rows = [(st[off[b]:off[b + 1]], int(lens[b])) for b in range(B)]
    for b, (row, n) in enumerate(rows):
        want = ref_s[b, :n]
        bad = np.nonzero(row[:n] != want)[0]
        assert bad.size == 0, (f"states differ from the oracle at song {b}, frame {int(bad[0])} (of {n}): got {int(row[bad[0]])}, "
                               f"want {int(want[bad[0]])}; {bad.size} frames of this song differ")
        tail = np.nonzero(row[n:] != -1)[0]
        assert tail.size == 0, (f"states past the end of song {b} ({n} frames) are not -1: frame {n + int(tail[0])} holds "
                                f"{int(row[n + tail[0]])}; {tail.size} such frames")
    ll = loglik_arena.view(ll_dtype, (B,)).cpu().numpy()
    bad = np.nonzero(_bits(ll) != _bits(ref_l))[0]
    assert bad.size == 0, f"loglik differs from the oracle at song {int(bad[0])}: got {ll[bad[0]]!r}, want {ref_l[bad[0]]!r}"
