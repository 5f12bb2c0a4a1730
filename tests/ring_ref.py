"""Replay of an append schedule of a RING session on the NumPy reference (tests/commit_ref.py), for one recording: what a session
of R history rows that commits (and acknowledges the frontier it read) after every append does, and which ring events the
schedule exercises.  A plain helper module: no fixtures, no GPU.

Frame t lives in row t mod R.  For every append of ``counts[k]`` frames (0 allowed) the replay records

    n0, n       frames before and after the append
    f0, f       the frontier before the append (= the acknowledged one) and after the commit that follows it
    states      the committed states of frames [f0, f) (int32)
    resident    n - f0 <= R: the append overwrites no row of [f0, n0) -- the session accepts it
    wraps       frames t in [n0, n), t > 0, with t mod R == 0: how often the append's stores pass from slot R - 1 to slot 0
    slot0       the append starts exactly at a slot 0 beyond frame 0 (n0 > 0, n0 mod R == 0): its first frame stores the frame maximum
                into slot R - 1 and its row into slot 0, and it resumes from slot R - 1
    range_straddle   the committed range [f0, f) holds frames on both sides of a slot R - 1 -> 0 step
    walk_straddle    the merge walk (rows n - 2 down to the merge frame f - 1, or to the stop frame where nothing merged) does

The frontier of the reference IS the device frontier, so ``resident`` is exactly the residency rule of vit_stream_append for a
caller that acknowledges every frontier it reads."""
import numpy as np

from tests import commit_ref as cr


def replay(psi, counts, R, L):
    """-> list of dicts, one per append (see the module docstring).  psi: commit_ref.back_pointers of the whole recording."""
    R, L = int(R), int(L)
    out = []
    n = f = 0
    for c in counts:
        c = int(c)
        n0, f0 = n, f
        n = n0 + c
        f, st = cr.commit(psi, n, f0, L)
        wraps = sum(1 for t in range(max(n0, 1), n) if t % R == 0)
        lo_walk = f - 1 if f > f0 else max(f0, n - 1 - L)          # the lowest row the merge walk reads
        walked = n >= 2 and lo_walk <= n - 2
        out.append(dict(n0=n0, n=n, f0=f0, f=f, states=st, resident=n - f0 <= R, wraps=wraps,
                        slot0=c > 0 and n0 > 0 and n0 % R == 0,
                        range_straddle=f > f0 and f0 // R != (f - 1) // R,
                        walk_straddle=walked and lo_walk // R != (n - 2) // R))
    return out


def summary(steps):
    """The conditions a parity test puts on its schedule, over one replay."""
    return dict(resident=all(s["resident"] for s in steps), wraps=sum(s["wraps"] for s in steps),
                slot0=sum(s["slot0"] for s in steps), range_straddle=sum(s["range_straddle"] for s in steps),
                walk_straddle=sum(s["walk_straddle"] for s in steps),
                stall_then_commit=_stall_then_commit(steps))


def _stall_then_commit(steps):
    """a commit that finds nothing (with more than 33 frames appended) followed later by one that commits"""
    stalls = [i for i, s in enumerate(steps) if s["n"] > 33 and s["n"] > s["n0"] and s["f"] == s["f0"]]
    return bool(stalls) and any(s["f"] > s["f0"] for s in steps[stalls[0] + 1:])


def smallest_ring(psis, counts_per_recording, L, candidates=(128, 192, 256)):
    """The smallest R of `candidates` for which every recording's replay is resident throughout; None if none is."""
    for R in candidates:
        if all(summary(replay(p, c, R, L))["resident"] for p, c in zip(psis, counts_per_recording)):
            return R
    return None
