"""Inputs whose sums round, and the two mutants they are meant to catch.  Plain NumPy, no GPU (tests/test_inexact_host.py,
tests/test_gpu_inexact.py; the cases themselves: tests/inexact_cases.py).

The decoder promises the reference's bits: every candidate is fl(delta[i] + A[j][i]), the target takes the maximum, the emission
is added last -- fl(fl(d + A) + E) -- and the back-trace recomputes fl(d + A[j][i]) and takes the lowest index attaining the
maximum.  On a dyadic grid with small magnitudes every one of those additions is exact, so a kernel that associates differently
((A + E) + d), or a back-trace that compares after the emission add, returns the same bits.  The generators of the geometry tests
are on such grids.  This module moves them off it:

  off_grid            one value -> one value over the whole array, v - k(v) 2^-bits: equalities and the order of values survive, so
                      the plan analysis classifies the twin like the original (row constants, windows, extra columns, step bands);
  off_grid_emissions  an independent offset per element;
  logprob_*           log of row-normalised random probabilities, for the unstructured dense kernels.

bits = 20: a float32 sum keeps a multiple of 2^-20 only below 16, and at T = 131 the running sums of the cases reach 2^6 .. 2^9, where
one ulp is 2^-17 .. 2^-14: the offsets lie below it for most of a song, so rounding creates ties between candidates that differ on
paper and breaks ties between candidates that are equal on paper.  (A value whose k is 0 stays on the grid; where that is the
floor of a banded matrix -- most of its entries -- the share of sums that round falls below one half, and the case takes another
seed: inexact_cases.RESEED.)

forward_reassociated and backtrace_reassociated are the reference recursion with one association changed each; premise_rounds and
premise_mutants measure, on the reference alone, whether an input can tell them from the real thing."""
import numpy as np

F32 = np.float32


def off_grid(X, rng, bits=20, kmax=8):
    """v -> fl32(v - k(v) 2^-bits) with one random integer k(v) in [0, kmax) per distinct value of the WHOLE array; -inf stays -inf.
    Asserts that distinct values stay distinct and in order."""
    X = np.asarray(X, F32)
    vals, inv = np.unique(X, return_inverse=True)
    k = rng.integers(0, kmax, len(vals))
    new = (vals.astype(np.float64) - k * 2.0 ** -bits).astype(F32)
    assert np.all(np.diff(new) > 0), "two values of the array are closer than the offsets"
    assert np.array_equal(np.isneginf(new), np.isneginf(vals))
    return np.ascontiguousarray(new[inv.reshape(-1)].reshape(X.shape))


def off_grid_emissions(E, rng, bits=20, kmax=8):
    """E - k 2^-bits with an independent k in [0, kmax) per element, rounded once to float32; -inf stays -inf."""
    E = np.asarray(E, F32)
    k = rng.integers(0, kmax, E.shape)
    return np.ascontiguousarray((E.astype(np.float64) - k * 2.0 ** -bits).astype(F32))


def stored(E32, f16):
    """What the oracle sees and what the decoder gets for a storage type: (float32 values, float16 array or None)."""
    if not f16:
        return np.ascontiguousarray(E32, F32), None
    E16 = np.asarray(E32, F32).astype(np.float16)
    return E16.astype(F32), E16


def logprob_matrix(S, rng):
    """logA_T [target, source] float32: log of random transition probabilities, every source's row normalised, in float64, rounded
    once."""
    P = rng.random((S, S))
    P /= P.sum(axis=1, keepdims=True)                   # P[source, target]
    return np.ascontiguousarray(np.log(P).T.astype(F32))


def logprob_prior(S, rng):
    p = rng.random(S)
    return np.log(p / p.sum()).astype(F32)


def logprob_emissions(B, T, S, rng):
    """[B, T, S] float32: log of random probabilities normalised over the states of every frame, in float64, rounded once."""
    P = rng.random((B, T, S))
    P /= P.sum(axis=2, keepdims=True)
    return np.ascontiguousarray(np.log(P).astype(F32))


def ragged(B, T):
    """B song lengths: T, 1, a mid-length song, 2, 3, then a spread over T / 4 .. T - 1 -- the log-likelihoods sample the delta history
    at that many frames."""
    head = [T, 1, T // 2 + 1, 2, 3][:B]
    rest = np.linspace(T // 4, T - 1, B - len(head)).astype(np.int64).tolist() if B > len(head) else []
    return np.minimum(np.asarray(head + rest, np.int64), T)


# ---------------------------------------------------------------------------------------------------------------------
# The reference recursion and its two mutants, one song [n, S] each, float32 throughout
# ---------------------------------------------------------------------------------------------------------------------
def forward_reference(A, pi, E):
    """Delta rows [n, S]: d_0 = fl(pi + E_0), d_t[j] = fl(max_i fl(d_{t-1}[i] + A[j][i]) + E_t[j])."""
    A, E = np.asarray(A, F32), np.asarray(E, F32)
    rows = np.empty(E.shape, F32)
    rows[0] = np.asarray(pi, F32) + E[0]
    for t in range(1, len(E)):
        rows[t] = np.max(rows[t - 1][None, :] + A, axis=1) + E[t]
    return rows


def forward_reassociated(A, pi, E):
    """MUTANT: d_t[j] = max_i fl(d_{t-1}[i] + fl(A[j][i] + E_t[j])) -- the emission folded into the matrix entry first."""
    A, E = np.asarray(A, F32), np.asarray(E, F32)
    rows = np.empty(E.shape, F32)
    rows[0] = np.asarray(pi, F32) + E[0]
    for t in range(1, len(E)):
        rows[t] = np.max(rows[t - 1][None, :] + (A + E[t][:, None]), axis=1)
    return rows


def backtrace_reference(A, rows):
    """From the arg-max of the last row back: the LOWEST source index attaining max_i fl(d_{t-1}[i] + A[j][i]) -> (states, loglik)."""
    n = len(rows)
    path = np.empty(n, np.int64)
    s = int(np.argmax(rows[-1]))
    ll = rows[-1][s]
    path[-1] = s
    for t in range(n - 1, 0, -1):
        s = int(np.argmax(rows[t - 1] + A[s]))
        path[t - 1] = s
    return path, ll


def backtrace_reassociated(A, rows, E):
    """MUTANT on a correct history: the arg-max is taken over fl(d_{t-1}[i] + fl(A[j][i] + E_t[j])) -- compared after the emission
    add, where two candidates one ulp apart can round together and the lower index wins, or the other way round."""
    A, E = np.asarray(A, F32), np.asarray(E, F32)
    n = len(rows)
    path = np.empty(n, np.int64)
    s = int(np.argmax(rows[-1]))
    path[-1] = s
    for t in range(n - 1, 0, -1):
        s = int(np.argmax(rows[t - 1] + (A[s] + E[t, s])))
        path[t - 1] = s
    return path


def _songs(E, lens):
    E = np.asarray(E, F32)
    E = E[None] if E.ndim == 2 else E
    lens = np.full(len(E), E.shape[1], np.int64) if lens is None else np.asarray(lens, np.int64)
    return [(b, E[b, :int(lens[b])]) for b in range(len(E))]


def premise_rounds(A, pi, E, lens=None):
    """The share of the finite candidate sums d_{t-1}[i] + A[j][i] of the reference recursion (every frame, target and source of
    every song) whose float64 sum differs from the float32 sum."""
    A = np.asarray(A, F32)
    A64 = A.astype(np.float64)
    inexact = total = 0
    for _, Eb in _songs(E, lens):
        rows = forward_reference(A, pi, Eb)
        for t in range(1, len(Eb)):
            d = rows[t - 1]
            c32 = d[None, :] + A
            c64 = d.astype(np.float64)[None, :] + A64
            fin = np.isfinite(c64)
            inexact += int(np.count_nonzero(fin & (c32.astype(np.float64) != c64)))
            total += int(np.count_nonzero(fin))
    return inexact / total if total else 0.0


def premise_mutants(A, pi, E, lens=None):
    """-> (the forward mutant changes a state or a log-likelihood bit of some song, the number of states the back-trace mutant
    changes, (reference states per song, reference log-likelihoods))."""
    A = np.asarray(A, F32)
    forward_visible, changed, ref_s, ref_l = False, 0, [], []
    for _, Eb in _songs(E, lens):
        rows = forward_reference(A, pi, Eb)
        path, ll = backtrace_reference(A, rows)
        mpath, mll = backtrace_reference(A, forward_reassociated(A, pi, Eb))
        forward_visible |= bool(np.any(mpath != path)) or F32(mll).tobytes() != F32(ll).tobytes()
        changed += int(np.count_nonzero(backtrace_reassociated(A, rows, Eb) != path))
        ref_s.append(path)
        ref_l.append(ll)
    return forward_visible, changed, (ref_s, np.asarray(ref_l, F32))
