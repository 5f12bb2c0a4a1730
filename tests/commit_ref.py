"""NumPy reference of the commit point of a streaming session (include/viterbi_hip.h vit_stream_commit).

float32, ``np.argmax`` back-pointers as in ``oracle/viterbi_oracle.py decode_numpy`` (lowest index among equal values, index 0 for
an all -inf frame), then the survivor walk with the frontier ``f`` and the lookback ``L``:

    U_{n-1} = all S states, U_{t-1} = psi_t[U_t]
    c = the LARGEST t with max(f, n-1-L) <= t <= n-2 and |U_t| = 1, s_c its element
    c exists:  f' = c + 1, states[f .. c] = s_c at frame c, s_{t-1} = psi_t[s_t] below it
    otherwise (or n < 2):  f' = f, nothing written

psi_t is a function of the frames before t only, so the back-pointers of a whole recording serve every prefix of it."""
import numpy as np


def back_pointers(logA_T, log_pi, logE):
    """psi int32 [T, S] of one recording logE [T, S] (row 0 unused: zeros)."""
    logA_T = np.ascontiguousarray(logA_T, np.float32)
    logE = np.ascontiguousarray(logE, np.float32)
    T, S = logE.shape
    psi = np.zeros((T, S), np.int32)
    delta = (np.asarray(log_pi, np.float32) + logE[0]).astype(np.float32)
    scratch = np.empty((S, S), np.float32)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            np.add(delta, logA_T, out=scratch)
            arg = np.argmax(scratch, axis=1)
            psi[t] = arg
            delta = (scratch[np.arange(S), arg] + logE[t]).astype(np.float32)
    return psi


def commit(psi, n, f, L):
    """One commit of a recording of n frames with f committed: -> (f', states of frames [f, f') as int32)."""
    n, f, L = int(n), int(f), int(L)
    assert L >= 1 and 0 <= f
    empty = np.zeros(0, np.int32)
    if n < 2:
        return f, empty
    S = psi.shape[1]
    t_stop = max(f, n - 1 - L)
    U = np.arange(S)
    for t in range(n - 2, t_stop - 1, -1):
        U = np.unique(psi[t + 1][U])
        if len(U) == 1:
            out = np.empty(t - f + 1, np.int32)
            s = int(U[0])
            out[t - f] = s
            for u in range(t - 1, f - 1, -1):
                s = int(psi[u + 1][s])
                out[u - f] = s
            return t + 1, out
    return f, empty


def walk(psi, lengths_after_each_append, L, f=0):
    """The commits after each append of one recording: a list of (n, f before, f after, states [f before, f after))."""
    out = []
    for n in lengths_after_each_append:
        f2, st = commit(psi, n, f, L)
        out.append((int(n), f, f2, st))
        f = f2
    return out
