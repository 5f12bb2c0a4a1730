"""NumPy restatement of the reference's float64 Viterbi variant (dcnet/tf_viterbi_decoding.py:209-263) on the library's inputs, a
host replay of the float64 floor form driven by the plan's own tables, and the inputs of the golden manifest's f64 cases.
Test infrastructure for tests/test_f64_host.py and tests/test_gpu_f64.py."""
import numpy as np
import torch

from viterbi_spl_amd import synth

TINY = np.finfo(np.float32).tiny


def decode_f64(logA_T, log_pi, logE, all_rows=False):
    """float32 logA_T [S, S] (row j = into target j), log_pi [S], logE [T, S]; only T1 is float64:
        d_0 = f64(fl32(log_pi + E_0));  d_t[j] = fl64(max_i fl64(d_{t-1}[i] + f64(A[j][i])) + f64(E_t[j])),  psi = LOWEST argmax.
    -> (states int64 [T], last d row float64 [S]) or, with all_rows, (states, last d row, d rows [T, S])."""
    A = np.ascontiguousarray(logA_T, np.float32).astype(np.float64)
    pi = np.ascontiguousarray(log_pi, np.float32)
    E = np.ascontiguousarray(logE, np.float32)
    T, S = E.shape
    ar = np.arange(S)
    psi = np.empty((T, S), np.int32)
    rows = np.empty((T, S), np.float64) if all_rows else None
    with np.errstate(invalid="ignore", over="ignore"):
        d = (pi + E[0]).astype(np.float32).astype(np.float64)      # the reference adds two float32 arrays, THEN stores into T1
        if all_rows:
            rows[0] = d
        for t in range(1, T):
            c = d[None, :] + A
            i = np.argmax(c, axis=1)
            psi[t] = i
            d = c[ar, i] + E[t].astype(np.float64)
            if all_rows:
                rows[t] = d
    s = int(np.argmax(d))
    states = np.empty(T, np.int64)
    states[T - 1] = s
    for t in range(T - 2, -1, -1):
        s = int(psi[t + 1, s])
        states[t] = s
    return (states, d, rows) if all_rows else (states, d)


def decode_f64_batch(logA_T, log_pi, E, lens):
    """The restatement song by song -> (states int64 [B, T] with -1 past a song's end, loglik float64 [B])."""
    B, T, _ = E.shape
    st = np.full((B, T), -1, np.int64)
    ll = np.empty(B, np.float64)
    for b in range(B):
        n = int(lens[b])
        s, d = decode_f64(logA_T, log_pi, E[b, :n])
        st[b, :n] = s
        ll[b] = d[s[-1]]
    return st, ll


def replay_floor_f64(plan, logE):
    """Follows f64.hip on the host, driven by the plan's own tables (tests/plan_replay.py: HostPlan).
    Forward: per target the max of the W window sums, of fl64(M + c_j) with M the max of d over the NON-EXTRA sources, and of the
    extra-column sums, all in float64; every d row and every M is kept.  Back-trace: for the path state j at t + 1 the window and
    extra-column candidates; fl64(M_t + c_j) below their max -> the lowest matching source, else all S candidates and the lowest
    index attaining the max.  -> (states int64 [T], loglik, d rows [T, S])."""
    assert plan.ok and plan.floor_ok and plan.n_dense == 0
    S, W = plan.S, plan.W
    E = np.ascontiguousarray(logE, np.float32)
    T = E.shape[0]
    lo = plan.lo[:S].astype(np.int64)
    rowc = plan.rowc[:S].astype(np.float64)
    win_idx = lo[:, None] + np.arange(W)[None, :]
    tab = plan.tabA[:, :S].T.astype(np.float64)                    # [S, W]
    xa = plan.extraA[:, :S].astype(np.float64)
    masked = np.zeros(S, bool)
    masked[plan.extras] = True
    ar = np.arange(S)
    hist = np.empty((T, S), np.float64)
    M = np.empty(T, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (plan.log_pi[:S] + E[0]).astype(np.float32).astype(np.float64)
        hist[0] = d
        for t in range(1, T):
            M[t - 1] = np.max(np.where(masked, -np.inf, d))
            m = np.maximum(np.max(d[win_idx] + tab, axis=1), M[t - 1] + rowc)
            for k, x in enumerate(plan.extras):
                m = np.maximum(m, d[x] + xa[k])
            d = m + E[t].astype(np.float64)
            hist[t] = d
        M[T - 1] = np.max(np.where(masked, -np.inf, d))
        s = int(np.argmax(d))
        loglik = d[s]
        path = np.empty(T, np.int64)
        path[-1] = s
        for t in range(T - 2, -1, -1):
            dt, j = hist[t], s
            cand_i = list(range(lo[j], lo[j] + W)) + list(plan.extras)
            cand_v = [dt[lo[j] + w] + tab[j, w] for w in range(W)] + [dt[x] + xa[k, j] for k, x in enumerate(plan.extras)]
            m = max(cand_v)
            if M[t] + rowc[j] < m:
                s = min(i for i, v in zip(cand_i, cand_v) if v == m)
            else:
                excl = masked | ((ar >= lo[j]) & (ar < lo[j] + W))
                vf = np.where(excl, -np.inf, dt + rowc[j])
                mm = max(m, np.max(vf))
                idx = [i for i, v in zip(cand_i, cand_v) if v == mm] + [int(i) for i in np.nonzero((vf == mm) & ~excl)[0]]
                s = min(idx) if idx else 0
            path[t] = s
    return path, loglik, hist


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def manifest_case_probs(c):
    """probs_st [321, T] float32 (Fortran order) of one f64 case of the golden manifest, as tests/golden/make_goldens.py built it."""
    T = c["T"]
    rows = torch.arange(321, dtype=torch.int64)
    cols = torch.arange(T, dtype=torch.int64)
    h = synth._cell_hash(synth._mix32(rows ^ c["seed"]), cols)
    if c["dense"]:
        p = ((h % 4093) + 1).to(torch.float64)
        return np.asfortranarray((p / p.sum(dim=0, keepdim=True)).to(torch.float32).numpy())
    return np.asfortranarray(((h % 4096).to(torch.float32) / 4096.0).numpy())


def manifest_log_inputs(golden, c):
    """(logA_T, log_pi, logE [T, 321]) float32: np.log(x + tiny) of the msnet parameters and of the case's probabilities, exactly as
    the reference's function forms them (np.log of float32 stays float32)."""
    A, pi = golden["params"]["msnet321_A"], golden["params"]["msnet321_pi"]
    probs_st = manifest_case_probs(c)
    logA_T = np.require(np.log(A.T + TINY), np.float32, ["C"])
    log_pi = np.log(pi + TINY).astype(np.float32)
    logE = np.require(np.log(probs_st.T + TINY), np.float32, ["C"])
    assert logA_T.dtype == np.float32 and logE.dtype == np.float32
    return logA_T, log_pi, logE


def band_params(S, half):
    """synth's band recipe: band +/- half over S - 1 bins, the unvoiced state last -> (logA_T, log_pi) float32."""
    return synth.log_params(synth.tonet_transition(S - 1, half), synth.floored_prior(S))
