"""What the streaming-session tiers share (tests/test_stream_grid_host.py, tests/test_gpu_stream_grid.py): which plans a session
serves, as literal tables; the append schedules and what they promise about launch boundaries, checked on the host; the chunk
counts the library's formulas give; and the feeding of a session from one padded tensor.  NumPy only -- `nan_rows`, `feed` and
`plan_case` take torch tensors and import what they need when they are called.

A schedule is a list of appends (n, counts): every recording b takes rows [b, :counts[b]] of a [B, n, S] chunk whose other rows
are NaN (a row the kernel must not read).  `segments`, `odd` and `staggered` are described at `schedule`."""
import numpy as np

from tests import floor_grid as fg

# (W, NWT) of banded_floor_forward_kernel<.., WgVariant::Stream> a session runs: every reachable pair of the floor form
# (kernels.hpp floor_stream_applies = floor_packed_applies; capi.hip st_family adds a back-trace over the rows, which every grid
# plan has).  Literal on purpose: the host tier holds it against the grid and against vit_workspace_bytes_stream.
STREAM_SERVED = {(16, 2), (16, 4), (16, 6), (16, 8), (16, 12), (32, 2), (32, 4), (32, 6), (32, 8), (32, 12),
                 (64, 4), (64, 6), (64, 8), (64, 12), (84, 4), (84, 6), (84, 8), (84, 12),
                 (96, 4), (96, 6), (96, 8), (96, 12), (128, 6), (128, 8), (128, 12)}
# voiced states n of the Durrieu geometry (20-bin bands, nine near bands; S = n + 1) -> a session is served (step4s_forward_kernel<..,
# WgVariant::Stream>, kernels.hpp step_kernel_instantiated: 704 < n <= 768)
STEP_SERVED = {704: False, 705: True, 706: True, 709: True, 768: True, 769: False}
# tests/floor_grid.py WAVE_FORM_SEEDS -> a session is served.  These plans have the wave form, which st_family does not ask about: a
# session runs the workgroup family whatever else the plan has.  All of them: floor-proven, no dense rows, W = 16 or 32 on six waves.
WAVE_SEED_SERVED = {0: True, 2: True, 3: True, 4: True, 5: True, 6: True, 7: True, 8: True, 9: True}

T_CAP = fg.T + 7                       # rows per recording of a grid session: above the longest length, so hist_rows != the frames walked
SCHEDULES = ("segments", "odd", "staggered", "skewed")
ODD_HEAD = (1, 1, 2, 3, 5, 7, 12, 13, 19)      # 63 frames: below, at and above the prefetch depths 2, 4 and 12, every unroll remainder
BOUNDARIES = (64, 128, 192)            # the frames floor_grid.emissions_hops forces a hop into


def chunked(lens, sizes):
    """Appends of `sizes` frames, each recording taking min(n, what it has left); appends nobody takes part in are left out."""
    lens = np.asarray(lens, np.int64)
    pos = np.zeros_like(lens)
    out = []
    for n in sizes:
        cnt = np.minimum(n, lens - pos)
        if cnt.max() > 0:
            out.append((int(n), cnt))
        pos = pos + cnt
    assert np.array_equal(pos, lens), "the schedule does not feed every frame"
    return out


def schedule(name, lens, T):
    """segments:  64 frames an append: a launch starts at frames 64, 128 and 192 of every recording that reaches them.
    odd:       1, 1, 2, 3, 5, 7, 12, 13, 19 (ending at frame 63), 1, 1 (launches start at frames 64 and 65), the rest 37 an append.
    staggered: 37 frames an append, recording b sits out the first b % 3 of them: the recordings of one launch stand at different
               positions (the per-launch tables); every recording's own boundaries are still the multiples of 37.
    skewed:    37 frames an append, but 37 - 7 (b % 3) for recording b in the first: different positions in every launch AND launch
               boundaries on different frames for different recordings."""
    lens = np.asarray(lens, np.int64)
    assert int(lens.max()) == T
    if name == "segments":
        return chunked(lens, [min(64, T - t) for t in range(0, T, 64)])
    if name == "odd":
        head = list(ODD_HEAD) + [1, 1]
        assert sum(ODD_HEAD) == 63 and sum(head) < T
        return chunked(lens, head + [min(37, T - t) for t in range(sum(head), T, 37)])
    assert name in ("staggered", "skewed")
    pos = np.zeros_like(lens)
    out = []
    k = 0
    r = np.arange(len(lens)) % 3
    while (pos < lens).any():
        if name == "staggered":
            cnt = np.where(r > k, 0, np.minimum(37, lens - pos))
        else:
            cnt = np.minimum(37 - 7 * r if k == 0 else 37, lens - pos)
        out.append((37, cnt))
        pos = pos + cnt
        k += 1
    return out


def launch_starts(sched, B):
    """Per recording, the frames at which one of its launches starts (appends it takes no frame of start nothing)."""
    pos = np.zeros(B, np.int64)
    starts = [set() for _ in range(B)]
    for n, cnt in sched:
        assert cnt.shape == (B,) and cnt.min() >= 0 and cnt.max() <= n
        for b in range(B):
            if cnt[b] > 0:
                starts[b].add(int(pos[b]))
        pos += cnt
    return starts, pos


def uniform_launches(sched, B):
    """Per append, what vit_stream_append calls uniform: every recording at the same position, taking the same count (two
    scalars instead of the per-launch tables)."""
    pos = np.zeros(B, np.int64)
    out = []
    for n, cnt in sched:
        out.append(bool((cnt == cnt[0]).all() and (pos == pos[0]).all()))
        pos += cnt
    return out


def premise_schedule(name, sched, lens):
    """What the schedule is for, on the host: it feeds every frame; `segments` starts a launch exactly at each of BOUNDARIES in
    every recording that reaches the frame; `odd` at 63 .. 65; `staggered` has launches that are not uniform and boundaries that
    differ between recordings."""
    lens = np.asarray(lens, np.int64)
    starts, pos = launch_starts(sched, len(lens))
    assert np.array_equal(pos, lens), name
    if name == "segments":
        for b, L in enumerate(lens):
            for t in BOUNDARIES:
                assert (t in starts[b]) == (L > t), (name, b, int(L), t)
    elif name == "odd":
        for b, L in enumerate(lens):
            for t in (1, 2, 4, 7, 12, 19, 31, 44, 63, 64, 65):
                assert (t in starts[b]) == (L > t), (name, b, int(L), t)
    else:
        assert not all(uniform_launches(sched, len(lens))), (name, "every launch is uniform")
        assert any(len(set(int(p) for p in row)) > 1 for row in _positions(sched, len(lens))), (name, "equal positions in every launch")
        if name == "skewed":        # (staggered delays whole appends: its boundaries are the multiples of 37 in every recording)
            long = [b for b, L in enumerate(lens) if L > 2 * 37]
            inner = {frozenset(t for t in starts[b] if 0 < t <= 2 * 37) for b in long}
            assert len(inner) >= 2, (name, "the recordings share their launch boundaries")


def _positions(sched, B):
    pos = np.zeros(B, np.int64)
    for n, cnt in sched:
        yield pos[cnt > 0].copy()
        pos += cnt


# ---------------------------------------------------------------------------------------------------------------------
# The chunk counts of a session's back-trace, restated from the sources (the host tier reads the constants and the divisors there)
# ---------------------------------------------------------------------------------------------------------------------
def sparse_chunks(B, T, n_cus, warm_sparse=64, max_chunks=32):          # backtrace_sparse.hip sparse_backtrace_chunks
    c = 16 * (n_cus if n_cus > 0 else 256) // max(B, 1)
    return max(1, min(c, max(T // (8 * warm_sparse), 1), max_chunks))


def lazy_chunks(B, T, warm=128, max_chunks=32):                         # backtrace_rows.hip backtrace_chunks
    c = (2 * 1024 + B - 1) // max(B, 1)
    return max(1, min(c, max(T // (8 * warm), 1), max_chunks))


def lane_chunks(B, T, n_cus, warm=64, max_chunks=256):                  # backtrace_lane.hip lane_backtrace_chunks
    c = 16 * 64 * (n_cus if n_cus > 0 else 256) // max(B, 1)
    return max(1, min(c, max(T // (2 * max(warm, 1)), 1), max_chunks))


# the shapes of the two long sessions of the GPU tier: (plan, B, lengths, rows per recording, frames an append)
LONG_LENGTHS = (2304, 1100)
LONG_T_CAP = 2400
LONG_APPEND = 768                      # reference_api.RecordingAccumulator hands its frames over 768 at a time
LONG_CHUNKS = {"sparse": 4, "lane": 18, "lazy": 2}


# ---------------------------------------------------------------------------------------------------------------------
# Feeding a session (torch)
# ---------------------------------------------------------------------------------------------------------------------
def nan_rows(E, lens):
    """E [B, T, S] on the device -> [B, T + 1, S]: NaN behind every length and in row T."""
    import torch
    B, T, S = E.shape
    out = torch.full((B, T + 1, S), float("nan"), dtype=E.dtype, device=E.device)
    for b, L in enumerate(lens):
        out[b, :int(L)] = E[b, :int(L)]
    return out


def feed(st, En, sched, first=0, upto=None):
    """Appends `first` .. `upto` - 1 of `sched` (default: all) from En = nan_rows(E, lens): recording b's rows pos[b] .. pos[b] +
    counts[b] - 1, NaN in every other row of the chunk.  The session stands where the appends before `first` leave it."""
    import torch
    B, T1, S = En.shape
    dev = En.device
    pos = np.zeros(B, np.int64)
    for n, cnt in sched[:first]:
        pos += cnt
    assert np.array_equal(st.lengths, pos)
    rows = torch.arange(B, device=dev)[:, None]
    for n, cnt in sched[first:upto]:
        k = np.arange(n)[None, :]
        idx = np.where(k < cnt[:, None], pos[:, None] + k, T1 - 1)        # (row T: NaN)
        st.append(En[rows, torch.from_numpy(idx).to(dev)].contiguous(), counts=cnt)
        pos += cnt
    return pos


# ---------------------------------------------------------------------------------------------------------------------
# One grid plan's decoder, inputs and oracle answers, shared by the GPU tiers that walk floor_grid.GRID
# ---------------------------------------------------------------------------------------------------------------------
_plan_cache = {}


def plan_case(dev, entry):
    """decoder and, per batch, (name, emissions float32 on the fp16 grid, lengths, the oracle's states and log-likelihoods): built once
    per plan and left unchanged.  With it a dict for whatever further oracle answers a module wants to keep beside them."""
    import torch  # noqa: F401
    from oracle import viterbi_oracle as vo
    from tests.plan_replay import HostPlan
    from viterbi_spl_amd import ViterbiDecoder
    if entry not in _plan_cache:
        _plan_cache.clear()                          # one plan at a time: the parametrisations walk plan by plan
        W, n, S, half, recipe = entry
        A, pi = fg.plan_params(entry)
        hp = HostPlan(A, pi)
        dec = ViterbiDecoder(A, pi, dev)
        info = dec.info
        assert info["banded_ok"] and info["floor_ok"] and not info["wave_ok"] and info["n_dense_rows"] == 0, info
        assert info["group_window"] == W and fg.waves_for(S) == n and S < 64 * n and info["extras"] == hp.extras, info
        batches = []
        for name, E, lens in fg.plan_batches(entry, A, hp.lo[:S], hp.extras):
            ref_s, ref_l = vo.decode_c(A, pi, E, lengths=lens)
            for x in (E, lens, ref_s, ref_l):
                x.setflags(write=False)
            batches.append((name, E, lens, ref_s, ref_l))
        fg.premise_forced(batches[1][3][-1], W, hp.lo[:S], hp.extras[0] if hp.extras else None)
        fg.premise_hops(batches[2][3], batches[2][2], W, hp.lo[:S], hp.extras)
        _plan_cache[entry] = (dec, batches, {"A": A, "pi": pi})
    return _plan_cache[entry]
