"""The split-window floor forward kernel (forward_form 6) with the half waves' partner lanes half a DPP row apart (lanes l and l ^ 8
share a target, joined by one DPP maximum) and, where the extra column leaves M by address, the frame maximum in three slots with
delta[x] in the fourth: not a bit may change against the one-target kernel (forward_form 1) and the CPU oracle -- paths,
log-likelihood bits and the raw history rows [B, T, SD] after zeroing the workspace (pad column S carries the frame maximum M).

Three directed emission sets, each checked on the CPU first, against the oracle's own delta rows (the dense recursion of
oracle.viterbi_oracle.decode_numpy, whose last row is held against decode_c), to have the property it claims ("premise"):
  (i)   every window position of every half-wave target wins: for every target j >= 256 and every position w there is a frame in
        which source lo_j + w alone carries the winning candidate of j (a one-hot spike in the frame before it) -- the winner in the
        lower half, in the upper half and at both ends of each, for each of the 32 target slots of each half wave;
  (ii)  every quad carries M: for every quad of lanes of every wave that holds a live, non-extra state there is a frame whose maximum
        M is attained in that quad's states and nowhere else (quads of idle slots and the extra column's quad cannot carry M);
  (iii) the extra column must not enter M: frames in which delta[x] is the frame's largest delta by more than 100, frames in which it
        is -inf, and the "inf" emissions of tests/test_gpu_floor_split_trim.py with their -0.0 values.
        In all four matrices the issue names, A[j, x] > c_j for every j, so fl(delta_x + c_j) can never exceed the true candidate
        fl(delta_x + A[j, x]): there a wrong M shows in pad column S of the history rows only (premise: delta_x above the true M by
        the margin in frames whose M is stored and compared).  "tonet361_lowx" is tonet's 361-state matrix with the extra column's
        entry 30 below the row constant in six rows, of full and of half waves: there the premise holds as stated -- some j for which
        fl(delta_x + c_j) exceeds every true candidate -- and a delta row would change."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests.plan_replay import HostPlan
from tests.test_floor_trim_host import _s300mid, _tonet
from tests.test_gpu_floor_split_trim import _check, _emissions, _random
from viterbi_spl_amd import ViterbiDecoder, _lib

pytestmark = pytest.mark.gpu

FULL_WAVES, HALF_WAVES = 4, 4
SPIKE = np.float32(300.0)                     # above every matrix entry's distance from 0 (tonet: 87.4) plus the noise (2.5) by > 200
MARGIN = 100.0
LENGTHS = ([37, 25, 13, 2], [24, 12, 1])      # every tail of the twelve-frame round, in batches of at most six songs
LOWX_ROWS = (5, 130, 200, 260, 300, 355)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _tonet_lowx():
    A, pi = _tonet(361)
    A = A.copy()
    c = HostPlan(A, pi).rowc
    for j in LOWX_ROWS:
        A[j, 360] = c[j] - np.float32(30.0)
    return A, pi


# name -> (matrix builder, extra column leaves M by address: one extra column x = S - 1, x % 4 == 0)
MATRICES = {
    "tonet361": (lambda: _tonet(361), True),
    "tonet321": (lambda: _tonet(321), True),
    "S257": (lambda: _random(257, 256, 12), True),
    "S300mid": (_s300mid, False),
    "tonet361_lowx": (_tonet_lowx, True),
}
_cache = {}


def _case(name):
    if name not in _cache:
        A, pi = MATRICES[name][0]()
        plan = HostPlan(A, pi)
        S = A.shape[0]
        assert plan.ok and plan.floor_ok and plan.W == 32 and plan.n_dense == 0 and len(plan.extras) == 1 and 256 < S < 384, name
        x = plan.extras[0]
        assert (x == S - 1 and x % 4 == 0) == MATRICES[name][1], (name, x)
        _cache[name] = {"A": A, "pi": pi, "plan": plan, "x": x}
    return _cache[name]


def _decoder(name, dev):
    c = _case(name)
    if "dec" not in c:
        c["dec"] = ViterbiDecoder(c["A"], c["pi"], dev)
    return c["dec"]


# ---- the kernel's maps, restated: lanes l and l ^ 8 of a half wave share a target; lanes with bit 3 clear take the targets in order
def _half_target(lane):
    return ((lane >> 4) << 3) | (lane & 7)


def _quad_states(wave, quad):
    lanes = range(4 * quad, 4 * quad + 4)
    if wave < FULL_WAVES:
        return [64 * wave + l for l in lanes]
    return [64 * FULL_WAVES + 32 * (wave - FULL_WAVES) + _half_target(l) for l in lanes]


def test_lane_map_restated():
    for wave in range(FULL_WAVES, FULL_WAVES + HALF_WAVES):
        seen = sorted(s for q in range(16) for s in _quad_states(wave, q))
        base = 256 + 32 * (wave - FULL_WAVES)
        assert seen == sorted(list(range(base, base + 32)) * 2)
        for q in range(16):
            assert _quad_states(wave, q) == _quad_states(wave, q ^ 2) and _quad_states(wave, q)[0] % 4 == 0


# ---- the oracle's delta rows
def _delta_rows(A, pi, E):
    """[B, T, S]: the dense recursion of oracle.viterbi_oracle.decode_numpy; the last row is held against decode_c's."""
    B, T, S = E.shape
    d = np.empty((B, T, S), np.float32)
    d[:, 0] = pi[None, :] + E[:, 0]
    for t in range(1, T):
        for b in range(B):
            d[b, t] = np.max(d[b, t - 1][None, :] + A, axis=1) + E[b, t]
    ref = vo.decode_c(A, pi, E, return_delta=True)[2]
    assert d[:, -1].tobytes() == ref.tobytes(), "the test's delta rows are not the oracle's"
    return d


def _noise(rng, B, T, S):
    return -(rng.integers(0, 6, (B, T, S)) / 2).astype(np.float32)


def _spread(cols, S, seed):
    """One spike per frame, the columns dealt out over two songs: E [2, n + 1, S]."""
    cols = list(cols)
    per = [cols[0::2], cols[1::2]]
    T = max(max(len(p) for p in per) + 1, 38)      # (at least the 37 frames the ragged batches take)
    assert T <= 200
    E = _noise(np.random.default_rng(seed), 2, T, S)
    for b, p in enumerate(per):
        for t, col in enumerate(p):
            E[b, t, col] = SPIKE
    return E


def _set_window(c):
    """(i): a spike on every source some half-wave target has in its window."""
    S, lo = c["plan"].S, c["plan"].lo
    cols = sorted({int(lo[j]) + w for j in range(256, S) for w in range(32)})
    return _spread(cols, S, seed=11)


def _premise_window(c, E, d):
    A, S, lo = c["A"], c["plan"].S, c["plan"].lo[:c["plan"].S].astype(np.int64)
    won = np.zeros((S, 32), bool)
    js = np.arange(256, S)
    for b in range(E.shape[0]):
        for t in range(1, E.shape[1]):
            cand = d[b, t - 1][None, :] + A[256:S]
            best = cand.max(axis=1)
            alone = (cand == best[:, None]).sum(axis=1) == 1
            w = cand.argmax(axis=1) - lo[256:S]
            ok = alone & (w >= 0) & (w < 32)
            won[js[ok], w[ok]] = True
    missing = np.argwhere(~won[256:S])
    assert missing.size == 0, ("premise", "(target - 256, window position) that never wins alone", missing[:8])


def _m_groups(c):
    """4-aligned groups of states that hold a live, non-extra state."""
    S, x = c["plan"].S, c["x"]
    return [g for g in range((S + 3) // 4) if any(s < S and s != x for s in range(4 * g, 4 * g + 4))]


def _set_quads(c):
    """(ii): a spike in every 4-aligned group of states, at a varying place in the group."""
    S, x = c["plan"].S, c["x"]
    cols = []
    for g in _m_groups(c):
        live = [s for s in range(4 * g, 4 * g + 4) if s < S and s != x]
        cols.append(live[g % len(live)])
    return _spread(cols, S, seed=12)


def _premise_quads(c, E, d):
    S, x = c["plan"].S, c["x"]
    carried = set()
    for b in range(E.shape[0]):
        for t in range(E.shape[1] - 1):                    # the frames whose M the next frame reads
            row = d[b, t].copy()
            row[x] = -np.inf
            top = np.flatnonzero(row == row.max())
            if np.isfinite(row.max()) and len({int(s) // 4 for s in top}) == 1:
                carried.add(int(top[0]) // 4)
    n = 0
    for wave in range(FULL_WAVES + HALF_WAVES):
        for quad in range(16):
            states = _quad_states(wave, quad)
            if not any(s < S and s != x for s in states):
                continue                                   # idle slots and the extra column's quad: nothing that could carry M
            assert len({s // 4 for s in states}) == 1
            assert states[0] // 4 in carried, ("premise", "no frame with M in this quad alone", wave, quad, states)
            n += 1
    assert n >= 64, n                                      # (S = 257: the half waves hold the extra column and idle slots only)


def _set_extra(c):
    """(iii): song 0 spikes the extra column every third frame and sends it to -inf in between; song 1 is the "inf" kind."""
    S, x = c["plan"].S, c["x"]
    T = 60
    E = _noise(np.random.default_rng(13), 2, T, S)
    E[0, 0::3, x] = SPIKE
    E[0, 1::6, x] = -np.inf
    E[1] = _emissions("inf", 1, T, S, quant=True)[0]
    return E


def _premise_extra(c, E, d, name):
    A, S, x, rowc = c["A"], c["plan"].S, c["x"], c["plan"].rowc[:c["plan"].S]
    others = np.delete(d[0], x, axis=1).max(axis=1)        # the true M of every frame of song 0
    big = np.flatnonzero(d[0, :-1, x] > others[:-1] + MARGIN)
    assert len(big) >= 10, ("premise", "frames with delta[x] far above M", len(big))
    assert np.sum(np.isneginf(d[0, :-1, x])) >= 5, ("premise", "frames with delta[x] = -inf")
    assert np.any((E[1] == 0) & np.signbit(E[1])) and np.any(np.isneginf(E[1])), ("premise", "-0.0 and -inf emissions")
    # some j for which fl(delta_x + c_j) would exceed every true candidate: possible only where A[j, x] < c_j
    hit = set()
    for t in big:
        true = np.max(d[0, t][None, :] + A, axis=1)
        wrong = (d[0, t, x] + rowc).astype(np.float32)
        hit |= {int(j) for j in np.flatnonzero(wrong > true)}
    if name == "tonet361_lowx":
        assert hit == set(LOWX_ROWS), ("premise", "rows a wrong M would change", sorted(hit))
    else:
        assert np.all(A[:, x] > rowc) and not hit, ("premise", "the extra column's entries lie above the row constants", sorted(hit))


SETS = {"window": (_set_window, _premise_window), "quads": (_set_quads, _premise_quads), "extra": (_set_extra, _premise_extra)}


def _directed(name, kind):
    c = _case(name)
    key = "set_" + kind
    if key not in c:
        E = SETS[kind][0](c)
        d = _delta_rows(c["A"], c["pi"], E)
        if kind == "extra":
            _premise_extra(c, E, d, name)
        else:
            SETS[kind][1](c, E, d)
        c[key] = E
    return c[key]


@pytest.mark.parametrize("kind", list(SETS))
@pytest.mark.parametrize("name", ["tonet361", "tonet321", "S257", "S300mid"])
def test_directed_set_is_bit_exact(dev, name, kind):
    E = _directed(name, kind)
    assert E.shape[0] <= 6 and E.shape[1] <= 200
    c = _case(name)
    _check(_decoder(name, dev), c["A"], c["pi"], torch.from_numpy(E).to(dev), None, (name, kind))


def test_extra_column_that_would_change_a_delta(dev):
    """Set (iii) on the matrix where a frame maximum that took the extra column in would change delta rows, not only pad column S."""
    name = "tonet361_lowx"
    E = _directed(name, "extra")
    c = _case(name)
    _check(_decoder(name, dev), c["A"], c["pi"], torch.from_numpy(E).to(dev), None, (name, "extra"))


@pytest.mark.parametrize("name", ["tonet361", "tonet321", "S257", "S300mid"])
def test_every_tail_of_the_round(dev, name):
    """Ragged lengths 1, 2, 12, 13, 24, 25, 37 over the first 37 frames of the three directed sets."""
    c = _case(name)
    Eall = np.concatenate([_directed(name, kind)[:, :37] for kind in SETS])[[0, 2, 4, 5]]
    assert Eall.shape[1] == 37
    for lengths in LENGTHS:
        E = torch.from_numpy(Eall[:len(lengths)].copy()).to(dev)
        _check(_decoder(name, dev), c["A"], c["pi"], E, torch.tensor(lengths, dtype=torch.int64, device=dev), (name, lengths))
