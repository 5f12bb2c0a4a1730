"""GPU tests of the host decoder's call path (viterbi_spl_amd/decoder.py, stream.py): every decode entry that takes a workspace
gives the same bits with its own buffer, with a caller's tensor of exactly the need + 256 bytes and for a single [T, S] input;
synchronises once if and only if it allocated; refuses a bad workspace before anything is enqueued; answers an unserved plan as
recorded in tests/golden/decoder_unserved.json; and a session's life cycle.  The comparisons against the oracle live in the
entries' own test files: here each entry is compared with the sibling that defines it (``decode``, ``decode_f64``, the emission
builder followed by ``decode(algo="wave")``), exactly.

Shapes: B = 3, T = 130, lengths (130, 1, 67), segment_frames = 64 -- the smallest at which every entry has more than one segment
and a ragged batch.  Plans of params.npz: tonet361 (wave form: serves every entry), jdc722 (floor form: the workgroup path of the
packed and budgeted decodes, and float64), dense97 (serves none of them)."""
import json

import numpy as np
import pytest
import torch

from tests.golden import make_decoder_unserved as mk
from viterbi_spl_amd import ViterbiDecoder, _lib, emissions

pytestmark = pytest.mark.gpu

B, T, K, LENGTHS = mk.B, mk.T, mk.K, mk.LENGTHS
N = sum(LENGTHS)
F64_GROUP_SPLIT = (2, LENGTHS[0] + LENGTHS[1])      # decode_f64_packed under the budget of its first two recordings: two groups


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


class Ctx:
    """A plan's decoder, the inputs of mk.inputs and the three sibling results, computed once."""

    def __init__(self, golden, dev, plan):
        p = golden["params"]
        self.dec = ViterbiDecoder(p[f"{plan}_logA_T"], p[f"{plan}_log_pi"], dev)
        self.E, self.lens, self.Ep, self.off, self.X, self.obs = mk.inputs(self.dec.S, dev)
        self._ref = {}

    def ref(self, sibling):
        if sibling not in self._ref:
            d = self.dec
            got = {"f32": lambda: d.decode(self.E, lengths=self.lens),
                   "f64": lambda: d.decode_f64(self.E, lengths=self.lens),
                   "logits": lambda: d.decode(emissions.shaun_log_emissions(self.X, 0.32, 5), lengths=self.lens, algo="wave")}[sibling]()
            self._ref[sibling] = norm(got, "padded", self.off)
        return self._ref[sibling]


_CTX = {}


def ctx_of(golden, dev, plan):
    if plan not in _CTX:
        _CTX[plan] = Ctx(golden, dev, plan)
    return _CTX[plan]


def norm(result, kind, off, single=False):
    """(states, loglik) of any entry -> ([the path of each recording inside its length], the log-likelihood bits)."""
    torch.cuda.synchronize()
    st, ll = (x.cpu().numpy() for x in result)
    bits = np.atleast_1d(ll).view(np.int32 if ll.dtype == np.float32 else np.int64)
    if single:
        return [st], bits
    if kind == "packed":
        return [st[off[b]:off[b + 1]] for b in range(B)], bits
    return [st[b, :LENGTHS[b]] for b in range(B)], bits


def same(a, b, recordings=range(B)):
    return all(np.array_equal(a[0][i], b[0][b_i]) and a[1][i] == b[1][b_i] for i, b_i in enumerate(recordings))


# name -> (plans, kind of input, sibling, synchronisations of a call that allocates, need(c), call(c, workspace, single))
def _padded(method, sized, **kw):
    return (lambda c: getattr(c.dec, sized)(B, T, *kw.values()),
            lambda c, ws, single: getattr(c.dec, method)(c.E[0] if single else c.E, lengths=None if single else c.lens, workspace=ws, **kw))


def _packed(method, sized, **kw):
    return (lambda c: getattr(c.dec, sized)(c.off, *kw.values()) if kw else getattr(c.dec, sized)(B, N),
            lambda c, ws, single: getattr(c.dec, method)(c.Ep, c.off, workspace=ws, **kw))


def _logits(method, sized, **kw):
    return (lambda c: getattr(c.dec, sized)(c.obs, B, T, *kw.values()),
            lambda c, ws, single: getattr(c.dec, method)(c.X[0] if single else c.X, c.obs, lengths=None if single else c.lens, workspace=ws, **kw))


def _f64_groups_budget(c):
    return c.dec.workspace_bytes_f64_packed(*F64_GROUP_SPLIT)


BOTH, WAVE = ("tonet361", "jdc722"), ("tonet361",)
ENTRIES = {
    "decode_checkpointed": (BOTH, "padded", "f32", 1) + _padded("decode_checkpointed", "workspace_bytes_checkpointed", segment_frames=K),
    "decode_f64": (BOTH, "padded", "f64", 0) + _padded("decode_f64", "workspace_bytes_f64"),
    "decode_f64_checkpointed": (BOTH, "padded", "f64", 1) + _padded("decode_f64_checkpointed", "workspace_bytes_f64_checkpointed", segment_frames=K),
    "decode_packed": (BOTH, "packed", "f32", 1) + _packed("decode_packed", "workspace_bytes_packed"),
    "decode_packed_checkpointed": (WAVE, "packed", "f32", 1) + _packed("decode_packed_checkpointed", "workspace_bytes_packed_checkpointed", segment_frames=K),
    "decode_packed_bounded": (BOTH, "packed", "f32", 1) + _packed("decode_packed_bounded", "workspace_bytes_packed_bounded", segment_frames=K),
    "decode_f64_packed": (BOTH, "packed", "f64", 1) + _packed("decode_f64_packed", "workspace_bytes_f64_packed"),
    "decode_f64_packed(groups)": (BOTH, "packed", "f64", 1,
                                  _f64_groups_budget,       # (the need of the largest group = the budget: the first two recordings)
                                  lambda c, ws, single: c.dec.decode_f64_packed(c.Ep, c.off, workspace=ws, max_workspace_bytes=_f64_groups_budget(c))),
    "decode_f64_packed_checkpointed": (BOTH, "packed", "f64", 1) + _packed("decode_f64_packed_checkpointed", "workspace_bytes_f64_packed_checkpointed", segment_frames=K),
    "decode_logits": (WAVE, "logits", "logits", 1) + _logits("decode_logits", "workspace_bytes_logits"),
    "decode_logits_checkpointed": (WAVE, "logits", "logits", 1) + _logits("decode_logits_checkpointed", "workspace_bytes_logits_checkpointed", segment_frames=K),
}
CASES = [(plan, name) for name, spec in ENTRIES.items() for plan in spec[0]]


class SyncCount:
    """Counts ``torch.cuda.Stream.synchronize`` and ``torch.cuda.synchronize`` inside a ``with`` block (both still run)."""

    def __enter__(self):
        self.n = 0
        self._mp = pytest.MonkeyPatch()
        for owner, name in ((torch.cuda.Stream, "synchronize"), (torch.cuda, "synchronize")):
            self._mp.setattr(owner, name, self._counting(getattr(owner, name)))
        return self

    def _counting(self, fn):
        def wrapper(*args, **kw):
            self.n += 1
            return fn(*args, **kw)
        return wrapper

    def __exit__(self, *exc):
        self._mp.undo()


def exact_workspace(need, dev):
    return torch.empty(need + 256, dtype=torch.uint8, device=dev)


@pytest.mark.parametrize("plan,name", CASES)
def test_workspace_modes_agree_and_synchronise_by_the_rule(golden, dev, plan, name):
    """States and log-likelihood bits: own buffer == caller's tensor of need + 256 bytes == single input == the sibling; one
    synchronisation where the call allocated, none with a caller's workspace (``decode_f64``: none either way)."""
    c = ctx_of(golden, dev, plan)
    _, kind, sibling, syncs, need, call = ENTRIES[name]
    ref = c.ref(sibling)
    if name == "decode_f64_packed(groups)":
        assert len(c.dec.plan_workspace_f64_packed(c.off, need(c))["groups"]) == 2
    with SyncCount() as own:
        r_own = call(c, None, False)
    ws = exact_workspace(need(c), dev)
    with SyncCount() as given:
        r_ws = call(c, ws, False)
    assert same(norm(r_own, kind, c.off), ref), "own buffer differs from " + sibling
    assert same(norm(r_ws, kind, c.off), ref), "caller's workspace differs from " + sibling
    assert (own.n, given.n) == (syncs, 0)
    if kind != "packed":
        r_one = call(c, None, True)
        assert r_one[0].shape == (T,) and r_one[1].shape == ()
        assert same(norm(r_one, kind, c.off, single=True), ref, recordings=[0]), "single input differs from " + sibling


@pytest.mark.parametrize("plan", BOTH)
def test_decoder_owned_buffers_never_synchronise(golden, dev, plan):
    """``decode`` / ``decode_into`` run in the slot buffers, ``decode_f64`` in slot 0's, shared with ``decode``; under a budget it
    first drops a slot-0 buffer larger than the budget.  None of them synchronises."""
    c = ctx_of(golden, dev, plan)
    dec = c.dec
    c.ref("f32"), c.ref("f64")                                           # (computed before the buffers are looked at)
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    loglik = torch.empty((B,), dtype=torch.float32, device=dev)
    dec._ws, dec._ws_slots = None, {}
    with SyncCount() as s:
        got = dec.decode(c.E, lengths=c.lens)
        dec.decode_into(c.E, states, loglik, c.lens)
        dec.decode_into(c.E, states, loglik, c.lens, slot=1)
    assert s.n == 0 and same(norm(got, "padded", c.off), c.ref("f32")) and same(norm((states, loglik), "padded", c.off), c.ref("f32"))
    assert dec._ws.numel() == dec.workspace_bytes(B, T, "auto") + 256 and sorted(dec._ws_slots) == [1]
    need = dec.workspace_bytes_f64(B, T)
    dec._workspace(4 * B, 2 * T)                                         # slot 0 grows past the float64 need ...
    big = dec._ws
    assert big.numel() > need + 256
    with SyncCount() as s:
        got = dec.decode_f64(c.E, lengths=c.lens)
    assert s.n == 0 and dec._ws is big and same(norm(got, "padded", c.off), c.ref("f64"))
    with SyncCount() as s:                                               # ... and the budget of exactly that need drops it
        got = dec.decode_f64(c.E, lengths=c.lens, max_workspace_bytes=need)
    assert s.n == 0 and dec._ws is not big and dec._ws.numel() == need + 256 and same(norm(got, "padded", c.off), c.ref("f64"))
    with SyncCount() as s:                                               # below the need: the checkpointed form, in a buffer of the call
        got = dec.decode_f64(c.E, lengths=c.lens, max_workspace_bytes=need - 1)
    assert s.n == 1 and dec._ws.numel() == need + 256 and same(norm(got, "padded", c.off), c.ref("f64"))
    dec._ws, dec._ws_slots = None, {}


@pytest.mark.parametrize("plan,name", [(spec[0][-1], name) for name, spec in ENTRIES.items()])
def test_bad_workspace_is_refused(golden, dev, plan, name):
    """One byte short of need + 256, another dtype, on the CPU: ValueError, and what an earlier good call returned is untouched."""
    c = ctx_of(golden, dev, plan)
    _, kind, sibling, _, need, call = ENTRIES[name]
    n = need(c)
    good = call(c, exact_workspace(n, dev), False)
    torch.cuda.synchronize()
    kept = [x.clone() for x in good]
    for bad in (torch.empty(n + 255, dtype=torch.uint8, device=dev), torch.empty(n + 256, dtype=torch.int8, device=dev),
                torch.empty(n + 256, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=f"at least {n + 256} bytes"):
            call(c, bad, False)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(good, kept)) and same(norm(good, kind, c.off), c.ref(sibling))


def test_unserved_plan_answers(golden, dev):
    """dense97: every size query, budgeted / packed / float64 / logits decode, budget plan and session open answers as recorded
    (exception type and full text, or the value)."""
    with open(mk.OUT) as fh:
        want = json.load(fh)
    got = json.loads(json.dumps(mk.record(ctx_of(golden, dev, mk.PLAN).dec, dev)))
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


@pytest.mark.parametrize("ring", [False, True])
def test_session_life_cycle(golden, dev, ring):
    c = ctx_of(golden, dev, "tonet361")
    dec = c.dec
    for args, kw in (((0, 10), {}), ((2,), {}), ((0,), {"ring_frames": 64})):
        with pytest.raises(ValueError):
            dec.stream(*args, **kw)
    unserved = ctx_of(golden, dev, mk.PLAN).dec
    for kw in ({"max_frames": 64}, {"ring_frames": 64}):
        with pytest.raises(_lib.ViterbiHipError):
            unserved.stream(2, **kw)
    st = dec.stream(B, ring_frames=64) if ring else dec.stream(B, T)
    st.reset()                                                           # before any commit
    assert st.committed_states is None and (st.lengths == 0).all()
    ref_s, ref_l = dec.decode(c.E)                                       # three recordings of T frames, fed in chunks
    parts = [[] for _ in range(B)]
    step = 30 if ring else 50
    for t0 in range(0, T, step):
        st.append(c.E[:, t0:t0 + step].contiguous())
        out = st.commit()
        if not ring:
            assert st.committed_states.shape == (B, T)
        for b in range(B):
            parts[b].append(out[-1][b])
    assert (st.lengths == T).all()
    first, tail, loglik = st.tail()
    for b in range(B):
        path = torch.cat(parts[b] + [tail[b]])
        assert first[b] == sum(len(p) for p in parts[b]) and torch.equal(path, ref_s[b]), b
    assert torch.equal(loglik.view(torch.int32), ref_l.view(torch.int32))
    assert (st.committed_states is None) == ring
    st.reset()
    assert (st.lengths == 0).all()
    st.close()
    st.close()
    rows = torch.empty((B, T), dtype=torch.int32, device=dev)
    i64 = torch.zeros((B,), dtype=torch.int64, device=dev)
    calls = {"append": lambda: st.append(c.E[:, :4].contiguous()), "lengths": lambda: st.lengths, "decode": st.decode,
             "decode_into": lambda: st.decode_into(rows), "commit": st.commit, "commit_into": lambda: st.commit_into(rows, i64),
             "commit_rel_into": lambda: st.commit_rel_into(rows, i64, i64.clone()), "ack": lambda: st.ack([0] * B), "tail": st.tail,
             "tail_into": lambda: st.tail_into(rows, i64), "reset": st.reset}
    for name, fn in calls.items():
        # (a ring session refuses the two calls that need every history row before it looks at the handle)
        text = "ring session" if ring and name in ("decode_into", "commit_into") else "the stream is closed"
        with pytest.raises(_lib.ViterbiHipError, match=text):
            fn()
