"""GPU tier of the two-stream schedule: two batches in flight on one plan, each in its own workspace slot, every result against the
CPU oracle (oracle.viterbi_oracle.decode_c; tests/f64_ref.py for the float64 decodes) run on that batch alone -- never against
another run of the library.

What two decodes in flight on one plan share, and what each part below is after:
* the per-plan forward records keyed by workspace pointer (capi.hip: FwdStamp, stamp_put / stamp_get): vit_backtrace takes the history
  layout, the family, aux_frames, the half-history flag and the emission pointer from the record -- with two slots the record it needs
  is not the most recent one (parts 2 and 3);
* the one pinned staging buffer per plan of the packed decodes (pk_stage / pk_upload): the host rewrites it for the next call while
  the previous call's upload may still be queued behind other work on its stream (part 4);
* the half history's lifetime rule: the back-trace of batch i re-reads the emissions of batch i while the forward pass of batch i + 1
  reads another tensor (parts 2 and 3);
* plan-wide options (bt_chunks, bt_block_waves, backtrace_form) in force while batches with different records are in flight.

A library fault must show as a wrong path, never as a GPU fault: two calls that could be confused with each other have the same B
and T (packed calls: the same multiset of lengths), and every workspace exists at the size that serves any form before anything is
enqueued, so a mix-up reads and writes inside buffers the test owns.  One process, one host thread, no captured graphs."""
import math
import time

import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests import f64_ref
from tests.common import GEN
from viterbi_spl_amd import ViterbiDecoder, _lib

pytestmark = pytest.mark.gpu

SENTINEL = -7
KINDS = tuple(GEN)                                   # peaks, dense, ties, scaled: the kind rotates step by step
ORDERS = ("pipelined", "forward_ahead", "forward_ahead_reversed")
PLANS = ("tonet361", "msnet321", "jdc722", "durrieu722", "dense361", "dense97")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def decoders(golden, dev):
    yield {name: ViterbiDecoder(golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"], dev) for name in PLANS}
    _steps_cache.clear()                             # the shared inputs and references live as long as the module's tests
    _rec_cache.clear()


def _params(golden, name):
    return golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. the schedule helper
# ----------------------------------------------------------------------------------------------------------------------------------
def _lengths(rng, B, T, step):
    """Ragged, different at every step: drawn from {T, T - 1, T // 2, 66, 65, 64, 3, 2, 1}; one song is T (even steps) or T - 1 frames
    long, so that every step has a song over (nearly) all chunks of the back-trace."""
    pool = np.asarray([T, T - 1, T // 2, 66, 65, 64, 3, 2, 1], np.int64)
    lens = rng.permutation(pool)[:B] if B <= len(pool) else rng.choice(pool, B)
    lens[int(rng.integers(B))] = T - (step & 1)
    return lens


_steps_cache = {}


def _steps(golden, dev, name, B, T, f16s):
    """The inputs of len(f16s) steps on plan `name` and the oracle's result for each, computed once per key and never modified: step i
    has its own emission kind (KINDS[i % 4]), seed, lengths and storage type.  The oracle decodes song by song, so one call over the
    songs of all steps is the oracle run on every batch alone."""
    key = (name, B, T, tuple(f16s))
    if key not in _steps_cache:
        A, pi = _params(golden, name)
        S = A.shape[0]
        rng = np.random.default_rng(1000 * T + B)
        steps = []
        for i, f16 in enumerate(f16s):
            E = GEN[KINDS[i % len(KINDS)]](B, T, S, seed=7919 * (i + 1) + T + B, dtype=torch.float16 if f16 else torch.float32, device=dev)
            steps.append({"E": E, "lens_h": _lengths(rng, B, T, i)})
        ref_s, ref_l = vo.decode_c(A, pi, np.concatenate([s["E"].float().cpu().numpy() for s in steps]),
                                   lengths=np.concatenate([s["lens_h"] for s in steps]))
        for i, s in enumerate(steps):
            s["lens"] = torch.from_numpy(s["lens_h"]).to(dev)
            s["ref_s"], s["ref_l"] = ref_s[i * B:(i + 1) * B], ref_l[i * B:(i + 1) * B]
            for b in range(B):                                         # (the ABI's rule, on the oracle's output: -1 past a song's end)
                n = int(s["lens_h"][b])
                assert np.all(s["ref_s"][b, :n] >= 0) and np.all(s["ref_s"][b, n:] == -1)
        _steps_cache[key] = steps
    return _steps_cache[key]


def _batches(golden, dev, name, B, T, f16s, algos, options=None):
    """batches[i] for run_schedule: the cached inputs and references of step i plus its own algo, its own options (set just before its
    forward pass) and fresh output tensors: states prefilled with SENTINEL, log-likelihoods with NaN."""
    out = []
    for i, s in enumerate(_steps(golden, dev, name, B, T, f16s)):
        b = dict(s)
        b["algo"] = algos[i]
        b["options"] = tuple(options[i]) if options else ()
        b["states"] = torch.full((B, T), SENTINEL, dtype=torch.int32, device=dev)
        b["loglik"] = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
        out.append(b)
    return out


def _forward(dec, b, slot):
    for key, value in b["options"]:
        dec.set_option(key, value)
    dec.decode_into(b["E"], b["states"], b["loglik"], b["lens"], algo=b["algo"], phase="forward", slot=slot)


def _backtrace(dec, b, slot):
    dec.decode_into(b["E"], b["states"], b["loglik"], b["lens"], algo=b["algo"], phase="backtrace", slot=slot)


def run_schedule(dec, batches, order):
    """Batch i runs in workspace slot i % 2 on two streams.  Every tensor and both workspaces (at the size that serves any form) exist
    before the first enqueue; one synchronisation at the end, none between steps.
    "pipelined": bench.py's step() -- the forward pass of batch i on a high-priority stream, its back-trace on a second stream behind
    an event, the forward pass into a slot behind the back-trace that last used it.
    "forward_ahead": per pair of steps (2j, 2j + 1) both forward passes, one event, both back-traces behind it; the next pair's forward
    passes wait for both back-traces.  The forward pass of the later batch has finished before the back-trace of the earlier one starts.
    "forward_ahead_reversed": the same with the back-trace of step 2j + 1 enqueued first -- the record wanted first is the most recent.
    -> for "pipelined" the steps i whose back-trace interval (timing events) intersected the forward pass of step i + 1, else None."""
    dev = dec.device
    B, T = batches[0]["E"].shape[:2]
    assert all(tuple(b["E"].shape[:2]) == (B, T) and tuple(b["states"].shape) == (B, T) for b in batches), "one (B, T) in both slots"
    ws = [dec._workspace(B, T, k, None) for k in (0, 1)]
    s_fwd, s_bt = torch.cuda.Stream(device=dev, priority=-1), torch.cuda.Stream(device=dev)
    spans = []
    torch.cuda.synchronize(dev)                                  # the inputs and the sentinels are in place
    try:
        if order == "pipelined":
            bt_done = [None, None]
            for i, b in enumerate(batches):
                k = i % 2
                with torch.cuda.stream(s_fwd):
                    if bt_done[k] is not None:
                        s_fwd.wait_event(bt_done[k])
                    f0 = torch.cuda.Event(enable_timing=True)
                    f0.record()
                    _forward(dec, b, k)
                    fwd_done = torch.cuda.Event(enable_timing=True)
                    fwd_done.record()
                with torch.cuda.stream(s_bt):
                    s_bt.wait_event(fwd_done)
                    b0 = torch.cuda.Event(enable_timing=True)
                    b0.record()
                    _backtrace(dec, b, k)
                    bt_done[k] = torch.cuda.Event(enable_timing=True)
                    bt_done[k].record()
                spans.append((f0, fwd_done, b0, bt_done[k]))
        elif order in ("forward_ahead", "forward_ahead_reversed"):
            bt_done = []
            for j in range(0, len(batches), 2):
                pair = list(range(j, min(j + 2, len(batches))))
                with torch.cuda.stream(s_fwd):
                    for ev in bt_done:
                        s_fwd.wait_event(ev)
                    for i in pair:
                        _forward(dec, batches[i], i % 2)
                    fwd_done = torch.cuda.Event()
                    fwd_done.record()
                with torch.cuda.stream(s_bt):
                    s_bt.wait_event(fwd_done)
                    bt_done = []
                    for i in (pair[::-1] if order == "forward_ahead_reversed" else pair):
                        _backtrace(dec, batches[i], i % 2)
                        bt_done.append(torch.cuda.Event())
                        bt_done[-1].record()
        else:
            raise ValueError(order)
    finally:
        torch.cuda.synchronize(dev)
    assert [dec._workspace(B, T, k, None) for k in (0, 1)] == ws, "a workspace slot was replaced while the schedule ran"
    if order != "pipelined":
        return None
    t = [[spans[0][0].elapsed_time(ev) for ev in sp] for sp in spans]            # ms since the first forward pass began
    return [i for i in range(len(t) - 1) if max(t[i][2], t[i + 1][0]) < min(t[i][3], t[i + 1][1])]


def check_batches(batches, what):
    """Every batch against the oracle's decode of it alone, bit for bit; no sentinel left, -1 past a song's length."""
    for i, b in enumerate(batches):
        st, ll = b["states"].cpu().numpy(), b["loglik"].cpu().numpy()
        assert not np.any(st == SENTINEL), (what, i, "states the back-trace did not write: %d" % int(np.sum(st == SENTINEL)))
        for s in range(st.shape[0]):
            n = int(b["lens_h"][s])
            assert np.all(st[s, n:] == -1) and np.all(st[s, :n] >= 0), (what, i, s, n)
        assert np.array_equal(st, b["ref_s"]), (what, i, b["algo"], "states differ in %d entries" % int(np.sum(st != b["ref_s"])))
        assert np.array_equal(ll.view(np.uint32), np.ascontiguousarray(b["ref_l"], np.float32).view(np.uint32)), (what, i, b["algo"], ll, b["ref_l"])


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. every family under every order, distinct data per step
# ----------------------------------------------------------------------------------------------------------------------------------
# (id, plan, algo, fp16 storage, options, B, T, the forward family and the history mode the case is about)
HALF, HALF8 = (("wave_history", 2),), (("wave_history", 2), ("bt_block_waves", 8))
CASES = (
    ("tonet361-group-f32", "tonet361", "group", False, (), 5, 1500, "group", "full"),         # the split floor kernel
    ("tonet361-group-f16", "tonet361", "group", True, (), 5, 1500, "group", "full"),
    ("tonet361-group-f32-lane", "tonet361", "group", False, (("backtrace_form", 4),), 5, 1500, "group", "full"),
    ("tonet361-wave-f32-full", "tonet361", "wave", False, (), 5, 1500, "wave", "full"),
    ("tonet361-wave-f32-half-1500", "tonet361", "wave", False, HALF, 5, 1500, "wave", "half"),
    ("tonet361-wave-f32-half-1500-bw8", "tonet361", "wave", False, HALF8, 5, 1500, "wave", "half"),
    ("tonet361-wave-f32-half-1501", "tonet361", "wave", False, HALF, 5, 1501, "wave", "half"),
    ("tonet361-wave-f32-half-1501-bw8", "tonet361", "wave", False, HALF8, 5, 1501, "wave", "half"),
    ("msnet321-wave-f16-half", "msnet321", "wave", True, HALF, 5, 1001, "wave", "half"),
    ("jdc722-banded-f16", "jdc722", "banded", True, (), 3, 800, "group", "full"),
    ("durrieu722-auto-f16-step0", "durrieu722", "auto", True, (("step_form", 0),), 3, 800, "dense", None),
    ("durrieu722-auto-f16-step3", "durrieu722", "auto", True, (("step_form", 3),), 3, 800, "dense", None),
    ("dense361-dense-f32", "dense361", "dense", False, (), 4, 600, "dense", None),
    ("dense97-dense-f32", "dense97", "dense", False, (), 9, 600, "dense", None),             # several songs per workgroup
)
N_STEPS = 6                                          # each slot is reused twice


@pytest.mark.parametrize("chunks", ["beside_forward", "library"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_family_under_every_order(golden, dev, decoders, case, order, chunks):
    """Six steps, two slots, every step its own emission kind, seed, ragged lengths: each batch equals the oracle's decode of it alone
    under bench.py's schedule and under the two gated orders, with bt_chunks = chunks_beside_forward(B) (what bench.py sets) and with
    the library's own count."""
    _, name, algo, f16, options, B, T, family, history = case
    dec = decoders[name]
    batches = _batches(golden, dev, name, B, T, [f16] * N_STEPS, [algo] * N_STEPS)
    try:
        for key, value in options:
            dec.set_option(key, value)
        n_chunks = dec.chunks_beside_forward(B) if chunks == "beside_forward" else 0
        if chunks == "beside_forward":
            assert 4 <= n_chunks <= 32 and T >= 8 * n_chunks, (n_chunks, T)     # premise: a forced count, chunks of real length
        dec.set_option("bt_chunks", n_chunks)
        assert dec.forward_family(B, algo) == family, (dec.forward_family(B, algo), family)
        if history is not None:
            assert dec.history_mode(B, T, algo) == history, (dec.history_mode(B, T, algo), history)
        overlapped = run_schedule(dec, batches, order)
    finally:
        dec.set_option("reset", 0)
    if overlapped is not None:                       # an observation, not a property: it depends on the machine's load
        print(f"\n[two streams] {case[0]} bt_chunks={n_chunks}: back-trace of step i ran beside the forward pass of step i + 1 for i in "
              f"{overlapped} ({len(overlapped)} of {N_STEPS - 1})")
    check_batches(batches, (case[0], order, chunks))


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. two different records in flight
# ----------------------------------------------------------------------------------------------------------------------------------
B3, T3 = 4, 900
# (id, (algo, fp16) of the even steps = slot 0, of the odd steps = slot 1)
PAIRS = (
    ("dense+group", ("dense", False), ("group", False)),
    ("group+wave", ("group", False), ("wave", False)),
    ("wave+dense", ("wave", False), ("dense", False)),
    ("group-f16+wave-f32", ("group", True), ("wave", False)),
)
FAMILY_OF = {"dense": "dense", "group": "group", "wave": "wave"}


@pytest.mark.parametrize("order", ORDERS[1:])
@pytest.mark.parametrize("pair", PAIRS, ids=[p[0] for p in PAIRS])
def test_two_records_in_flight(golden, dev, decoders, pair, order):
    """The two slots hold histories of different families (and storage types) when the back-traces run: each back-trace follows the
    record of ITS workspace, in either order.  Four steps: every slot is written twice.  (A stamp_get that returns the most recent
    record whatever the workspace fails every case here: the checked back-trace refuses the other batch's emission pointer.)"""
    _, even, odd = pair
    dec = decoders["tonet361"]
    side = [even, odd, even, odd]
    batches = _batches(golden, dev, "tonet361", B3, T3, [f for _, f in side], [a for a, _ in side])
    for a, _ in (even, odd):
        assert dec.forward_family(B3, a) == FAMILY_OF[a]
        assert dec.history_mode(B3, T3, a) == "full"
    run_schedule(dec, batches, order)
    check_batches(batches, (pair[0], order))


@pytest.mark.parametrize("order", ORDERS[1:])
def test_option_changes_between_the_two_forward_passes(golden, dev, decoders, order):
    """wave_history 2 before the forward pass into slot 0, wave_history 0 before the one into slot 1, both wave form: when the
    back-traces run the option says "full" and slot 0 holds a half history.  The header's promise: the back-trace follows the record
    (layout, half flag, emission pointer), not the option's current value."""
    dec = decoders["tonet361"]
    try:
        dec.set_option("wave_history", 2)
        assert dec.forward_family(B3, "wave") == "wave" and dec.history_mode(B3, T3, "wave") == "half"
        dec.set_option("wave_history", 0)
        assert dec.history_mode(B3, T3, "wave") == "full"
        batches = _batches(golden, dev, "tonet361", B3, T3, [False] * 4, ["wave"] * 4,
                           options=[(("wave_history", 2 if i % 2 == 0 else 0),) for i in range(4)])
        run_schedule(dec, batches, order)
    finally:
        dec.set_option("reset", 0)
    check_batches(batches, ("wave_history 2 | 0", order))


def _two_forward_passes(dec, batches):
    """Both forward passes on one stream, the second stream behind them (the state every refusal below starts from)."""
    dev = dec.device
    ws = [dec._workspace(B3, T3, k, None) for k in (0, 1)]
    s_fwd, s_bt = torch.cuda.Stream(device=dev, priority=-1), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s_fwd):
        _forward(dec, batches[0], 0)
        _forward(dec, batches[1], 1)
        fwd_done = torch.cuda.Event()
        fwd_done.record()
    s_bt.wait_event(fwd_done)
    return ws, s_fwd, s_bt


def test_refusal_of_the_other_slots_emissions(golden, dev, decoders):
    """With a second batch in flight: a back-trace on slot 1's workspace with slot 0's emission tensor is refused; the correct calls
    afterwards give the oracle's results.  Slot 0 holds a half history (its back-trace reads its emissions again), slot 1 a group one."""
    dec = decoders["tonet361"]
    batches = _batches(golden, dev, "tonet361", B3, T3, [False] * 2, ["wave", "group"], options=[(("wave_history", 2),), ()])
    try:
        dec.set_option("wave_history", 2)
        assert dec.history_mode(B3, T3, "wave") == "half" and dec.forward_family(B3, "group") == "group"
        ws, s_fwd, s_bt = _two_forward_passes(dec, batches)
        try:
            with torch.cuda.stream(s_bt):
                with pytest.raises(_lib.ViterbiHipError, match="invalid argument"):
                    dec.decode_into(batches[0]["E"], batches[1]["states"], None, batches[1]["lens"], algo="group", phase="backtrace", slot=1)
                with pytest.raises(_lib.ViterbiHipError, match="invalid argument"):
                    dec.decode_into(batches[1]["E"], batches[0]["states"], None, batches[0]["lens"], algo="wave", phase="backtrace", slot=0)
                _backtrace(dec, batches[1], 1)
                _backtrace(dec, batches[0], 0)
        finally:
            torch.cuda.synchronize(dev)
        assert [dec._workspace(B3, T3, k, None) for k in (0, 1)] == ws
    finally:
        dec.set_option("reset", 0)
    check_batches(batches, "after a refused back-trace")


def test_refusal_after_the_slot_was_rewritten_with_another_shape(golden, dev, decoders):
    """With a second batch in flight: a forward pass of another (B, T) into slot 0 (slices of the same tensors: the workspace stays the
    same) replaces the record, and a back-trace of the old shape is refused.  The back-trace of the new shape gives the oracle's result
    for its songs and writes nothing for the song that is no longer part of the batch; slot 1 is untouched by all of it."""
    dec = decoders["tonet361"]
    batches = _batches(golden, dev, "tonet361", B3, T3, [False] * 2, ["wave", "group"])
    b0, b1 = batches
    assert dec.forward_family(B3 - 1, "wave") == "wave" and dec.forward_family(B3, "group") == "group"
    ws, s_fwd, s_bt = _two_forward_passes(dec, batches)
    try:
        with torch.cuda.stream(s_fwd):                                          # B - 1 songs of the same tensors, the same pointers
            dec.decode_into(b0["E"][:B3 - 1], b0["states"][:B3 - 1], b0["loglik"][:B3 - 1], b0["lens"][:B3 - 1], algo="wave", phase="forward", slot=0)
            fwd_done = torch.cuda.Event()
            fwd_done.record()
        with torch.cuda.stream(s_bt):
            s_bt.wait_event(fwd_done)
            with pytest.raises(_lib.ViterbiHipError, match="no forward pass on record"):
                _backtrace(dec, b0, 0)
            dec.decode_into(b0["E"][:B3 - 1], b0["states"][:B3 - 1], b0["loglik"][:B3 - 1], b0["lens"][:B3 - 1], algo="wave", phase="backtrace", slot=0)
            bt_done = torch.cuda.Event()
            bt_done.record()
            _backtrace(dec, b1, 1)
        with torch.cuda.stream(s_fwd):                                          # the same memory as [B, T / 2, S]: T differs, B does not
            s_fwd.wait_event(bt_done)
            E_half = b0["E"][:B3 // 2].view(B3, T3 // 2, -1)
            assert E_half.data_ptr() == b0["E"].data_ptr() and E_half.is_contiguous()
            dec.decode_into(E_half, b0["states"][:B3 // 2].view(B3, T3 // 2), None, None, algo="wave", phase="forward", slot=0)
            with pytest.raises(_lib.ViterbiHipError, match="no forward pass on record"):
                _backtrace(dec, b0, 0)
    finally:
        torch.cuda.synchronize(dev)
    assert [dec._workspace(B3, T3, k, None) for k in (0, 1)] == ws
    assert bool((b0["states"][B3 - 1] == SENTINEL).all()), "the refused back-trace, or the one of B - 1 songs, wrote song B - 1"
    check_batches([b1], "slot 1 beside the rewritten slot 0")
    cut = dict(b0, states=b0["states"][:B3 - 1], loglik=b0["loglik"][:B3 - 1], lens_h=b0["lens_h"][:B3 - 1], ref_s=b0["ref_s"][:B3 - 1],
               ref_l=b0["ref_l"][:B3 - 1])
    check_batches([cut], "slot 0 with B - 1 songs")


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. packed decodes back to back on one staging buffer
# ----------------------------------------------------------------------------------------------------------------------------------
# X and Y hold the same multiset of lengths in another order (Y is a rotation of X) and different emissions: tables that reach the
# wrong call describe recordings inside both calls' buffers, and the paths come out wrong.
LENS_361 = (1000, 1, 2, 65, 300, 301, 777, 64, 3, 500, 129, 1000)
LENS_361_SMALL = (150, 1, 2, 65, 151, 64)                      # the float64 pairing: tests/f64_ref.py is a NumPy loop
LENS_722 = (400, 1, 2, 65, 399, 130)

_rec_cache = {}


def _recordings(golden, dev, name, lens, rot, f16, f64=False):
    """Recording set (X: rot = 0, Y: a rotation of the lengths and other emissions) -> packed emissions, host offsets and the
    reference's result per recording (float32 oracle, or the float64 restatement), computed once."""
    key = (name, lens, rot, f16, f64)
    if key not in _rec_cache:
        A, pi = _params(golden, name)
        ln = np.roll(np.asarray(lens, np.int64), rot)
        kind = KINDS[1 if rot else 0]                                            # X: peaks, Y: dense
        E = GEN[kind](len(ln), int(ln.max()), A.shape[0], seed=31 + 101 * rot + len(ln), dtype=torch.float16 if f16 else torch.float32, device=dev)
        off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
        Ep = torch.cat([E[b, :int(n)] for b, n in enumerate(ln)], dim=0).contiguous()
        Eh = E.float().cpu().numpy()
        ref_s, ref_l = f64_ref.decode_f64_batch(A, pi, Eh, ln) if f64 else vo.decode_c(A, pi, Eh, lengths=ln)
        _rec_cache[key] = {"Ep": Ep, "off": off, "lens": ln, "ref_s": ref_s, "ref_l": ref_l, "f64": f64}
    return _rec_cache[key]


def _packed_workspace(dec, entry, rec):
    B, N = len(rec["lens"]), int(rec["off"][-1])
    need = {"packed": lambda: dec.workspace_bytes_packed(B, N),
            "packed_checkpointed": lambda: dec.workspace_bytes_packed_checkpointed(rec["off"], 64),
            "packed_bounded": lambda: dec.workspace_bytes_packed_bounded(rec["off"], 64),
            "f64_packed": lambda: dec.workspace_bytes_f64_packed(B, N)}[entry]()
    assert need > 0
    return torch.empty(need + 256, dtype=torch.uint8, device=dec.device)


def _packed_call(dec, entry, rec, ws):
    """One packed decode in the caller's workspace: enqueued on the current stream, no synchronisation."""
    if entry == "packed":
        return dec.decode_packed(rec["Ep"], rec["off"], out_dtype=torch.int32, workspace=ws)
    if entry == "f64_packed":
        return dec.decode_f64_packed(rec["Ep"], rec["off"], out_dtype=torch.int32, workspace=ws)
    return getattr(dec, "decode_" + entry)(rec["Ep"], rec["off"], segment_frames=64, out_dtype=torch.int32, workspace=ws)


def check_packed(result, rec, what):
    st, ll = result[0].cpu().numpy(), result[1].cpu().numpy()
    off = rec["off"]
    assert st.shape == (int(off[-1]),) and ll.shape == (len(rec["lens"]),), what
    assert np.all(st >= 0), (what, "the packed states carry no -1")
    for b, n in enumerate(rec["lens"]):
        got, want = st[off[b]:off[b + 1]], rec["ref_s"][b, :n]
        assert np.array_equal(got, want), (what, b, int(n), "states differ in %d entries" % int(np.sum(got != want)))
    if rec["f64"]:
        assert ll.dtype == np.float64 and np.array_equal(f64_ref.bits64(ll), f64_ref.bits64(rec["ref_l"])), (what, ll, rec["ref_l"])
    else:
        assert ll.dtype == np.float32 and np.array_equal(ll.view(np.uint32), np.ascontiguousarray(rec["ref_l"], np.float32).view(np.uint32)), (what, ll, rec["ref_l"])


# (id, plan, fp16, the lengths, the second call)
BACK_TO_BACK = (
    ("tonet361-packed", "tonet361", False, LENS_361, "packed"),
    ("tonet361-checkpointed", "tonet361", False, LENS_361, "packed_checkpointed"),
    ("tonet361-f64", "tonet361", False, LENS_361_SMALL, "f64_packed"),
    ("jdc722-f16-bounded", "jdc722", True, LENS_722, "packed_bounded"),        # the workgroup-form kernels, the third staging caller
)


@pytest.mark.parametrize("case", BACK_TO_BACK, ids=[c[0] for c in BACK_TO_BACK])
def test_packed_calls_back_to_back_on_one_stream(golden, dev, decoders, case):
    """decode_packed(X), then a packed decode of Y, on one stream without a synchronisation in between: the second call stages its
    tables in the buffer the first call's upload reads from."""
    _, name, f16, lens, second = case
    dec = decoders[name]
    assert (dec.forward_family(len(lens), "wave") == "wave") if name == "tonet361" else not dec.info["wave_ok"]
    X = _recordings(golden, dev, name, lens, 0, f16)
    Y = _recordings(golden, dev, name, lens, 5 if len(lens) > 6 else 2, f16, f64=second == "f64_packed")
    assert sorted(X["lens"]) == sorted(Y["lens"]) and not np.array_equal(X["lens"], Y["lens"])
    wx, wy = _packed_workspace(dec, "packed", X), _packed_workspace(dec, second, Y)
    torch.cuda.synchronize(dev)
    try:
        rx = _packed_call(dec, "packed", X, wx)
        ry = _packed_call(dec, second, Y, wy)
    finally:
        torch.cuda.synchronize(dev)
    check_packed(rx, X, (case[0], "X"))
    check_packed(ry, Y, (case[0], "Y"))


def test_packed_calls_on_two_streams_with_the_upload_held_back(golden, dev, decoders):
    """The staging buffer's hazard window held open: stream 1 runs a filler (forward passes of a [2, 30000, 361] batch, the
    latency-bound form), then decode_packed(X); decode_packed(Y) follows at once on stream 2.  The upload of X's tables is still queued
    behind the filler when the host stages Y's tables -- asserted: the event behind the filler has not finished when call(X) has
    returned.  Only the wait in pk_stage keeps Y's tables out of X's upload.  The filler is sized in the run: its device time (timing
    events, a warm-up pass) is at least ten times the host time of call(X) (perf_counter, a warm-up call); ten covers a host thread that
    is descheduled on a shared machine."""
    dec = decoders["tonet361"]
    X = _recordings(golden, dev, "tonet361", LENS_361, 0, False)
    Y = _recordings(golden, dev, "tonet361", LENS_361, 5, False)
    assert sorted(X["lens"]) == sorted(Y["lens"]) and not np.array_equal(X["lens"], Y["lens"])
    wx, wy = _packed_workspace(dec, "packed", X), _packed_workspace(dec, "packed", Y)
    FB, FT = 2, 30000
    E_fill = GEN["peaks"](FB, FT, dec.S, seed=5, device=dev)
    st_fill = torch.empty((FB, FT), dtype=torch.int32, device=dev)
    ll_fill = torch.empty((FB,), dtype=torch.float32, device=dev)
    assert dec.forward_family(FB, "group") == "group"
    dec._workspace(FB, FT, 2, None)                                              # the filler's own slot

    def filler():
        dec.decode_into(E_fill, st_fill, ll_fill, None, algo="group", phase="forward", slot=2)

    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    try:
        # warm-up on the streams of the run (code objects, the pinned buffer, the allocator's blocks per stream), then the two measurements
        with torch.cuda.stream(s1):
            _packed_call(dec, "packed", X, wx)
            filler()
        with torch.cuda.stream(s2):
            _packed_call(dec, "packed", Y, wy)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(s1):
            t0 = time.perf_counter()
            _packed_call(dec, "packed", X, wx)
            host_x = time.perf_counter() - t0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            filler()
            e1.record()
        torch.cuda.synchronize(dev)
        fill_ms = e0.elapsed_time(e1)
        n_fill = max(1, math.ceil(10 * host_x * 1e3 / fill_ms))
        assert n_fill <= 256, (host_x, fill_ms)                                  # (a host call of tens of milliseconds: nothing to learn here)
        assert n_fill * fill_ms >= 10 * host_x * 1e3

        with torch.cuda.stream(s1):
            for _ in range(n_fill):
                filler()
            ev = torch.cuda.Event()
            ev.record()
            t0 = time.perf_counter()
            rx = _packed_call(dec, "packed", X, wx)
            host_x_run = time.perf_counter() - t0
            filler_still_running = not ev.query()
        with torch.cuda.stream(s2):
            ry = _packed_call(dec, "packed", Y, wy)
            filler_done_after_y = ev.query()
    finally:
        torch.cuda.synchronize(dev)
        dec._ws_slots.pop(2, None)
    print(f"\n[two streams] staging hazard: filler {n_fill} x {fill_ms:.3f} ms on the device, call(X) {host_x * 1e3:.3f} ms on the host "
          f"(warm-up; {host_x_run * 1e3:.3f} ms in the run); filler unfinished when call(X) returned: {filler_still_running}; finished when "
          f"call(Y) returned (it waits for X's upload): {filler_done_after_y}")
    assert filler_still_running, "premise: the upload of X's tables was still queued when the host began staging Y's"
    check_packed(rx, X, "X on stream 1 behind the filler")
    check_packed(ry, Y, "Y on stream 2")


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. two whole decodes on two streams
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swapped", [False, True], ids=["ckpt-first", "f64-first"])
def test_two_whole_decodes_on_two_streams(golden, dev, decoders, swapped):
    """decode_checkpointed(E1) on one stream and decode_f64(E2) on another, each in its own workspace, enqueued without waiting for
    each other: the float32 oracle for the first, the float64 restatement for the second."""
    dec = decoders["tonet361"]
    A, pi = _params(golden, "tonet361")
    B, T = 3, 500
    c32, c64 = _steps(golden, dev, "tonet361", B, T, [False, False])
    key = ("f64", B, T)
    if key not in _rec_cache:
        _rec_cache[key] = f64_ref.decode_f64_batch(A, pi, c64["E"].cpu().numpy(), c64["lens_h"])
    ref64_s, ref64_l = _rec_cache[key]
    w1 = torch.empty(dec.workspace_bytes_checkpointed(B, T, 64) + 256, dtype=torch.uint8, device=dev)
    w2 = torch.empty(dec.workspace_bytes_f64(B, T) + 256, dtype=torch.uint8, device=dev)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    if swapped:
        s1, s2 = s2, s1

    def ckpt():
        with torch.cuda.stream(s1):
            return dec.decode_checkpointed(c32["E"], segment_frames=64, lengths=c32["lens"], out_dtype=torch.int32, workspace=w1)

    def f64():
        with torch.cuda.stream(s2):
            return dec.decode_f64(c64["E"], lengths=c64["lens"], out_dtype=torch.int32, workspace=w2)

    torch.cuda.synchronize(dev)
    try:
        if swapped:
            r64, r32 = f64(), ckpt()
        else:
            r32, r64 = ckpt(), f64()
    finally:
        torch.cuda.synchronize(dev)
    st, ll = r32[0].cpu().numpy(), r32[1].cpu().numpy()
    assert np.array_equal(st, c32["ref_s"]), "checkpointed: states differ in %d entries" % int(np.sum(st != c32["ref_s"]))
    assert np.array_equal(ll.view(np.uint32), np.ascontiguousarray(c32["ref_l"], np.float32).view(np.uint32)), (ll, c32["ref_l"])
    st, ll = r64[0].cpu().numpy().astype(np.int64), r64[1].cpu().numpy()
    assert np.array_equal(st, ref64_s), "float64: states differ in %d entries" % int(np.sum(st != ref64_s))
    assert ll.dtype == np.float64 and np.array_equal(f64_ref.bits64(ll), f64_ref.bits64(ref64_l)), (ll, ref64_l)
