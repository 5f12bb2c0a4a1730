"""The per-case check of the randomised parity tests: one case of tests/random_cases.py through every entry point of the decoder
on the GPU, each against its reference, bit for bit.  tests/test_gpu_random_parity.py walks the committed table with it and
scripts/fuzz_parity.py walks case(seed, 0), case(seed, 1), ... until its time is up.

host_references(c) is what the comparison is made against and needs no GPU (tests/test_random_cases_host.py uses it for the table's
premises): the C restatement on the stored rows, the float64 restatement where the float64 decodes serve the plan, and the
back-pointers of the session recordings.  check_case(dec, c, dev) raises AssertionError whose text carries (seed, index, entry point,
options): ``random_cases.case(seed, index)`` and this function rerun exactly that.

F32_REFERENCE is the float32 reference of every comparison, a module attribute so that a sensitivity run can put a mutant in its
place (argmax_highest_batch below)."""
import ctypes
import math

import numpy as np

from oracle import viterbi_oracle as vo
from tests import commit_ref as cr
from tests import f64_ref
from tests import inexact
from tests import random_cases as rc
from tests import ring_ref as rr
from tests.common import logits_case

VIT_EUNSUPPORTED = -5
SENTINEL = -7
POISON = 0xFF


def F32_REFERENCE(A, pi, E, lens):
    return vo.decode_c(A, pi, E, lengths=np.asarray(lens, np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# Mutants (host): what the table's inputs must be able to tell from the reference
# ---------------------------------------------------------------------------------------------------------------------
def backtrace_highest(A, rows):
    """MUTANT of inexact.backtrace_reference: the HIGHEST index attaining a maximum, at the last row and at every step."""
    def last_argmax(v):
        return len(v) - 1 - int(np.argmax(v[::-1]))
    n = len(rows)
    path = np.empty(n, np.int64)
    with np.errstate(invalid="ignore"):
        s = last_argmax(rows[-1])
        ll = rows[-1][s]
        path[-1] = s
        for t in range(n - 1, 0, -1):
            s = last_argmax(rows[t - 1] + A[s])
            path[t - 1] = s
    return path, ll


def argmax_highest_batch(A, pi, E, lens):
    """The batch form of the highest-index mutant, shaped like F32_REFERENCE's answer."""
    B, T, _ = E.shape
    st = np.full((B, T), -1, np.int32)
    ll = np.empty(B, np.float32)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            n = int(lens[b])
            p, l = backtrace_highest(np.asarray(A, np.float32), inexact.forward_reference(A, pi, E[b, :n]))
            st[b, :n], ll[b] = p, l
    return st, ll


def decode_f64_in_float32(A, pi, E):
    """MUTANT of f64_ref.decode_f64: the same loop with the running score kept in float32 -> (states, loglik as float64)."""
    with np.errstate(invalid="ignore", over="ignore"):
        rows = inexact.forward_reference(A, pi, E)
        p, l = inexact.backtrace_reference(np.asarray(A, np.float32), rows)
    return p, np.float64(l)


# ---------------------------------------------------------------------------------------------------------------------
# References (host)
# ---------------------------------------------------------------------------------------------------------------------
def host_references(c, sessions=True):
    """{"f32": (states [B, T], loglik [B]), "f64": the same of the float64 restatement or None, "psi": the back-pointers of the session
    recordings or None, "ring": the ring size of the case or None}."""
    sv = rc.served(c)
    out = {"f32": F32_REFERENCE(c["A"], c["pi"], c["E32"], c["lens"]), "f64": None, "psi": None, "ring": None}
    if "f64" in sv:
        out["f64"] = f64_ref.decode_f64_batch(c["A"], c["pi"], c["E32"], c["lens"])
    if sessions and "commit" in sv:
        s = c["session"]
        out["psi"] = [cr.back_pointers(c["A"], c["pi"], c["E32"][b, :int(s["lens"][b])]) for b in range(s["B"])]
        out["ring"] = rr.smallest_ring(out["psi"], per_recording(s["schedule_commit"], s["B"]), s["lookback_ring"])
    return out


def per_recording(schedule, B):
    return [[int(cnt[b]) for _, cnt in schedule] for b in range(B)]


def paths_change(ref_s, ref_l, lens):
    """(songs of at least 17 frames with a finite log-likelihood, those of them whose path changes state)."""
    n = moving = 0
    for b in range(len(lens)):
        k = int(lens[b])
        if k >= 17 and np.isfinite(ref_l[b]):
            n += 1
            moving += bool(np.any(np.diff(ref_s[b, :k]) != 0))
    return n, moving


# ---------------------------------------------------------------------------------------------------------------------
# The GPU side
# ---------------------------------------------------------------------------------------------------------------------
class _Ctx:
    def __init__(self, dec, c, dev):
        import torch
        self.torch, self.dec, self.c, self.dev = torch, dec, c, dev
        self.entry, self.opts = "", {}
        self.runs = 0

    def fail(self, what):
        c = self.c
        raise AssertionError(f"case ({c['seed']}, {c['index']}) entry {self.entry} options {self.opts}: {what}   [{rc.case_id(c)}]")

    def check(self, ok, what):
        if not ok:
            self.fail(what)

    def begin(self, entry, opts, **note):
        """Name the call for a failure's text and set its options (`note`: arguments that are no plan options)."""
        self.entry, self.opts = entry, dict(opts)
        self.dec.set_option("reset", 0)
        for k, v in opts.items():
            self.dec.set_option(k, v)
        self.opts.update(note)

    def end(self):
        self.dec.set_option("reset", 0)

    def ws(self, need):
        """`need` + 256 bytes of workspace, every byte 0xFF."""
        return self.torch.full((int(need) + 256,), POISON, dtype=self.torch.uint8, device=self.dev)

    def compare(self, st, ll, ref_s, ref_l, lens, padded_T=None):
        """st: [B, T] (padded) or a list of per-song arrays; ll [B]; by bits, no NaN."""
        ll = np.ascontiguousarray(ll)
        ref_l = np.ascontiguousarray(ref_l, ll.dtype)
        self.check(not np.isnan(ll).any(), f"NaN log-likelihood {ll}")
        u = np.uint32 if ll.dtype == np.float32 else np.uint64
        bad = np.nonzero(ll.view(u) != ref_l.view(u))[0]
        self.check(bad.size == 0, f"log-likelihood bits differ at song {bad[:1]}: got {ll[bad[:1]]!r}, want {ref_l[bad[:1]]!r}")
        for b in range(len(lens)):
            n = int(lens[b])
            row = np.asarray(st[b])
            d = np.nonzero(row[:n] != ref_s[b][:n])[0]
            self.check(d.size == 0, f"states differ at song {b}, frame {d[:1]} of {n}: got {row[d[:1]]}, want {np.asarray(ref_s[b])[d[:1]]}; "
                                    f"{d.size} frames of this song differ")
            if padded_T is not None:
                self.check(bool((row[n:padded_T] == -1).all()), f"states past the end of song {b} are not -1")
        self.runs += 1

    def refused(self, call, *outputs):
        """`call` must raise ViterbiHipError; `outputs`: (tensor, its sentinel copy) pairs that must be unchanged."""
        from viterbi_spl_amd._lib import ViterbiHipError
        try:
            call()
        except ViterbiHipError:
            pass
        else:
            self.fail("served() says refused, the call decoded")
        self.torch.cuda.synchronize()
        for t, keep in outputs:
            self.check(bool(self.torch.equal(t, keep)), "a refused call wrote to its outputs")

    def raw_refused(self, name, args_of):
        """The C entry point `name` with sentinel outputs: VIT_EUNSUPPORTED, outputs untouched.  args_of(ws_ptr, ws_bytes, states_ptr,
        loglik_ptr) -> the arguments behind the plan and in front of the stream."""
        from viterbi_spl_amd import _lib
        torch = self.torch
        ws = self.ws(1 << 20)
        ws_ptr = (ws.data_ptr() + 255) & ~255
        states = torch.full((1 << 16,), SENTINEL, dtype=torch.int32, device=self.dev)
        loglik = torch.full((64,), float(SENTINEL), dtype=torch.float64, device=self.dev)
        with torch.cuda.device(self.dev):
            rc_ = getattr(_lib.load(), name)(self.dec._plan, *args_of(ws_ptr, 1 << 20, states.data_ptr(), loglik.data_ptr()),
                                             torch.cuda.current_stream(self.dev).cuda_stream)
        torch.cuda.synchronize()
        self.check(rc_ == VIT_EUNSUPPORTED, f"{name} answered {rc_}, the header says VIT_EUNSUPPORTED ({VIT_EUNSUPPORTED})")
        self.check(bool((states == SENTINEL).all()) and bool((loglik == float(SENTINEL)).all()) and bool((ws == POISON).all()),
                   f"{name} refused the call and wrote to its outputs or its workspace")


def _builder(mode, n_bins):
    """(obs parameters of decode_logits, the stand-alone builder with the same arguments): the reference's three geometries."""
    from viterbi_spl_amd import ViterbiDecoder
    from viterbi_spl_amd import emissions as em
    if mode == 0:
        obs = ViterbiDecoder.obs_params("shaun", n_bins, 5, math.log(0.32 / (1.0 - 0.32)), math.log(0.8 / (1.0 - 0.8)), 2.0)
        return obs, lambda x: em.shaun_log_emissions(x, 0.32, 5)
    if mode == 1:
        return ViterbiDecoder.obs_params("softmax", n_bins, 15), lambda x: em.softmax_log_emissions(x, 15)
    v = np.float32(0.32)
    obs = ViterbiDecoder.obs_params("softmax_scaled", n_bins, 5, float(np.log(v / (np.float32(1) - v))))
    return obs, lambda x: em.softmax_scaled_log_emissions(x, 0.32, None, 5)


def _budget(full_need, size_of, rung, above):
    """A budget at the rung `size_of(rung)` (the whole history where the entry has no segments): exactly there, or one byte below."""
    at = int(size_of(rung)) or int(full_need)
    return min(at, int(full_need)) - (0 if above else 1)


def check_case(dec, c, dev, refs=None, guarded=False):
    """Every entry point on case `c`; -> the number of decodes compared.  `dec`: a ViterbiDecoder of (c["A"], c["pi"]) on `dev`."""
    import torch
    from viterbi_spl_amd import _lib
    from viterbi_spl_amd._lib import ViterbiHipError
    x = _Ctx(dec, c, dev)
    hp, sv = c["hp"], rc.served(c)
    refs = refs or host_references(c)
    ref_s, ref_l = refs["f32"]
    A, pi, B, T, S, lens = c["A"], c["pi"], c["B"], c["T"], c["S"], c["lens"]
    E = torch.from_numpy(c["E16"] if c["f16"] else c["E32"]).to(dev)
    dt = _lib.VIT_F16 if c["f16"] else _lib.VIT_F32
    lens_t = torch.from_numpy(lens).to(dev)
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum(lens)
    N = int(off[-1])
    Ep = torch.cat([E[b, :int(lens[b])] for b in range(B)], dim=0).contiguous()
    ref_packed = [ref_s[b, :int(lens[b])] for b in range(B)]

    def unpack(sp):
        sp = sp.cpu().numpy()
        return [sp[off[b]:off[b + 1]] for b in range(B)]

    # ---- served-set agreement on the size queries
    x.begin("size queries", {})
    obs, build = _builder(c["obs_mode"], S - 1)
    sizes = {
        "checkpointed": dec._need("checkpointed", False, B, T, 64), "packed": dec._need("packed", False, B, N),
        "packed_checkpointed": dec._need("packed_checkpointed", False, B, off.ctypes.data, 64),
        "packed_bounded": dec._need("packed_bounded", False, B, off.ctypes.data, 64),
        "f64": dec._need("f64", False, B, T), "f64_checkpointed": dec._need("f64_checkpointed", False, B, T, 64),
        "f64_packed": dec._need("f64_packed", False, B, N),
        "f64_packed_checkpointed": dec._need("f64_packed_checkpointed", False, B, off.ctypes.data, 64),
        "f64_packed_bounded": dec._need("f64_packed_checkpointed", False, B, off.ctypes.data, 64),
        "logits": dec.workspace_bytes_logits(obs, B, T), "logits_checkpointed": dec.workspace_bytes_logits_checkpointed(obs, B, T, 64),
        "stream": dec.workspace_bytes_stream(c["session"]["B"], 64), "commit": dec._need("stream_commit", False, c["session"]["B"]),
        "ring": dec.workspace_bytes_stream_ring(c["session"]["B"], 128),
    }
    for e, need in sizes.items():
        x.check((need > 0) == (e in sv), f"served() says {e in sv} for {e}, its size query answers {need}")

    # ---- decode: every form
    for algo, o in c["decode_forms"]:
        name = "decode:" + algo
        algo_, o = ("wave", dict(o, wave_history=2)) if algo == "wave-half" else (algo, o)
        x.begin(name, o)
        ok = {"auto": True, "dense": True, "group": rc.group_ok(hp), "wave": bool(hp.ok and hp.wave_ok)}[algo_]
        if algo == "wave-half" and ok and T >= 2:          # the library says whether the plan has a half history: its size query,
            ok = dec.history_mode(B, 1024, "wave") == "half"   # at a length where the rows outweigh the tables
        states = torch.full((B, T), SENTINEL, dtype=torch.int32, device=dev)
        loglik = torch.full((B,), float(SENTINEL), dtype=torch.float32, device=dev)
        if not ok:
            x.refused(lambda: dec.decode_into(E, states, loglik, lens_t, algo_), (states, states.clone()), (loglik, loglik.clone()))
        else:
            dec._workspace(B, T, 0, algo_)
            dec._ws.fill_(POISON)
            dec.decode_into(E, states, loglik, lens_t, algo_)
            torch.cuda.synchronize()
            x.compare(states.cpu().numpy(), loglik.cpu().numpy(), ref_s, ref_l, lens, T)
        x.end()

    if guarded:                                            # the outputs of one decode between guards
        from tests import guarded as gd
        x.begin("decode:auto guarded", {})
        sa, la = gd.Arena(B * T * 4, dev), gd.Arena(B * 4, dev, lead=4)
        dec._workspace(B, T, 0, "auto")
        dec._ws.fill_(POISON)
        dec.decode_into(E, sa.view(torch.int32, (B, T)), la.view(torch.float32, (B,)), lens_t, "auto")
        torch.cuda.synchronize()
        try:
            gd.assert_decode_outputs(sa, la, ref_s, ref_l, lens, T)
        except AssertionError as e:
            x.fail(str(e))
        x.runs += 1
        x.end()

    # ---- decode under a budget
    x.begin("decode:max_workspace_bytes", {})
    rung, above = c["budget"]["decode"]
    budget = _budget(dec.workspace_bytes(B, T, "auto"), lambda K: dec._need("checkpointed", False, B, T, K), rung, above)
    x.opts = {"max_workspace_bytes": budget}
    try:
        mode = dec.plan_workspace(B, T, "auto", budget)
    except ViterbiHipError:
        mode = None
    if mode is None:
        x.refused(lambda: dec.decode(E, lengths=lens_t, out_dtype=torch.int32, max_workspace_bytes=budget))
    else:
        x.check(mode["workspace_bytes"] <= budget, f"plan_workspace answers {mode} for a budget of {budget}")
        st, ll = dec.decode(E, lengths=lens_t, out_dtype=torch.int32, max_workspace_bytes=budget)
        torch.cuda.synchronize()
        x.compare(st.cpu().numpy(), ll.cpu().numpy(), ref_s, ref_l, lens, T)
    dec._ws = None
    x.end()

    # ---- the float32 entry points with a workspace of their own
    def padded(entry, K, call, size):
        x.begin(entry, dict(c["options"][entry]))
        x.opts["segment_frames"] = K
        if entry in sv:
            st, ll = call(x.ws(size()))
            torch.cuda.synchronize()
            x.compare(st.cpu().numpy(), ll.cpu().numpy(), ref_s, ref_l, lens, T)
        x.end()

    def packed(entry, K, call, size, want_s=ref_packed, want_l=ref_l):
        x.begin(entry, dict(c["options"][entry]))
        if K:
            x.opts["segment_frames"] = K
        if entry in sv:
            sp, ll = call(x.ws(size()))
            torch.cuda.synchronize()
            x.compare(unpack(sp), ll.cpu().numpy(), want_s, want_l, lens)
        x.end()

    K = c["K"]
    padded("checkpointed", K["checkpointed"], lambda ws: dec.decode_checkpointed(E, K["checkpointed"], lens_t, torch.int32, ws),
           lambda: dec.workspace_bytes_checkpointed(B, T, K["checkpointed"]))
    packed("packed", 0, lambda ws: dec.decode_packed(Ep, off, torch.int32, ws), lambda: dec.workspace_bytes_packed(B, N))
    packed("packed_checkpointed", K["packed_checkpointed"],
           lambda ws: dec.decode_packed_checkpointed(Ep, off, K["packed_checkpointed"], torch.int32, ws),
           lambda: dec.workspace_bytes_packed_checkpointed(off, K["packed_checkpointed"]))
    packed("packed_bounded", K["packed_bounded"], lambda ws: dec.decode_packed_bounded(Ep, off, K["packed_bounded"], torch.int32, ws),
           lambda: dec.workspace_bytes_packed_bounded(off, K["packed_bounded"]))
    if "checkpointed" not in sv:
        x.begin("checkpointed", {})
        x.raw_refused("vit_decode_checkpointed", lambda w, n, s, l: (E.data_ptr(), dt, B, T, lens_t.data_ptr(), w, n, s, l, 64))
    for e in ("packed_checkpointed", "packed_bounded"):
        if e not in sv:
            x.begin(e, {})
            x.raw_refused("vit_decode_" + e, lambda w, n, s, l: (Ep.data_ptr(), dt, B, off.ctypes.data, w, n, s, l, 64))
    if "packed" not in sv:
        x.begin("packed", {})
        x.raw_refused("vit_decode_packed", lambda w, n, s, l: (Ep.data_ptr(), dt, B, off.ctypes.data, w, n, s, l))
    x.end()

    if "packed" in sv:
        x.begin("packed:max_workspace_bytes", {})
        rung, above = c["budget"]["packed"]
        entry = "packed_checkpointed" if hp.ok and hp.wave_ok else "packed_bounded"
        plan_of = dec.plan_workspace_packed if hp.ok and hp.wave_ok else dec.plan_workspace_packed_bounded
        budget = _budget(sizes["packed"], lambda K_: dec._need(entry, False, B, off.ctypes.data, K_), rung, above)
        x.opts = {"max_workspace_bytes": budget}
        try:
            mode = plan_of(off, budget)
        except ViterbiHipError:
            mode = None
        if mode is None:
            x.refused(lambda: dec.decode_packed(Ep, off, torch.int32, None, budget))
        else:
            x.check(mode["workspace_bytes"] <= budget, f"the plan answers {mode} for a budget of {budget}")
            sp, ll = dec.decode_packed(Ep, off, torch.int32, x.ws(mode["workspace_bytes"]), budget)
            torch.cuda.synchronize()
            x.compare(unpack(sp), ll.cpu().numpy(), ref_packed, ref_l, lens)
        x.end()

    # ---- the float64 decodes
    if "f64" in sv:
        r64_s, r64_l = refs["f64"]
        r64_packed = [r64_s[b, :int(lens[b])] for b in range(B)]

        def padded64(entry, call, size, K_=0):
            x.begin(entry, dict(c["options"][entry]))
            if K_:
                x.opts["segment_frames"] = K_
            st, ll = call(x.ws(size()))
            torch.cuda.synchronize()
            x.compare(st.cpu().numpy(), ll.cpu().numpy(), r64_s, r64_l, lens, T)
            x.end()

        padded64("f64", lambda ws: dec.decode_f64(E, lens_t, torch.int32, ws), lambda: dec.workspace_bytes_f64(B, T))
        padded64("f64_checkpointed", lambda ws: dec.decode_f64_checkpointed(E, K["f64_checkpointed"], lens_t, torch.int32, ws),
                 lambda: dec.workspace_bytes_f64_checkpointed(B, T, K["f64_checkpointed"]), K["f64_checkpointed"])
        packed("f64_packed", 0, lambda ws: dec.decode_f64_packed(Ep, off, torch.int32, ws), lambda: dec.workspace_bytes_f64_packed(B, N),
               r64_packed, r64_l)
        packed("f64_packed_checkpointed", K["f64_packed_checkpointed"],
               lambda ws: dec.decode_f64_packed_checkpointed(Ep, off, K["f64_packed_checkpointed"], torch.int32, ws),
               lambda: dec.workspace_bytes_f64_packed_checkpointed(off, K["f64_packed_checkpointed"]), r64_packed, r64_l)
        # decode_f64_packed_bounded and the budget of decode_f64: a rung of their ladders, from either side
        x.begin("f64_packed_bounded", dict(c["options"]["f64_packed_bounded"]))
        rung, above = c["budget"]["f64"]
        budget = _budget(dec.workspace_bytes_f64_packed(B, N), lambda K_: dec._need("f64_packed_checkpointed", False, B, off.ctypes.data, K_), rung, above)
        x.opts["max_workspace_bytes"] = budget
        try:
            mode = dec.plan_workspace_f64_packed_bounded(off, budget)
        except ViterbiHipError:
            mode = None
        if mode is None:
            x.refused(lambda: dec.decode_f64_packed_bounded(Ep, off, budget, torch.int32))
        else:
            x.check(mode["workspace_bytes"] <= budget, f"the plan answers {mode} for a budget of {budget}")
            sp, ll = dec.decode_f64_packed_bounded(Ep, off, budget, torch.int32, x.ws(mode["workspace_bytes"]))
            torch.cuda.synchronize()
            x.compare(unpack(sp), ll.cpu().numpy(), r64_packed, r64_l, lens)
        x.end()
        x.begin("f64:max_workspace_bytes", dict(c["options"]["f64"]))
        budget = _budget(dec.workspace_bytes_f64(B, T), lambda K_: dec._need("f64_checkpointed", False, B, T, K_), rung, above)
        x.opts["max_workspace_bytes"] = budget
        try:
            mode = dec.plan_workspace_f64(B, T, budget)
        except ViterbiHipError:
            mode = None
        if mode is None:
            x.refused(lambda: dec.decode_f64(E, lens_t, torch.int32, None, budget))
        else:
            x.check(mode["workspace_bytes"] <= budget, f"the plan answers {mode} for a budget of {budget}")
            st, ll = dec.decode_f64(E, lens_t, torch.int32, x.ws(mode["workspace_bytes"]), budget)
            torch.cuda.synchronize()
            x.compare(st.cpu().numpy(), ll.cpu().numpy(), r64_s, r64_l, lens, T)
        dec._ws = None
        x.end()
    else:
        x.begin("f64", {})
        x.raw_refused("vit_decode_f64", lambda w, n, s, l: (E.data_ptr(), dt, B, T, lens_t.data_ptr(), w, n, s, l))
        x.begin("f64_checkpointed", {})
        x.raw_refused("vit_decode_f64_checkpointed", lambda w, n, s, l: (E.data_ptr(), dt, B, T, lens_t.data_ptr(), w, n, s, l, 64))
        x.begin("f64_packed", {})
        x.raw_refused("vit_decode_f64_packed", lambda w, n, s, l: (Ep.data_ptr(), dt, B, off.ctypes.data, w, n, s, l))
        x.begin("f64_packed_checkpointed", {})
        x.raw_refused("vit_decode_f64_packed_checkpointed", lambda w, n, s, l: (Ep.data_ptr(), dt, B, off.ctypes.data, w, n, s, l, 64))
        x.end()

    # ---- the fused decodes: the rows written through emissions_out are the stand-alone builder's, the path is the oracle's on those rows
    op = ctypes.byref(dec._obs_struct(obs))
    if "logits" in sv:
        cols = S if c["obs_mode"] == 1 else S - 1
        X = torch.from_numpy(logits_case(c["logits_seed"], B * T, cols)).to(dev).view(B, T, cols).contiguous()
        rows = build(X)
        torch.cuda.synchronize()
        rows_h = rows.cpu().numpy()
        lg_s, lg_l = F32_REFERENCE(A, pi, rows_h, lens)
        x.begin("logits", dict(c["options"]["logits"]))
        x.opts["obs_mode"] = c["obs_mode"]
        eo = torch.full((B, T, S), 7.0, dtype=torch.float32, device=dev)
        st, ll = dec.decode_logits(X, obs, lens_t, torch.int32, eo, x.ws(dec.workspace_bytes_logits(obs, B, T)))
        torch.cuda.synchronize()
        eo_h = eo.cpu().numpy()
        for b in range(B):
            n = int(lens[b])
            x.check(np.array_equal(eo_h[b, :n].view(np.uint32), rows_h[b, :n].view(np.uint32)), f"emissions_out of song {b} differs from the builder's rows")
            x.check(bool((eo_h[b, n:] == 7.0).all()), f"emissions_out of song {b} was written past its length")
        x.compare(st.cpu().numpy(), ll.cpu().numpy(), lg_s, lg_l, lens, T)
        x.end()
        if "logits_checkpointed" in sv:
            Kl = K["logits_checkpointed"]
            x.begin("logits_checkpointed", dict(c["options"]["logits_checkpointed"]))
            x.opts.update(obs_mode=c["obs_mode"], segment_frames=Kl)
            st, ll = dec.decode_logits_checkpointed(X, obs, Kl, lens_t, torch.int32, x.ws(dec.workspace_bytes_logits_checkpointed(obs, B, T, Kl)))
            torch.cuda.synchronize()
            x.compare(st.cpu().numpy(), ll.cpu().numpy(), lg_s, lg_l, lens, T)
            x.end()
            x.begin("logits:max_workspace_bytes", {})
            rung, above = c["budget"]["logits"]
            budget = _budget(dec.workspace_bytes_logits(obs, B, T), lambda K_: dec.workspace_bytes_logits_checkpointed(obs, B, T, K_), rung, above)
            x.opts = {"obs_mode": c["obs_mode"], "max_workspace_bytes": budget}
            try:
                mode = dec.plan_workspace_logits(obs, B, T, budget)
            except ViterbiHipError:
                mode = None
            if mode is None:
                x.refused(lambda: dec.decode_logits(X, obs, lens_t, torch.int32, None, None, budget))
            else:
                x.check(mode["workspace_bytes"] <= budget, f"the plan answers {mode} for a budget of {budget}")
                st, ll = dec.decode_logits(X, obs, lens_t, torch.int32, None, x.ws(mode["workspace_bytes"]), budget)
                torch.cuda.synchronize()
                x.compare(st.cpu().numpy(), ll.cpu().numpy(), lg_s, lg_l, lens, T)
            x.end()
    elif S >= 32:
        cols = S if c["obs_mode"] == 1 else S - 1
        X = torch.zeros((B, T, cols), dtype=torch.float32, device=dev)
        x.begin("logits", {}, obs_mode=c["obs_mode"])
        x.raw_refused("vit_decode_logits", lambda w, n, s, l: (X.data_ptr(), op, B, T, lens_t.data_ptr(), w, n, None, s, l))
        x.begin("logits_checkpointed", {}, obs_mode=c["obs_mode"])
        x.raw_refused("vit_decode_logits_checkpointed", lambda w, n, s, l: (X.data_ptr(), op, B, T, lens_t.data_ptr(), w, n, s, l, 64))
        x.end()

    _sessions(x, E, refs)
    return x.runs


def _chunk(x, E, pos, n, cnt):
    """The chunk tensor of one append: recording b's rows pos[b] .. pos[b] + cnt[b] - 1, NaN in every row no recording takes."""
    torch = x.torch
    buf = torch.full((len(cnt), n, E.shape[2]), float("nan"), dtype=E.dtype, device=x.dev)
    for b in range(len(cnt)):
        buf[b, :int(cnt[b])] = E[b, int(pos[b]):int(pos[b] + cnt[b])]
    return buf


def _sessions(x, E, refs):
    torch, dec, c, dev = x.torch, x.dec, x.c, x.dev
    from viterbi_spl_amd._lib import ViterbiHipError  # noqa: F401
    sv = rc.served(c)
    s = c["session"]
    Bs, slens = s["B"], s["lens"]
    A, pi = c["A"], c["pi"]
    cap = int(slens.max()) + s["cap_extra"]
    if "stream" not in sv:
        x.begin("stream", {})
        x.refused(lambda: dec.stream(Bs, cap))
        x.begin("ring", {})
        x.refused(lambda: dec.stream(Bs, ring_frames=128))
        x.end()
        return
    # linear session: after every append, decode() is the oracle on the frames each recording holds so far
    x.begin("stream", dict(c["options"]["stream"]))
    if "commit" not in sv:
        x.opts.pop("backtrace_form", None)                  # (the lane form is a banded plan's)
        x.begin("stream", x.opts)
    st = dec.stream(Bs, cap, workspace=x.ws(dec.workspace_bytes_stream(Bs, cap)))
    pos = np.zeros(Bs, np.int64)
    for k, (n, cnt) in enumerate(s["schedule"]):
        st.append(_chunk(x, E, pos, n, cnt), counts=cnt)
        pos = pos + cnt
        x.opts["append"] = k
        x.check(np.array_equal(st.lengths, pos), f"lengths {st.lengths} after append {k}, want {pos}")
        got_s, got_l = st.decode(out_dtype=torch.int32)
        torch.cuda.synchronize()
        want_s, want_l = F32_REFERENCE(A, pi, c["E32"][:Bs, :int(pos.max())], pos)
        x.compare(got_s.cpu().numpy(), got_l.cpu().numpy(), want_s, want_l, pos, int(pos.max()))
    st.close()
    x.end()

    if "commit" not in sv:                                  # step plans: a session, no commit point
        x.begin("commit", {})
        st = dec.stream(Bs, cap)
        st.append(E[:Bs, :int(slens.min())].contiguous())
        states = torch.full((Bs, cap), SENTINEL, dtype=torch.int32, device=dev)
        committed = torch.full((Bs,), SENTINEL, dtype=torch.int64, device=dev)
        x.refused(lambda: st.commit_into(states, committed), (states, states.clone()), (committed, committed.clone()))
        st.close()
        x.begin("ring", {})
        x.refused(lambda: dec.stream(Bs, ring_frames=128))
        x.end()
        return

    psi = refs["psi"]
    sched = s["schedule_commit"]
    whole_s, whole_l = F32_REFERENCE(A, pi, c["E32"][:Bs, :int(slens.max())], slens)
    # commit on a linear session, every `cadence`-th append and after the last
    x.begin("commit", dict(c["options"]["commit"]))
    L = s["lookback"]
    x.opts.update(max_lookback=L, cadence=s["cadence"])
    st = dec.stream(Bs, cap, workspace=x.ws(dec.workspace_bytes_stream(Bs, cap)))
    states = torch.full((Bs, cap), SENTINEL, dtype=torch.int32, device=dev)
    committed = torch.full((Bs,), SENTINEL, dtype=torch.int64, device=dev)
    pos = np.zeros(Bs, np.int64)
    f = np.zeros(Bs, np.int64)
    for k, (n, cnt) in enumerate(sched):
        st.append(_chunk(x, E, pos, n, cnt), counts=cnt)
        pos = pos + cnt
        if (k + 1) % s["cadence"] and k + 1 < len(sched):
            continue
        x.opts["append"] = k
        st.commit_into(states, committed, L)
        torch.cuda.synchronize()
        got_f, got = committed.cpu().numpy(), states.cpu().numpy()
        for b in range(Bs):
            f2, want = cr.commit(psi[b], int(pos[b]), int(f[b]), L)
            x.check(int(got_f[b]) == f2, f"recording {b}: frontier {int(got_f[b])} after {int(pos[b])} frames, tests/commit_ref says {f2} (from {int(f[b])})")
            x.check(np.array_equal(got[b, int(f[b]):f2], want), f"recording {b}: the states committed for frames [{int(f[b])}, {f2}) differ")
            x.check(bool((got[b, f2:] == SENTINEL).all()), f"recording {b}: written past the frontier {f2}")
            f[b] = f2
    got_s, got_l = st.decode(out_dtype=torch.int32)
    torch.cuda.synchronize()
    x.compare(got_s.cpu().numpy(), got_l.cpu().numpy(), whole_s, whole_l, slens, int(slens.max()))
    got = states.cpu().numpy()
    for b in range(Bs):
        x.check(np.array_equal(got[b, :int(f[b])], whole_s[b, :int(f[b])]), f"recording {b}: the committed prefix is not the whole decode's")
    st.close()
    x.end()

    # ring session: commit and acknowledge after every append, then the tail
    R = refs["ring"]
    if R is None:
        return
    x.begin("ring", dict(c["options"]["ring"]))
    L = s["lookback_ring"]
    x.opts.update(max_lookback=L, ring_frames=R)
    replays = [rr.replay(psi[b], per_recording(sched, Bs)[b], R, L) for b in range(Bs)]
    st = dec.stream(Bs, ring_frames=R, workspace=x.ws(dec.workspace_bytes_stream_ring(Bs, R)))
    pos = np.zeros(Bs, np.int64)
    parts = [[] for _ in range(Bs)]
    gc = np.zeros(Bs, np.int64)
    for k, (n, cnt) in enumerate(sched):
        st.append(_chunk(x, E, pos, n, cnt), counts=cnt)
        pos = pos + cnt
        x.opts["append"] = k
        stride = max(1, min(int(pos.max()), R))
        states = torch.full((Bs, stride), SENTINEL, dtype=torch.int32, device=dev)
        first = torch.full((Bs,), -9, dtype=torch.int64, device=dev)
        committed = torch.full((Bs,), -9, dtype=torch.int64, device=dev)
        st.commit_rel_into(states, first, committed, max_lookback=L)
        torch.cuda.synchronize()
        gf, gc, gs = first.cpu().numpy(), committed.cpu().numpy(), states.cpu().numpy()
        for b in range(Bs):
            want = replays[b][k]
            x.check(int(gf[b]) == want["f0"] and int(gc[b]) == want["f"],
                    f"recording {b}: frontiers ({int(gf[b])}, {int(gc[b])}), tests/ring_ref says ({want['f0']}, {want['f']})")
            m = want["f"] - want["f0"]
            x.check(np.array_equal(gs[b, :m], want["states"]), f"recording {b}: the states of frames [{want['f0']}, {want['f']}) differ")
            x.check(bool((gs[b, m:] == SENTINEL).all()), f"recording {b}: written outside the committed range")
            parts[b].append(gs[b, :m].copy())
        st.ack(gc)
    x.opts["append"] = "tail"
    stride = max(1, min(int(pos.max()), R))
    states = torch.full((Bs, stride), SENTINEL, dtype=torch.int32, device=dev)
    first = torch.full((Bs,), -9, dtype=torch.int64, device=dev)
    loglik = torch.full((Bs,), float("nan"), dtype=torch.float32, device=dev)
    st.tail_into(states, first, loglik)
    torch.cuda.synchronize()
    gs = states.cpu().numpy()
    x.check(np.array_equal(first.cpu().numpy(), gc), "the tail starts at another frontier than the last commit's")
    for b in range(Bs):
        m = int(pos[b] - gc[b])
        x.check(bool((gs[b, m:] == SENTINEL).all()), f"recording {b}: the tail wrote outside [0, n - f)")
        parts[b].append(gs[b, :m].copy())
    x.compare([np.concatenate(p) for p in parts], loglik.cpu().numpy(), whole_s, whole_l, slens)
    st.close()
    x.end()
