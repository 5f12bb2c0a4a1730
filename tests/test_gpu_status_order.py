"""Which refusal wins when a call carries two defects at once: vit_decode_checkpointed, vit_decode_packed,
vit_decode_packed_checkpointed, vit_decode_packed_bounded and vit_decode_logits on uploaded plans -- tonet361 (wave form), jdc722
(floor form), durrieu722 (step form) and dense97 (served by none of them).  Three songs of 65, 130 and 1 frames, segments of 64.
Every such call is refused before anything is enqueued.  The expected codes are the order of the checks in csrc/capi.hip as callers
have met it so far (first the arguments, then the plan, then the offsets, then the sizes); then one valid decode per plan shows
that the refused calls left nothing behind in the plan."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -4, -5
LENS = np.array([65, 130, 1], np.int64)
OFF = np.array([0, 65, 195, 196], np.int64)
BAD_OFF = np.array([0, 65, 65, 196], np.int64)        # an empty recording
B, T, N, K = 3, 130, 196, 64
PLANS = ["tonet361", "jdc722", "durrieu722", "dense97"]
BIG = 1 << 28


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


class Call:
    """One plan on the device with buffers for every entry point; each method returns the status of one raw C call."""

    def __init__(self, golden, dev, name):
        self.lib = _lib.load()
        self.name = name
        self.A, self.pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
        self.dec = ViterbiDecoder(self.A, self.pi, dev)
        self.S = self.dec.S
        self.E = synth.emissions_peaks(B, T, self.S, seed=5, device=dev)
        self.Ep = torch.cat([self.E[b, :int(n)] for b, n in enumerate(LENS)], dim=0).contiguous()
        self.lengths = torch.from_numpy(LENS).to(dev)
        self.X = synth.pitch_logits(B, T, self.S - 1, seed=3, device=dev)
        self.obs = _lib.ObsParams(0, self.S - 1, 5, 0.0, 1.0, 2.0, None)
        self.buf = torch.empty(BIG + 512, dtype=torch.uint8, device=dev)
        self.ws = (self.buf.data_ptr() + 255) & ~255
        self.states = torch.full((B * T,), 12345, dtype=torch.int32, device=dev)
        self.loglik = torch.full((B,), 7.0, dtype=torch.float32, device=dev)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.states == 12345).all()) and bool((self.loglik == 7.0).all())

    def need(self, entry):
        lib, p = self.lib, self.dec._plan
        return {"checkpointed": lambda: lib.vit_workspace_bytes_checkpointed(p, B, T, K),
                "packed": lambda: lib.vit_workspace_bytes_packed(p, B, N),
                "packed_checkpointed": lambda: lib.vit_workspace_bytes_packed_checkpointed(p, B, OFF.ctypes.data, K),
                "packed_bounded": lambda: lib.vit_workspace_bytes_packed_bounded(p, B, OFF.ctypes.data, K),
                "logits": lambda: lib.vit_workspace_bytes_logits(p, ctypes.byref(self.obs), B, T)}[entry]()

    def run(self, entry, nB=B, off=OFF, logE=True, ws=None, ws_bytes=BIG, dt=_lib.VIT_F32, seg=K, mode=0):
        lib, p = self.lib, self.dec._plan
        ws = self.ws if ws is None else ws
        st, ll = self.states.data_ptr(), self.loglik.data_ptr()
        if entry == "checkpointed":
            return lib.vit_decode_checkpointed(p, self.E.data_ptr() if logE else None, dt, nB, T, self.lengths.data_ptr(), ws, ws_bytes, st, ll, seg, None)
        if entry == "logits":
            obs = _lib.ObsParams(mode, self.S - 1, 5, 0.0, 1.0, 2.0, None)
            return lib.vit_decode_logits(p, self.X.data_ptr() if logE else None, ctypes.byref(obs), nB, T, self.lengths.data_ptr(), ws, ws_bytes, None, st, ll, None)
        e = self.Ep.data_ptr() if logE else None
        if entry == "packed":
            return lib.vit_decode_packed(p, e, dt, nB, off.ctypes.data, ws, ws_bytes, st, ll, None)
        fn = {"packed_checkpointed": lib.vit_decode_packed_checkpointed, "packed_bounded": lib.vit_decode_packed_bounded}[entry]
        return fn(p, e, dt, nB, off.ctypes.data, ws, ws_bytes, st, ll, seg, None)


@pytest.fixture(scope="module")
def calls(golden, dev):
    return {name: Call(golden, dev, name) for name in PLANS}


# the plans an entry point serves; every other plan of PLANS is refused with VIT_EUNSUPPORTED once its arguments are in order
SERVED = {"checkpointed": ["tonet361", "jdc722", "durrieu722"], "packed": ["tonet361", "jdc722", "durrieu722"],
          "packed_checkpointed": ["tonet361"], "packed_bounded": ["tonet361", "jdc722", "durrieu722"], "logits": ["tonet361"]}
PACKED = ["packed", "packed_checkpointed", "packed_bounded"]
BUDGETED = ["checkpointed", "packed_checkpointed", "packed_bounded"]


@pytest.mark.parametrize("entry", list(SERVED))
def test_the_sizes_agree_with_who_is_served(calls, entry):
    for name in PLANS:
        assert (calls[name].need(entry) > 0) == (name in SERVED[entry]), (entry, name)


@pytest.mark.parametrize("entry", PACKED)
def test_unserved_plan_and_bad_offsets(calls, entry):
    """The plan is asked before the offsets are read."""
    for name in PLANS:
        if name not in SERVED[entry]:
            assert calls[name].run(entry, off=BAD_OFF) == EUNSUPPORTED, (entry, name)
            assert calls[name].run(entry, off=BAD_OFF, ws_bytes=0) == EUNSUPPORTED, (entry, name)
            assert calls[name].untouched()


@pytest.mark.parametrize("entry", PACKED)
def test_bad_offsets_and_no_workspace(calls, entry):
    """The offsets are validated before the workspace is measured."""
    for name in SERVED[entry]:
        assert calls[name].run(entry, off=BAD_OFF, ws_bytes=0) == EINVAL, (entry, name)
        assert calls[name].run(entry, off=BAD_OFF, ws_bytes=0, logE=False) == EINVAL, (entry, name)
        assert calls[name].untouched()


@pytest.mark.parametrize("entry", list(SERVED))
def test_null_emissions_and_no_workspace(calls, entry):
    """A null emission (logits) pointer is an invalid argument, not a small workspace -- for a plan that is served; a plan that is
    not is refused first by the packed budgeted pair, by vit_decode_packed and by vit_decode_logits, while vit_decode_checkpointed
    looks at its pointers before it looks at the plan."""
    for name in PLANS:
        served = name in SERVED[entry]
        want = EINVAL if served or entry == "checkpointed" else EUNSUPPORTED
        assert calls[name].run(entry, logE=False, ws_bytes=0) == want, (entry, name)
        assert calls[name].untouched()


@pytest.mark.parametrize("entry", BUDGETED)
def test_short_segment_and_unserved_plan(calls, entry):
    """segment_frames is an argument: refused before the plan is asked."""
    for name in PLANS:
        assert calls[name].run(entry, seg=63) == EINVAL, (entry, name)
        assert calls[name].run(entry, seg=63, ws_bytes=0) == EINVAL, (entry, name)
        assert calls[name].untouched()


@pytest.mark.parametrize("entry", list(SERVED))
def test_bad_dtype_and_unserved_plan(calls, entry):
    """The emission storage type (vit_decode_logits: the builder mode) is an argument: refused before the plan is asked."""
    for name in PLANS:
        assert calls[name].run(entry, dt=7, mode=3) == EINVAL, (entry, name)
        assert calls[name].untouched()


@pytest.mark.parametrize("entry", list(SERVED))
def test_empty_batch(calls, entry):
    """B = 0 with a null emission pointer and no workspace bytes: nothing to do is not an error for a plan that is served
    (vit_decode_checkpointed refuses the null pointer first, as vit_decode does); a plan that is not served is still refused."""
    off0 = np.zeros(1, np.int64)
    for name in PLANS:
        served = name in SERVED[entry]
        want = EINVAL if entry == "checkpointed" else (OK if served else EUNSUPPORTED)
        assert calls[name].run(entry, nB=0, off=off0, logE=False, ws_bytes=0) == want, (entry, name)
        assert calls[name].untouched()


@pytest.mark.parametrize("entry", list(SERVED))
def test_workspace_one_byte_short_or_misaligned(calls, entry):
    for name in SERVED[entry]:
        c = calls[name]
        need = int(c.need(entry))
        assert 0 < need <= BIG
        assert c.run(entry, ws_bytes=need - 1) == EWORKSPACE, (entry, name)
        assert c.run(entry, ws=c.ws + 1, ws_bytes=need) == EINVAL, (entry, name)
        assert c.run(entry, ws=c.ws + 1, ws_bytes=need - 1) == EINVAL, (entry, name)       # the pointer is checked first
        assert c.untouched()


@pytest.mark.parametrize("name", PLANS)
def test_a_valid_decode_still_runs(calls, name):
    """After every refusal above (this module's tests share their plans and run in file order): a decode with exactly the size the
    library asks for returns VIT_OK through every entry point that serves the plan, and all of them decode the states of
    vit_decode_packed -- dense97, which has no packed decode, the oracle's through vit_decode."""
    c = calls[name]
    if name == "dense97":
        ref_s, ref_l = vo.decode_c(c.A, c.pi, c.E.cpu().numpy(), lengths=LENS)
        st, ll = c.dec.decode(c.E, lengths=c.lengths, out_dtype=torch.int32)
        assert np.array_equal(st.cpu().numpy(), ref_s) and np.array_equal(ll.cpu().numpy(), ref_l)
        return
    c.states.fill_(12345)
    assert c.run("packed", ws_bytes=int(c.need("packed"))) == OK
    torch.cuda.synchronize()
    want_s, want_l = c.states[:N].clone(), c.loglik.clone()
    assert bool((want_s >= 0).all()) and bool((want_s < c.S).all())
    for entry in PACKED[1:]:
        if name in SERVED[entry]:
            c.states.fill_(12345)
            c.loglik.fill_(7.0)
            assert c.run(entry, ws_bytes=int(c.need(entry))) == OK, entry
            torch.cuda.synchronize()
            assert torch.equal(c.states[:N], want_s) and torch.equal(c.loglik.view(torch.int32), want_l.view(torch.int32)), entry
    padded = ["checkpointed"] + (["logits"] if name in SERVED["logits"] else [])
    for entry in padded:
        c.states.fill_(12345)
        assert c.run(entry, ws_bytes=int(c.need(entry))) == OK, entry
        torch.cuda.synchronize()
        if entry == "checkpointed":
            st = c.states.view(B, T)
            for b in range(B):
                assert torch.equal(st[b, :int(LENS[b])], want_s[int(OFF[b]):int(OFF[b + 1])]), (entry, b)
