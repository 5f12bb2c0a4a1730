"""GPU tests of the bounded-workspace decode for plans without the wave form (the 722-state grids): banded plans with the floor
form (jdc722, jdc721, imm722w: the checkpoint / resume variant of the one-target floor kernel, sparse back-trace over the workgroup
rows) and step plans (durrieu722, durrieu721: the same variant of the step kernel, lazy back-trace per segment).  Everything through
ViterbiDecoder.  Bar: states and log-likelihood bit-equal to the CPU oracle run on every song alone.
GROUP_PLANS are (W, NWT) = (84, 12) and (128, 12); every other pair of the variant: tests/test_gpu_floor_variant_grid.py."""
import time

import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from viterbi_spl_amd import ViterbiDecoder, _lib, synth
from viterbi_spl_amd import decoder as decoder_module

pytestmark = pytest.mark.gpu

GROUP_PLANS = ["jdc722", "jdc721", "imm722w", "durrieu722", "durrieu721"]
GEN = {"peaks": synth.emissions_peaks, "dense": synth.emissions_dense, "ties": synth.emissions_ties, "scaled": synth.emissions_scaled}
SEGMENTS = (64, 100, 128, 640, 4096)
ORACLE_SECONDS = [0.0]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _module_time():
    t0 = time.time()
    yield
    print(f"\ntest_gpu_ckpt_group: {time.time() - t0:.0f} s in all, {ORACLE_SECONDS[0]:.0f} s of them in the CPU oracle")


def _oracle(A, pi, E, lengths=None):
    t0 = time.time()
    out = vo.decode_c(A, pi, E, lengths=lengths)
    ORACLE_SECONDS[0] += time.time() - t0
    return out


def _params(golden, name):
    return golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]


def _scan_only_jdc722(golden):
    """jdc722 with one in-window entry below its row's constant: still banded, but the floor form is not proven."""
    A = np.array(golden["params"]["jdc722_logA_T"], np.float32, copy=True)
    vals, counts = np.unique(A[300], return_counts=True)
    A[300, 303] = np.float32(vals[np.argmax(counts)]) - np.float32(5)
    return A, golden["params"]["jdc722_log_pi"]


def _small_case(kind, f16, T, S, dev):
    E = GEN[kind](9, T, S, seed=31, device=dev, dtype=torch.float16 if f16 else torch.float32)
    lens = torch.tensor([T, 1, 2, 63, 64, 65, T - 1, 300, 128], dtype=torch.int64, device=dev).clamp(max=T)
    return E, lens


@pytest.mark.parametrize("name", GROUP_PLANS)
def test_ckpt_group_small(golden, dev, name):
    """The matrix of test_checkpointed_decode_small on the 722-state plans: every segment length (T a multiple of it or not,
    shorter than one segment), ragged songs that end in any segment or before it, fp32 and fp16 storage, with and without
    `lengths`.  Frames past a song's end are -1 (the oracle's convention)."""
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    assert not dec.info["wave_ok"]
    for kind, f16, T in (("peaks", False, 1000), ("dense", True, 777), ("ties", False, 640), ("scaled", False, 129)):
        E, lens = _small_case(kind, f16, T, dec.S, dev)
        for use_len in (False, True):
            ln = lens if use_len else None
            ref_s, ref_l = _oracle(A, pi, E.float().cpu().numpy(), lengths=ln.cpu().numpy() if use_len else None)
            if use_len:
                lh = lens.cpu().numpy()
                assert all((ref_s[b, lh[b]:] == -1).all() for b in range(len(lh)))
            for K in SEGMENTS:
                st, ll = dec.decode_checkpointed(E, segment_frames=K, lengths=ln, out_dtype=torch.int32)
                assert np.array_equal(st.cpu().numpy(), ref_s), (name, kind, T, use_len, K)
                assert np.array_equal(ll.cpu().numpy(), ref_l), (name, kind, T, use_len, K)


@pytest.mark.parametrize("name", ["jdc722", "durrieu722"])
def test_ckpt_group_stays_inside_its_workspace(golden, dev, name):
    """The same decode in a caller-owned workspace that holds 0xFF bytes (NaN patterns) beforehand, handed over as an interior,
    256-byte aligned pointer with 1 MB of guard bytes on either side: the oracle's result, every guard byte unchanged (the
    banded kernel stores the frame maximum one row behind the row it computes -- for the first frame of a resumed segment that
    is the row in front of the segment, which must be the song's own), and a second call returns identical bytes."""
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    G = 1 << 20
    E, lens = _small_case("peaks", False, 1000, dec.S, dev)                  # song 0: 1000 frames, longer than every K below
    ref_s, ref_l = _oracle(A, pi, E.cpu().numpy(), lengths=lens.cpu().numpy())
    for K in (64, 100, 640):
        need = dec.workspace_bytes_checkpointed(9, 1000, K)
        buf = torch.full((G + 256 + need + 256 + G,), 0xFF, dtype=torch.uint8, device=dev)
        off = G + (-(buf.data_ptr() + G)) % 256                              # first 256-byte aligned address behind the front guard
        ws = buf[off:off + need + 256]
        assert ws.data_ptr() % 256 == 0
        outs = []
        for _ in range(2):
            st, ll = dec.decode_checkpointed(E, segment_frames=K, lengths=lens, out_dtype=torch.int32, workspace=ws)
            torch.cuda.synchronize()
            outs.append((st.cpu().numpy(), ll.cpu().numpy()))
        assert np.array_equal(outs[0][0], ref_s) and np.array_equal(outs[0][1], ref_l), (name, K)
        assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes(), (name, K)
        assert bool((buf[:off] == 0xFF).all()), (name, K, "bytes in front of the workspace were written")
        assert bool((buf[off + need:] == 0xFF).all()), (name, K, "bytes behind the workspace were written")


@pytest.mark.parametrize("name", ["jdc722", "durrieu722"])
def test_ckpt_group_full_size(golden, dev, name):
    """[256, 30000, 722] fp16 in a workspace below 1/16 of vit_workspace_bytes (segments of 1024 frames): bit-equal to the normal
    decode on every song and to the oracle on sampled ones (the one-frame song, the 1025-frame song, a full-length song)."""
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    B, T, S, K = 256, 30000, dec.S, 1024
    base = synth.emissions_peaks(32, T, S, seed=555, device=dev, dtype=torch.float16)
    base[24:] = synth.emissions_dense(8, T, S, seed=556, device=dev, dtype=torch.float16)
    E = base.repeat(8, 1, 1).contiguous()
    del base
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    lens[3], lens[40], lens[41], lens[200] = 1, 1024, 1025, 29999
    need = dec.workspace_bytes_checkpointed(B, T, K)
    full = dec.workspace_bytes(B, T)
    assert need * 16 <= full
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    want_s, want_l = dec.decode(E, lengths=lens, out_dtype=torch.int32)
    dec._ws = None                                                       # (the normal decode's 22 GB)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st, ll = dec.decode_checkpointed(E, segment_frames=K, lengths=lens, out_dtype=torch.int32, workspace=ws)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{name}: checkpointed decode [256, 30000, 722], segments of {K}: workspace {need / 1e6:.0f} MB (full history {full / 1e6:.0f} MB), "
          f"{int(lens.sum()) / dt / 1e6:.0f} Mframes/s")
    assert torch.equal(st, want_s) and torch.equal(ll, want_l)
    picks = [3, 41, 31]
    ref_s, ref_l = _oracle(A, pi, E[picks].float().cpu().numpy(), lengths=lens[picks].cpu().numpy())
    assert np.array_equal(st[picks].cpu().numpy(), ref_s) and np.array_equal(ll[picks].cpu().numpy(), ref_l)


@pytest.mark.parametrize("name", ["jdc722", "durrieu722"])
def test_ckpt_group_budget_policy(golden, dev, name):
    """ViterbiDecoder.decode(max_workspace_bytes=...) and the module-level decode(): "full" while the budget holds the history,
    then straight to "checkpointed" (there is no half history for the workgroup layout), the same bits in every mode; a budget
    nothing fits raises and names the need."""
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    B, T = 8, 3000
    E = synth.emissions_peaks(B, T, dec.S, seed=77, device=dev, dtype=torch.float16)
    lens = torch.tensor([T, 1, 2999, 1025, 64, T, 2048, 777], dtype=torch.int64, device=dev)
    ref_s, ref_l = _oracle(A, pi, E.float().cpu().numpy(), lengths=lens.cpu().numpy())
    full = dec.workspace_bytes(B, T, "auto")
    seen = []
    for budget in (2 * full, full, full - 1, full // 2, full // 4, full // 8, full // 20):
        mode = dec.plan_workspace(B, T, "auto", budget)
        assert mode["workspace_bytes"] <= budget
        seen.append(mode["mode"])
        dec._ws = None
        st, ll = dec.decode(E, lengths=lens, out_dtype=torch.int32, max_workspace_bytes=budget)
        assert np.array_equal(st.cpu().numpy(), ref_s) and np.array_equal(ll.cpu().numpy(), ref_l), (name, budget, mode)
        st, ll = decoder_module.decode(E, A, pi, lengths=lens, out_dtype=torch.int32, max_workspace_bytes=budget)
        assert np.array_equal(st.cpu().numpy(), ref_s) and np.array_equal(ll.cpu().numpy(), ref_l), (name, budget, mode, "module-level decode")
    assert seen == ["full", "full"] + ["checkpointed"] * 5, seen
    with pytest.raises(_lib.ViterbiHipError, match=str(full)):
        dec.decode(E, max_workspace_bytes=100000)
    with pytest.raises(_lib.ViterbiHipError, match=str(full)):
        decoder_module.decode(E, A, pi, max_workspace_bytes=100000)
    with pytest.raises(_lib.ViterbiHipError):
        dec.decode(E, algo="dense", max_workspace_bytes=full // 4)           # the dense kernel has no bounded form


def test_ckpt_group_refusals_are_loud_and_early(golden, dev):
    """Plans the checkpointed decode does not serve raise from decode_checkpointed, and at the C ABI the refusal comes before
    anything is enqueued: a `states` buffer filled with a sentinel is untouched (with `lengths` given an accepted call starts by
    filling it with -1)."""
    lib = _lib.load()
    p = golden["params"]
    for A, pi in ((p["dense97_logA_T"], p["dense97_log_pi"]), _scan_only_jdc722(golden)):
        dec = ViterbiDecoder(A, pi, dev)
        B, T = 3, 200
        E = synth.emissions_dense(B, T, dec.S, seed=1, device=dev)
        with pytest.raises(_lib.ViterbiHipError):
            dec.decode_checkpointed(E, segment_frames=64)
        st = torch.full((B, T), 12345, dtype=torch.int32, device=dev)
        ll = torch.full((B,), 7.0, dtype=torch.float32, device=dev)
        lens = torch.tensor([T, 5, 100], dtype=torch.int64, device=dev)
        ws = torch.empty(dec.workspace_bytes(B, T) + 256, dtype=torch.uint8, device=dev)
        rc = lib.vit_decode_checkpointed(dec._plan, E.data_ptr(), _lib.VIT_F32, B, T, lens.data_ptr(), (ws.data_ptr() + 255) & ~255,
                                         ws.numel() - 256, st.data_ptr(), ll.data_ptr(), 64, None)
        torch.cuda.synchronize()
        assert rc == -5                                                      # VIT_EUNSUPPORTED
        assert bool((st == 12345).all()) and bool((ll == 7.0).all())
        st2, _ = dec.decode(E, lengths=lens, out_dtype=torch.int32)          # the normal decode still serves the plan
        ref_s, _ = _oracle(np.asarray(A, np.float32), np.asarray(pi, np.float32), E.cpu().numpy(), lengths=lens.cpu().numpy())
        assert np.array_equal(st2.cpu().numpy(), ref_s)


@pytest.mark.parametrize("name", ["jdc722", "durrieu722"])
def test_ckpt_group_ignores_kernel_selection_options(golden, dev, name):
    """forward_form, backtrace_form (ignored) and bt_fast_rows (honoured) set on the plan: the same bits."""
    A, pi = _params(golden, name)
    dec = ViterbiDecoder(A, pi, dev)
    E, lens = _small_case("dense", True, 777, dec.S, dev)
    ref_s, ref_l = _oracle(A, pi, E.float().cpu().numpy(), lengths=lens.cpu().numpy())
    try:
        for key, values in (("forward_form", (1, 2, 3)), ("backtrace_form", (1, 2, 4)), ("bt_fast_rows", (1,))):
            for v in values:
                dec.set_option(key, v)
                for K in (100, 640):
                    st, ll = dec.decode_checkpointed(E, segment_frames=K, lengths=lens, out_dtype=torch.int32)
                    assert np.array_equal(st.cpu().numpy(), ref_s) and np.array_equal(ll.cpu().numpy(), ref_l), (name, key, v, K)
                dec.set_option("reset", 0)
    finally:
        dec.set_option("reset", 0)
