"""Construction A of tests/far_offsets.py on the GPU: [B, T, S] batches whose songs 1 and 2 START past element 2^31 and byte 2^32 of
the emission (or logit) tensor and of the history, with live lengths of a few hundred frames and NaN everywhere else.  Every
uniform-batch entry point against the oracle on the live frames, bit for bit; states behind a length are -1 over all of T."""
import numpy as np
import pytest
import torch

from tests import f64_ref, far_offsets as fo
from tests.common import f32_bits
from viterbi_spl_amd import ViterbiDecoder, _lib, emissions as em, synth

pytestmark = pytest.mark.gpu

CASES = [("tonet361", False, "peaks"), ("tonet361", True, "ties"), ("msnet321", False, "dense"), ("msnet321", True, "peaks"),
         ("jdc722", False, "ties"), ("jdc722", True, "peaks"), ("durrieu722", False, "dense"), ("durrieu722", True, "dense"),
         ("dense361", False, "ties"), ("dense361", True, "peaks")]
IDS = [f"{n}-{'f16' if h else 'f32'}" for n, h, _ in CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _setup(golden, dev, name, f16, kind, layouts, budget=60 << 30):
    """-> (decoder, A, pi, B, T, lens, live (host), E (device, NaN outside the live frames), the history rows used).  `layouts`: the
    names of fo.history_rows whose marks the batch must pass (those the plan has)."""
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    rows = fo.history_rows(_lib.load(), dec._plan)
    used = {k: rows[k] for k in layouts if k in rows}
    assert used, (name, layouts, rows)
    widest = max(used.values(), key=lambda ri: ri[0] * ri[1])
    S, isz = dec.S, 2 if f16 else 4
    B, T = fo.shape_a(S, isz, widest, budget=budget)
    for r, i in used.values():                                     # song 1 starts past both marks of every buffer
        assert T * S >= max(fo.mark_elements(isz)) and T * r >= max(fo.mark_elements(i))
    fo.need_free(B * T * (S * isz + widest[0] * widest[1]))
    lens = fo.LIVE_A[B]
    live = fo.live_songs(kind, lens, S, seed=len(name) + 2 * f16, f16=f16)
    E = fo.nan_batch((B, T, S), torch.float16 if f16 else torch.float32, dev)
    for b, n in enumerate(lens):
        E[b, :n] = torch.from_numpy(live[b, :n]).to(dev)
    return dec, A, pi, B, T, lens, live, E, used


def _check(st, ll, ref_s, ref_l, what, bits=f32_bits):
    L = ref_s.shape[1]
    assert np.array_equal(st[:, :L].cpu().numpy(), ref_s), what
    assert bool((st[:, L:] == -1).all()), (what, "states behind the lengths")
    assert np.array_equal(bits(ll.cpu().numpy()), bits(ref_l)), (what, ll, ref_l)


def _algos(dec):
    if dec.info["banded_ok"]:
        return ("dense", "group", "wave") if dec.info["wave_ok"] else ("dense", "banded")
    return ("dense", "auto") if dec.info["step_ok"] else ("dense",)


@pytest.mark.parametrize("name,f16,kind", CASES, ids=IDS)
def test_decode_every_family_and_history(golden, dev, name, f16, kind):
    """decode() with every forward family the plan serves, the sparse and the whole-row back-trace, and -- wave form -- the full and
    the half history (song 2 of the half history starts past element 2^31, song 1 past byte 2^32)."""
    dec, A, pi, B, T, lens, live, E, used = _setup(golden, dev, name, f16, kind, ("dense", "group", "wave", "auto"))
    ref_s, ref_l = fo.expected_a(A, pi, live, lens)
    ln = torch.tensor(lens, dtype=torch.int64, device=dev)
    with fo.measured(f"a/decode/{name}/{'f16' if f16 else 'f32'}", (B, T, dec.S)):
        for algo in _algos(dec):
            for btf in ((0, 2) if dec.info["banded_ok"] and algo != "dense" else (0,)):
                for hist in ((1, 2) if algo == "wave" else (0,)):
                    dec.set_option("backtrace_form", btf)
                    dec.set_option("wave_history", hist)
                    if hist:
                        assert dec.history_mode(B, T, "wave") == ("full", "half")[hist - 1]
                    st, ll = dec.decode(E, lengths=ln, algo=algo, out_dtype=torch.int32)
                    dec.set_option("reset", 0)
                    _check(st, ll, ref_s, ref_l, (name, algo, btf, hist))
    del dec, E, st, ll
    fo.release()


@pytest.mark.parametrize("name,f16,kind", [c for c in CASES if c[0] != "dense361"], ids=[i for i in IDS if not i.startswith("dense361")])
def test_decode_checkpointed(golden, dev, name, f16, kind):
    """decode_checkpointed: far emission rows (its history is a few thousand rows per song: below the marks at any size that fits)."""
    dec, A, pi, B, T, lens, live, E, used = _setup(golden, dev, name, f16, kind, ("dense",))
    ref_s, ref_l = fo.expected_a(A, pi, live, lens)
    ln = torch.tensor(lens, dtype=torch.int64, device=dev)
    with fo.measured(f"a/decode_checkpointed/{name}/{'f16' if f16 else 'f32'}", (B, T, dec.S)):
        for K in (64, 100, 1024):
            st, ll = dec.decode_checkpointed(E, segment_frames=K, lengths=ln, out_dtype=torch.int32)
            _check(st, ll, ref_s, ref_l, (name, K))
    del dec, E, st, ll
    fo.release()


@pytest.mark.parametrize("name,f16,kind", [c for c in CASES if c[0] in ("tonet361", "msnet321", "jdc722")],
                         ids=[i for i in IDS if i.split("-")[0] in ("tonet361", "msnet321", "jdc722")])
def test_decode_f64(golden, dev, name, f16, kind):
    """decode_f64 and decode_f64_checkpointed on two songs (rows of doubles: three do not fit): the far song, of 257 frames, starts
    past both marks of the emissions and of the float64 history, which the forward pass writes and the back-trace reads back there."""
    dec, A, pi, B, T, lens, live, E, used = _setup(golden, dev, name, f16, kind, ("f64",))
    ref_s, ref_l = f64_ref.decode_f64_batch(A, pi, np.asarray(live, np.float32), lens)
    ref_s = ref_s.astype(np.int32)
    ln = torch.tensor(lens, dtype=torch.int64, device=dev)
    with fo.measured(f"a/decode_f64/{name}/{'f16' if f16 else 'f32'}", (B, T, dec.S)):
        st, ll = dec.decode_f64(E, lengths=ln, out_dtype=torch.int32)
        _check(st, ll, ref_s, ref_l, (name, "f64"), f64_ref.bits64)
        del dec, st, ll                                            # (with it the whole history it kept for the next decode)
        fo.release()
        dec = ViterbiDecoder(A, pi, dev)
        for K in (64, 1024):
            st, ll = dec.decode_f64_checkpointed(E, segment_frames=K, lengths=ln, out_dtype=torch.int32)
            _check(st, ll, ref_s, ref_l, (name, "f64 checkpointed", K), f64_ref.bits64)
    del dec, E, st, ll
    fo.release()


LOGITS = [("tonet361", "shaun", 5, False), ("tonet361", "softmax", 15, False), ("msnet321", "softmax_scaled", 5, False),
          ("tonet361", "shaun", 5, True)]


@pytest.mark.parametrize("name,mode,spw,with_out", LOGITS, ids=[f"{n}-{m}{'-emissions_out' if o else ''}" for n, m, _, o in LOGITS])
def test_decode_logits(golden, dev, name, mode, spw, with_out):
    """decode_logits and decode_logits_checkpointed on [B, T, cols] logits whose songs 1, 2 start past the marks (NaN outside the live
    frames); with_out: an emissions_out tensor of the same reach.  Expected: the oracle on the emissions the builder kernel makes of
    the live frames alone (a small tensor at low offsets)."""
    import math
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    S = dec.S
    n_bins = S - 1
    cols = n_bins + (1 if mode == "softmax" else 0)
    rows = fo.history_rows(_lib.load(), dec._plan)
    B, T = fo.shape_a(cols, 4, rows["wave"], budget=(40 << 30) if with_out else (60 << 30))
    assert T * cols >= 1 << 31 and T * rows["wave"][0] >= 1 << 31
    fo.need_free(B * T * 4 * (cols + rows["wave"][0] + (S if with_out else 0)))
    lens = fo.LIVE_A[B]
    L = max(lens)
    live = synth.pitch_logits(B, L, cols, seed=11, device=dev)
    if mode == "shaun":
        obs = ViterbiDecoder.obs_params("shaun", n_bins, spw, math.log(0.32 / 0.68), math.log(0.8 / 0.2), 2.0)
        built = em.shaun_log_emissions(live, 0.32, spw)
    elif mode == "softmax":
        obs = ViterbiDecoder.obs_params("softmax", n_bins, spw)
        built = em.softmax_log_emissions(live, spw)
    else:
        vth = np.float32(0.4)
        obs = ViterbiDecoder.obs_params("softmax_scaled", n_bins, spw, threshold_logit=float(np.log(vth / (np.float32(1) - vth))))
        built = em.softmax_scaled_log_emissions(live, 0.4, None, spw)
    ref_s, ref_l = fo.expected_a(A, pi, built.cpu().numpy(), lens)
    X = fo.nan_batch((B, T, cols), torch.float32, dev)
    for b, n in enumerate(lens):
        X[b, :n] = live[b, :n]
    ln = torch.tensor(lens, dtype=torch.int64, device=dev)
    eo = torch.full((B, T, S), -77.0, dtype=torch.float32, device=dev) if with_out else None
    with fo.measured(f"a/decode_logits/{name}/{mode}{'/emissions_out' if with_out else ''}", (B, T, cols)):
        st, ll = dec.decode_logits(X, obs, lengths=ln, out_dtype=torch.int32, emissions_out=eo)
        _check(st, ll, ref_s, ref_l, (name, mode))
        if with_out:
            for b, n in enumerate(lens):
                assert torch.equal(eo[b, :n].view(torch.int32), built[b, :n].view(torch.int32)), (b, "emissions_out")
        else:
            for K in (64, 1024):
                st, ll = dec.decode_logits_checkpointed(X, obs, segment_frames=K, lengths=ln, out_dtype=torch.int32)
                _check(st, ll, ref_s, ref_l, (name, mode, K))
    del dec, X, eo, st, ll
    fo.release()


@pytest.mark.parametrize("name,f16,kind", [c for c in CASES if c[0] != "dense361"], ids=[i for i in IDS if not i.startswith("dense361")])
def test_linear_stream_session(golden, dev, name, f16, kind):
    """stream(B, max_frames=T): recordings 1, 2 keep their history rows past the marks of the session's workspace.  Appended in ragged
    chunks, then decode() -- the oracle's states and log-likelihoods -- and, where the plan has a commit point, commit(): the
    committed prefix is the oracle's."""
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    rows = fo.history_rows(_lib.load(), dec._plan)
    S, isz = dec.S, 2 if f16 else 4
    r, i = rows["stream"]
    B = 3
    T = fo.rows_past([(r, i)])
    assert T * r >= 1 << 31
    fo.need_free(B * T * r * i)
    lens = fo.LIVE_A[B]
    L = max(lens)
    live = fo.live_songs(kind, lens, S, seed=5 + f16, f16=f16)
    ref_s, ref_l = fo.expected_a(A, pi, live, lens)
    E = torch.from_numpy(live).to(dev)
    with fo.measured(f"a/stream/{name}/{'f16' if f16 else 'f32'}", (B, T, S)):
        sess = dec.stream(B, max_frames=T)
        t = 0
        for n in (1, 63, 100, L - 164):
            sess.append(E[:, t:t + n].contiguous(), counts=[max(0, min(n, m - t)) for m in lens])
            t += n
        assert sess.lengths.tolist() == list(lens)
        st, ll = sess.decode(out_dtype=torch.int32)
        assert np.array_equal(st.cpu().numpy(), ref_s) and np.array_equal(f32_bits(ll.cpu().numpy()), f32_bits(ref_l)), name
        if dec._need("stream_commit", False, B) > 0:
            done, fresh = sess.commit(out_dtype=torch.int32)
            for b in range(B):
                assert 0 <= done[b] <= lens[b] and np.array_equal(fresh[b].cpu().numpy(), ref_s[b, :done[b]]), (name, b, done)
            assert kind != "peaks" or min(done[1:]) > 0, (name, done)      # (peak emissions coalesce within a few frames: DESIGN.md 2)
        sess.close()
    del dec, sess, st, ll
    fo.release()
