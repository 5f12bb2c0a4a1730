"""Every kernel geometry on inputs whose sums round (tests/inexact.py, tests/inexact_cases.py).

The geometry tests of tests/test_gpu_parity.py draw their matrices and emissions from dyadic grids with small magnitudes, where
every addition of the recursion is exact: a kernel that forms fl(d + fl(A + E)), or a back-trace that compares after the emission
add, returns the reference's bits there.  These tests decode the off-grid twins of the same matrices (one value -> one value, so
the plan classifies the twin like the original -- asserted through dec.info and vit_forward_family) and log-probability inputs for
the unstructured dense kernels.  tests/test_inexact_host.py asserts, on the reference alone, that on every case at least half of
the candidate sums round (measured per case: the docstring of tests/inexact_cases.py; by family: wave 0.53 - 0.94, path 0.63 - 0.81,
banded 0.53 - 0.81, sparse 0.54 - 0.77, dense 0.91 - 1.00 (S = 1: 0, by construction), wide 0.51, step 0.64 - 0.90), that the reassociated forward pass is
visible on it, and that the reassociated back-trace is visible in every structure.

Bar: states and log-likelihood bits equal oracle.viterbi_oracle.decode_c.  No tolerance."""
import numpy as np
import pytest
import torch

from tests import floor_grid as fg
from tests import inexact_cases as ic
from viterbi_spl_amd import ViterbiDecoder, _lib

pytestmark = pytest.mark.gpu

INFO_KEYS = ("banded_ok", "floor_ok", "pair_ok", "wave_ok", "step_ok", "group_window", "extras", "n_dense_rows", "lo_affine")
K = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x, np.float32)
    return x.view(np.uint32)


def algos(dec):
    if dec.info["banded_ok"]:
        return ("dense", "group", "wave") if dec.info["wave_ok"] else ("dense", "banded")
    return ("dense", "auto") if dec.info["step_ok"] else ("dense",)


def setup(dev, cid):
    """(case, decoder of the twin, emissions and lengths on the device, the oracle's states and log-likelihoods).  The twin's plan
    must be the original's: the same flags, window, extra columns and dense rows, the same forward family for every algo."""
    c = ic.case(cid)
    dec = ViterbiDecoder(c.A, c.pi, dev)
    if c.A0 is not None:
        orig = ViterbiDecoder(c.A0, c.pi0, dev)
        for k in INFO_KEYS:
            assert dec.info[k] == orig.info[k], (cid, k, dec.info[k], orig.info[k])
        for algo in ("auto",) + algos(dec) + (("banded",) if dec.info["banded_ok"] else ()):
            assert dec.forward_family(c.B, algo) == orig.forward_family(c.B, algo), (cid, algo)
    E = torch.from_numpy(np.array(c.E16 if c.f16 else c.E)).to(dev)           # (a copy: the case's arrays are read-only)
    assert E.dtype == (torch.float16 if c.f16 else torch.float32)
    ref_s, ref_l, _ = ic.oracle(cid)
    return c, dec, E, torch.from_numpy(c.lens).to(dev), ref_s, ref_l


def check(got, ref_s, ref_l, what):
    st, ll = got
    st = st.cpu().numpy()
    assert np.array_equal(st, ref_s), (what, "states", np.argwhere(st != ref_s)[:6].tolist())
    assert np.array_equal(_bits(ll), _bits(ref_l)), (what, "log-likelihood bits", ll.cpu().numpy(), ref_l)


# ------------------------------------------------------------------ a. wave geometries
@pytest.mark.parametrize("cid", ic.ids("wave"))
def test_wave_geometries(dev, cid):
    """The option walk of test_wave_form_geometries -- both register budgets, every back-trace form, the full and the half history,
    every specialised forward variant -- then forced chunkings, then the workgroup and dense kernels on the same songs."""
    c, dec, E, lens, ref_s, ref_l = setup(dev, cid)
    assert dec.info["wave_ok"] == (c.S + len(c.extras) < 384) and dec.info["extras"] == c.extras, (cid, dec.info)
    try:
        if dec.info["wave_ok"]:
            dec.set_option("wave_history", 2)
            half_ok = dec.history_mode(c.B, c.T, "wave") == "half"
            dec.set_option("reset", 0)
            for two in (0, 1, 2):
                for btf in (0, 1, 2):
                    for hist in ((1, 2) if half_ok else (1,)):
                        for uni in ((0, 1, 2, 3) if btf == 0 else (0,)):
                            for key, v in (("wave_two", two), ("backtrace_form", btf), ("wave_history", hist), ("wave_uniform", uni)):
                                dec.set_option(key, v)
                            check(dec.decode(E, lengths=lens, algo="wave", out_dtype=torch.int32), ref_s, ref_l, (cid, two, btf, hist, uni))
            dec.set_option("reset", 0)
            for chunks, warm in ((7, 0), (32, 1)):
                for hist in ((1, 2) if half_ok else (1,)):
                    for btf in (0, 2):
                        for key, v in (("bt_chunks", chunks), ("bt_warm", warm), ("bt_fast_rows", 1 if warm == 1 else 0),
                                       ("wave_history", hist), ("backtrace_form", btf)):
                            dec.set_option(key, v)
                        check(dec.decode(E, lengths=lens, algo="wave", out_dtype=torch.int32), ref_s, ref_l, (cid, "chunks", chunks, warm, hist, btf))
            dec.set_option("reset", 0)
        for algo in ("group", "dense"):
            assert dec.forward_family(c.B, algo) == algo
            for chunks, warm in ((0, -1), (7, 0), (32, 1)):
                dec.set_option("bt_chunks", chunks)
                dec.set_option("bt_warm", warm)
                check(dec.decode(E, lengths=lens, algo=algo, out_dtype=torch.int32), ref_s, ref_l, (cid, algo, chunks, warm))
            dec.set_option("reset", 0)
    finally:
        dec.set_option("reset", 0)


@pytest.mark.parametrize("cid", ("wave3", "wave4", "wave8"))
def test_wave_variants_on_the_same_songs(dev, cid):
    """No, one and two extra columns: decode_packed, decode_checkpointed and decode_packed_checkpointed (segments of 64 frames) on the
    songs of test_wave_geometries."""
    c, dec, E, lens, ref_s, ref_l = setup(dev, cid)
    assert dec.info["wave_ok"] and len(c.extras) == {"wave3": 0, "wave4": 1, "wave8": 2}[cid]
    check(dec.decode_checkpointed(E, segment_frames=K, lengths=lens, out_dtype=torch.int32), ref_s, ref_l, (cid, "decode_checkpointed"))
    order = fg.pack_order(c.lens)
    off = fg.offsets_of(c.lens[order])
    Ep = torch.cat([E[b, :int(c.lens[b])] for b in order], dim=0).contiguous()
    for entry, kw in (("decode_packed", {}), ("decode_packed_checkpointed", {"segment_frames": K})):
        st, ll = getattr(dec, entry)(Ep, off, out_dtype=torch.int32, **kw)
        st = st.cpu().numpy()
        for k, b in enumerate(order):
            assert np.array_equal(st[off[k]:off[k + 1]], ref_s[b, :c.lens[b]]), (cid, entry, "states of song", int(b))
        assert np.array_equal(_bits(ll), _bits(ref_l[order])), (cid, entry, "log-likelihood bits")


# ------------------------------------------------------------------ b. structure cases
@pytest.mark.parametrize("cid", ic.ids("path") + ic.ids("banded") + ic.ids("sparse"))
def test_structures(dev, cid):
    """Floor and scan forward forms, lean (affine / tabulated window starts) and generic back-traces, dense rows, extra columns in
    mid-matrix, floors of -50, -3 and -inf, the sparse bands of the wide windows: every algo of the plan, every back-trace form."""
    c, dec, E, lens, ref_s, ref_l = setup(dev, cid)
    info = dec.info
    assert info["banded_ok"], (cid, info)
    fwd, bt = fg.selected_kernels(info)
    if c.family == "path":
        assert c.name.startswith(fwd) and (bt.startswith(c.name.split("+")[1]) or c.name.split("+")[1] == "lean"), (c.name, info)
    if c.family == "banded":
        assert info["extras"] == c.extras and info["n_dense_rows"] == len(c.dense_rows), (cid, info)
    if c.family == "sparse":
        assert info["group_window"] == c.W and info["floor_ok"] and fwd == "floor" and bt.startswith("lean"), (cid, info)
    try:
        for btf in (0, 1, 2):
            dec.set_option("backtrace_form", btf)
            for algo in algos(dec):
                check(dec.decode(E, lengths=lens, algo=algo, out_dtype=torch.int32), ref_s, ref_l, (cid, btf, algo, info))
    finally:
        dec.set_option("reset", 0)


# ------------------------------------------------------------------ c. dense
@pytest.mark.parametrize("S", ic.DENSE_S)
def test_dense_size_classes(dev, S):
    """Log-probability matrices and emissions in every size class of the dense kernels: streaming (S <= 64, S > 368) and
    matrix-resident (64 / 128 / 184 sources per half row), both forms, fp32 and fp16 storage."""
    for f16 in (False, True):
        cid = f"dense{S}-{'f16' if f16 else 'f32'}"
        c, dec, E, lens, ref_s, ref_l = setup(dev, cid)
        assert not dec.info["banded_ok"] and not dec.info["step_ok"] and dec.forward_family(c.B, "auto") == "dense", (cid, dec.info)
        try:
            for form in (0, 1):
                dec.set_option("dense_form", form)
                check(dec.decode(E, lengths=lens, out_dtype=torch.int32), ref_s, ref_l, (cid, form))
                dec.set_option("reset", 0)
        finally:
            dec.set_option("reset", 0)


@pytest.mark.parametrize("B", ic.GROUPS_B)
def test_dense_groups_of_songs(dev, B):
    """The 1-, 4- and 8-songs-per-workgroup instantiations of the streaming dense kernel, ragged songs inside a group.  At 97 states
    the matrix-resident form takes the launch whatever "dense_songs" says (dense.hip launch_dense), so every setting runs with
    "dense_form" 1 as well: only then does the streaming kernel with that many songs per workgroup decode the batch."""
    c, dec, E, lens, ref_s, ref_l = setup(dev, f"dense97-B{B}")
    try:
        for ns in (0, 4, 8):
            for form in (0, 1):
                dec.set_option("dense_songs", ns)
                dec.set_option("dense_form", form)
                check(dec.decode(E, lengths=lens, algo="dense", out_dtype=torch.int32), ref_s, ref_l, (B, ns, form))
                dec.set_option("reset", 0)
    finally:
        dec.set_option("reset", 0)


# ------------------------------------------------------------------ d. wide windows in the generic back-trace
def test_generic_backtrace_with_wide_windows(dev):
    """Windows of 84 sources, the paths forced through window sources beyond the first 64, behind the workgroup and the dense forward
    pass, every back-trace form."""
    c, dec, E, lens, ref_s, ref_l = setup(dev, "wide200")
    assert dec.info["banded_ok"] and dec.info["group_window"] == 84 and dec.info["n_dense_rows"] == 0, dec.info
    step = ref_s[0][1:c.T] - ref_s[0][:c.T - 1]
    assert np.sum((step <= -24) & np.isin(ref_s[0][1:c.T], fg.WIDE_ROWS)) > 10, "the path must enter wide rows through window sources beyond the first 64"
    try:
        for algo in ("auto", "dense", "group"):
            for btf in (0, 1, 2):
                dec.set_option("backtrace_form", btf)
                check(dec.decode(E, lengths=lens, algo=algo, out_dtype=torch.int32), ref_s, ref_l, (algo, btf))
    finally:
        dec.set_option("reset", 0)


# ------------------------------------------------------------------ e. step kernels
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("geometry", ic.STEP_GEOMETRIES, ids=lambda g: "n%d-bw%d-kb%d" % g)
def test_step_geometries(dev, geometry, f16):
    """Generated step matrices with 1, 3, 9, 14 and 15 near bands: both step forms where the forward step kernel is instantiated
    (707 voiced states, 20-bin bands, nine near bands), the dense forward kernels with the band-table back-trace elsewhere, and the
    plain dense kernel."""
    n, bw, kb = geometry
    cid = f"step-n{n}-bw{bw}-kb{kb}-{'f16' if f16 else 'f32'}"
    c, dec, E, lens, ref_s, ref_l = setup(dev, cid)
    assert not dec.info["banded_ok"] and dec.info["step_ok"] == (geometry == (707, 20, 9)), (cid, dec.info)
    assert dec.forward_family(c.B, "auto") == "dense"
    try:
        for algo, form in (("auto", 0), ("auto", 3), ("dense", 0)):
            dec.set_option("step_form", form)
            check(dec.decode(E, lengths=lens, algo=algo, out_dtype=torch.int32), ref_s, ref_l, (cid, algo, form))
            dec.set_option("reset", 0)
    finally:
        dec.set_option("reset", 0)
