"""The split floor kernel's full-window waves store their delta copies with ds_write_addtid_b32 (M0 + immediate + 4 * lane, no
address register).  Two things can go wrong that no other test aims at: the address (M0 carries the wave and win_shift, the
immediate the buffer and the copy), and the wait in front of the barrier, which the compiler does not derive for an inline-asm
store -- a missing one is a race, not a fault.  So forward_form 6 is held against forward_form 1 and the CPU oracle bit for bit --
states, log-likelihoods and the raw history rows with their pad columns -- on every instantiation the launcher can pick, every
win_shift, and the lengths that hit every boundary of the round split (interior rounds, the clamped round, every tail parity,
both LDS buffers); and one long decode is repeated twenty times in one process and must give the same bytes every time."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests.test_floor_trim_host import _widths
from tests.test_gpu_floor_split import _bits, _history, _matrix
from viterbi_spl_amd import ViterbiDecoder, _lib, synth

pytestmark = pytest.mark.gpu

B, T_LONG = 3, 3001
LENGTHS = [1, 2, 12, 13, 14, 24, 25, 26, 37, 61, T_LONG]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


def _tonet(S, dmax):
    return synth.log_params(synth.tonet_transition(S - 1, dmax), synth.floored_prior(S))


def _plan(name):
    """(logA_T, log_pi, options, the width the full waves run at, extra column in M's slot quad (XQ), extra columns)"""
    if name == "tonet361":                      # <1, 12, float, false, true, 29>: what the bench runs
        return _tonet(361, 14) + ({}, 29, True, 1)
    if name == "tonet321":                      # <1, 12, float, false, true, 25>
        return _tonet(321, 12) + ({}, 25, True, 1)
    if name == "whole_window":                  # <1, 12, float, false, true, 32>
        return _tonet(361, 14) + ({"floor_live_window": 1}, 32, True, 1)
    if name == "select":                        # one extra column x = S - 1 with x % 4 != 0: the select (XQ false) instantiation
        A, pi, _ = _matrix(323, np.random.default_rng(323))
        return A, pi, {}, None, False, 1
    A, pi, _ = _matrix(330, np.random.default_rng(330), n_extras=2)   # generic extras: <-1, 12, float>, whole window
    return A, pi, {}, 32, False, 2


@pytest.fixture(scope="module")
def case(dev, request):
    """One plan: the decoder, the emissions [3, 3001, S] (three distinct songs) and, per length, the oracle's answer and what
    forward_form 1 leaves (computed once, shared by the win_shift cases)."""
    A, pi, opts, wf, xq, nx = _plan(request.param)
    S = A.shape[0]
    dec = ViterbiDecoder(A, pi, dev)
    info = dec.info
    assert info["floor_ok"] and info["group_window"] == 32 and info["n_dense_rows"] == 0 and 256 < S < 384, info
    assert info["n_extras"] == nx and ((nx == 1 and info["extras"] == [S - 1] and (S - 1) % 4 == 0) == xq), info
    if wf is not None and not opts:
        assert _widths(A, pi)[1] == wf, (request.param, _widths(A, pi))
    E = synth.emissions_peaks(B, T_LONG, S, seed=41, device=dev)
    assert not torch.equal(E[0], E[1]) and not torch.equal(E[1], E[2])
    En = E.cpu().numpy()
    ref = {}
    for L in LENGTHS:
        EL = E[:, :L].contiguous()
        for k, v in opts.items():
            dec.set_option(k, v)
        dec.set_option("forward_form", 1)
        st, ll = dec.decode(EL, algo="group", out_dtype=torch.int32)
        h1 = _history(dec, EL, None, 1)          # (resets the options)
        os_, ol = vo.decode_c(A, pi, En[:, :L])
        assert np.array_equal(st.cpu().numpy(), os_) and np.array_equal(_bits(ll.cpu().numpy()), _bits(ol)), (request.param, L, "form 1")
        ref[L] = (EL, os_, ol, h1)
    return request.param, dec, opts, ref


def _form6(dec, opts, sh, EL):
    for k, v in opts.items():
        dec.set_option(k, v)
    dec.set_option("win_shift", sh)
    dec.set_option("forward_form", 6)
    st, ll = dec.decode(EL, algo="group", out_dtype=torch.int32)
    for k, v in opts.items():                    # (_history sets the form itself; the other options must still stand)
        dec.set_option(k, v)
    dec.set_option("win_shift", sh)
    h = _history(dec, EL, None, 6)               # (resets the options)
    return st.cpu().numpy(), ll.cpu().numpy(), h


@pytest.mark.parametrize("sh", [0, 1, 2, 3])
@pytest.mark.parametrize("case", ["tonet361", "tonet321", "whole_window", "select", "generic_extras"], indirect=True)
def test_split_kernel_against_one_target_kernel_and_oracle(case, sh):
    name, dec, opts, ref = case
    for L in LENGTHS:
        EL, os_, ol, h1 = ref[L]
        st, ll, h6 = _form6(dec, opts, sh, EL)
        assert np.array_equal(st, os_), (name, sh, L, "states")
        assert np.array_equal(_bits(ll), _bits(ol)), (name, sh, L, "log-likelihood")
        assert np.array_equal(h6, h1), (name, sh, L, "history rows", np.argwhere(h6 != h1)[:8])


@pytest.mark.parametrize("case", ["tonet361"], indirect=True)
def test_twenty_decodes_give_the_same_bytes(case):
    """A store that has not landed when the barrier releases would show as a difference between runs, not as a fault."""
    name, dec, opts, ref = case
    EL, os_, ol, h1 = ref[T_LONG]
    first = _form6(dec, opts, -1, EL)            # (-1: the plan's own shift)
    assert np.array_equal(first[0], os_) and np.array_equal(_bits(first[1]), _bits(ol)) and np.array_equal(first[2], h1)
    for rep in range(1, 20):
        st, ll, h6 = _form6(dec, opts, -1, EL)
        assert np.array_equal(st, first[0]) and np.array_equal(_bits(ll), _bits(first[1])), (rep, "differs from the first decode")
        assert np.array_equal(h6, first[2]), (rep, "history rows", np.argwhere(h6 != first[2])[:8])
