"""GPU test of the wave form's launch table (wave.hip): every history mode an entry point reaches, with every register form
("wave_two" 0 / 1 / 2) and every uniform-lane form ("wave_uniform" 0 - 3) the options can ask for, on the shipped 361- and
321-state matrices with float32 and float16 emissions.  Bar: the oracle's states, its log-likelihood bits.

Seven songs of 1, 2, 63, 64, 65, 129 and 150 frames: two workgroups of four waves (the second one partial); the tails of the
unrolled frame loop for every prefetch depth; with segments of 64 frames a song that ends just before, at and just behind a segment
boundary, and three segments with a short last one.  The padded entries see T = 150 with lengths, the packed ones the same songs
back to back."""
import numpy as np
import pytest
import torch

from oracle import viterbi_oracle as vo
from tests.common import GEN
from viterbi_spl_amd import ViterbiDecoder, _lib

pytestmark = pytest.mark.gpu

LENS = np.array([1, 2, 63, 64, 65, 129, 150], np.int64)
T, K = 150, 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return torch.device("cuda:0")


@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("name", ["tonet361", "msnet321"])
def test_every_cell_of_the_launch_table(golden, dev, name, dt):
    A, pi = golden["params"][f"{name}_logA_T"], golden["params"][f"{name}_log_pi"]
    dec = ViterbiDecoder(A, pi, dev)
    assert dec.info["wave_ok"]
    B, S = len(LENS), dec.S
    E = GEN["peaks"](B, T, S, seed=41, device=dev, dtype=dt)
    E[4:] = GEN["dense"](B - 4, T, S, seed=42, device=dev, dtype=dt)
    lens = torch.from_numpy(LENS).to(dev)
    ref_s, ref_l = vo.decode_c(A, pi, E.float().cpu().numpy(), lengths=LENS)
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum(LENS)
    Ep = torch.cat([E[b, :int(n)] for b, n in enumerate(LENS)], dim=0).contiguous()
    ref_p = np.concatenate([ref_s[b, :int(n)] for b, n in enumerate(LENS)])
    dec.set_option("wave_history", 2)
    half_ok = dec.history_mode(B, T, "wave") == "half"
    dec.set_option("reset", 0)
    entries = {
        "full": lambda: dec.decode(E, lengths=lens, algo="wave", out_dtype=torch.int32),
        "half": lambda: dec.decode(E, lengths=lens, algo="wave", out_dtype=torch.int32),
        "checkpointed": lambda: dec.decode_checkpointed(E, segment_frames=K, lengths=lens, out_dtype=torch.int32),
        "packed": lambda: dec.decode_packed(Ep, off, out_dtype=torch.int32),
        "packed_checkpointed": lambda: dec.decode_packed_checkpointed(Ep, off, segment_frames=K, out_dtype=torch.int32),
    }
    ran = 0
    for two in (0, 1, 2):
        for uni in (0, 1, 2, 3):
            for entry, run in entries.items():
                if entry == "half" and not half_ok:
                    continue
                dec.set_option("wave_two", two)
                dec.set_option("wave_uniform", uni)
                if entry == "half":
                    dec.set_option("wave_history", 2)
                    assert dec.history_mode(B, T, "wave") == "half"
                try:
                    st, ll = run()
                    what = (name, dt, entry, two, uni)
                    want = ref_p if entry.startswith("packed") else ref_s
                    assert np.array_equal(st.cpu().numpy(), want), what
                    assert np.array_equal(ll.cpu().numpy().view(np.int32), ref_l.view(np.int32)), what
                    assert dec.info["wave_ok"], what
                finally:
                    dec.set_option("reset", 0)
                ran += 1
    assert ran == 12 * (5 if half_ok else 4)
