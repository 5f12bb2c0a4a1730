"""bench.py --dump-outputs (CPU): the last step's paths and log-likelihoods as float32 .npy files within the size budget, and
--steps / --warmup checked before anything runs."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _batch(B, T, S=361):
    g = torch.Generator().manual_seed(3)
    return torch.randint(0, S, (B, T), generator=g, dtype=torch.int32), torch.randn(B, generator=g) * 1e4


def test_dump_writes_the_whole_batch_when_it_fits(tmp_path):
    st, ll = _batch(6, 50)
    bench.dump_outputs(str(tmp_path / "out"), st, ll)
    assert sorted(os.listdir(tmp_path / "out")) == ["loglik.npy", "states.npy"]
    s, l = np.load(tmp_path / "out" / "states.npy"), np.load(tmp_path / "out" / "loglik.npy")
    assert s.dtype == np.float32 and l.dtype == np.float32
    assert np.array_equal(s, st.numpy().astype(np.float32)) and np.array_equal(l, ll.numpy())


def test_dump_samples_whole_songs_over_the_budget(tmp_path, monkeypatch):
    B, T = 40, 1000
    monkeypatch.setattr(bench, "DUMP_BYTES", 10 * (4 * T + 8) + 4096 + 4 * B)      # room for 10 of the 40 paths
    st, ll = _batch(B, T)
    outs = []
    for run in ("a", "b"):
        d = tmp_path / run
        bench.dump_outputs(str(d), st, ll)
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= bench.DUMP_BYTES + 3 * 128     # (.npy headers)
        outs.append((np.load(d / "song_index.npy"), np.load(d / "states.npy"), np.load(d / "loglik.npy")))
    idx, s, l = outs[0]
    assert idx.shape == (10,) and np.all(np.diff(idx) > 0)
    assert np.array_equal(s, st.numpy()[idx.astype(np.int64)].astype(np.float32))
    assert np.array_equal(l, ll.numpy())
    assert all(np.array_equal(x, y) for x, y in zip(outs[0], outs[1]))           # a fixed sample: the same rows every run


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_rejects_steps_it_cannot_time(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit) as e:
        bench.parse()
    assert e.value.code == 2
