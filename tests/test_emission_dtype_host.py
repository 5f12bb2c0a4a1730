"""Host tests of the ``emission_dtype`` argument of the three logits post-processors: the validation runs before anything touches a
device, and the default keeps today's float32 rows.  (What float16 rows decode to: tests/test_gpu_half_pipeline.py.)"""
import inspect

import numpy as np
import pytest

from viterbi_spl_amd import emissions as em
from viterbi_spl_amd import reference_api as ra


@pytest.mark.parametrize("cls", [ra.Viterbi, ra.SoftMaxViterbi, ra.ScaledSoftMaxViterbi])
def test_emission_dtype_default_and_validation(cls):
    par = inspect.signature(cls.__init__).parameters
    assert par["emission_dtype"].default == "float32"
    A, pi = np.full((4, 4), 0.25), np.full(4, 0.25)
    args = (A, pi, 0.4, False) if cls is ra.ScaledSoftMaxViterbi else (A, pi)
    for bad in ("bfloat16", "float64", None, np.float16):
        with pytest.raises(ValueError, match="emission_dtype"):
            cls(*args, emission_dtype=bad)


def test_builders_take_an_emission_dtype():
    import torch
    for fn in (em.shaun_log_emissions, em.softmax_log_emissions, em.softmax_scaled_log_emissions):
        assert inspect.signature(fn).parameters["dtype"].default is torch.float32
