"""The C oracle's orc_mix on irregular CSR == fa_mix restated per operation in plain torch (every
product and every sum rounded to the dtype, the first term passed through): special values, zero and
negative weights, unsorted and repeated columns, post-scale.  tests/test_gpu_mix.py compares the HIP
mixing kernels with this oracle, so this is what makes it a reference there."""
from __future__ import annotations

import pytest
import torch

from refcases import bits_equal, mix_inputs, mix_matrices, mix_post_scale, torch_mix_reference

MATRICES = ["star9", "torus9", "undirected_tree10", "complete11_dense", "random12", "handmade"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize("name", MATRICES)
def test_oracle_mix_equals_per_operation_torch(name, dtype):
    from oracle import orc
    rp, cs, vs, num_in = mix_matrices()[name]
    post = mix_post_scale(len(rp) - 1)
    xs = mix_inputs(dtype, num_in, 2049, 17, special=True)
    exp, exp2 = torch_mix_reference(xs, rp, cs, vs, post)
    got, got2 = orc.mix(xs, rp, cs, vs, post_scale=post)
    for r, (a, b) in enumerate(zip(got + got2, exp + exp2)):
        assert bits_equal(a, b), (name, dtype, r)
    nan_rows = sum(bool(torch.isnan(e[:8]).any()) for e in exp)
    assert nan_rows > 0  # the special values reached the rows
