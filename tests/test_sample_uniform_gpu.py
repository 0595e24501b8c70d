"""GPU: the uniform number behind g2v_sample_rows_bf16's Gumbel noise at the top of its range.

u = (r24 + 0.5) / 2^24 with r24 the top 24 bits of the Philox word.  fp32 holds r24 + 0.5 exactly only below 2^23; before the
kernel formed -log u from 1 - u there, r24 = 2^24 - 1 gave u = 1.0 and a score of +inf whatever the logit - one uniformly random
token per 2^24 elements, 0.9 % of the draws at the 151 936-entry vocabulary - and every draw in the upper half, where the winners
are, carried up to half a step of error in 1 - u.  tests/test_scratch_contracts_gpu.py met the second effect on 64 x 151 936 random
logits (row 53 missed the owning test's bound); the cases here are the first effect, planted: the (seed, row, step, index) whose
r24 is 0xFFFFFF, found with tests/imageop_check.py's Philox restatement."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import imageop_check as I  # noqa: E402

SEED, N = 0x1234567890ABCDEF, 151936
ALL_ONES = [(85, 85091), (188, 77766)]                       # (step, index) of row 0 with r24 == 2^24 - 1 under SEED


@pytest.mark.parametrize("step,index", ALL_ONES)
def test_the_largest_uniform_number_does_not_outvote_the_logits(step, index):
    from g2vlm_amd import hip
    r = I.philox_first(np.array([index]), 0, step, 0, SEED & 0xFFFFFFFF, SEED >> 32)
    assert int(r[0]) >> 8 == 0xFFFFFF                        # the planted case is what it claims to be
    x = torch.zeros((1, N), dtype=torch.bfloat16, device="cuda")
    x[0, 7] = 30.0                                           # the largest Gumbel noise of 24 bits is -log(-log(1 - 2^-25)) = 17.3: 7 wins
    sc = I.gumbel_scores(x[0].float().cpu().numpy(), 1.0, SEED, step, 0)
    assert int(sc.argmax()) == 7 and abs(sc[index] - 17.33) < 0.01
    rng = hip.make_rng(SEED, 1.0, "cuda")
    rng[2] = step
    out = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hip.sample_rows_bf16(x, out, torch.zeros(129, dtype=torch.int32, device="cuda"), rng)
    assert out.tolist() == [7], (out.tolist(), index)
    x[0, 7] = 0.0                                            # and among equal logits that draw does win, with its finite noise
    assert int(I.gumbel_scores(x[0].float().cpu().numpy(), 1.0, SEED, step, 0).argmax()) == index
    rng = hip.make_rng(SEED, 1.0, "cuda")
    rng[2] = step
    hip.sample_rows_bf16(x, out, torch.zeros(129, dtype=torch.int32, device="cuda"), rng)
    assert out.tolist() == [index]
