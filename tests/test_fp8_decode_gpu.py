"""GPU: the FP8 (e4m3) weight-only GEMVs of the decode step (csrc/decode_fp8.hip: g2v_gemv_pg_fp8, g2v_gemv_pg_batch_fp8).

The scale is a power of two, so the kernels compute a bf16 Linear on dequantize_rows(q, s): every form is checked element by
element with tests/gemm_check.py against the fp64 reference on the dequantised matrix (zero flags, the project's TAU and
ULP_BOUND, no quantisation allowance), and against the bf16 kernels on the same matrix.

The batch-1 entry is always driven with 8 different activation vectors (one launch each): with a single vector a swapped
weight-byte pair can go unflagged (tests/test_fp8_decode_cpu.py).

Fused-norm forms: the activation the kernel multiplies is read back exactly by running the bf16 hip.gemv_pg norm form against
a K x K identity matrix (its output is the normalised bf16 row; the fp8 kernels sum the squares in that kernel's lane layout
and order, so their rstd is the same number).

Measured on an MI355X: zero flags everywhere; SwiGLU at most 0.50 ulp; implied accumulation error at most 1.1e-8 T (TAU 1.5e-5);
27-56 % of the elements have more than one admissible value."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_check as D  # noqa: E402
from decode_check import Case  # noqa: E402

pytestmark = pytest.mark.gpu
MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def measured():
    yield
    for k, v in sorted(MEASURED.items()):
        print(f"[fp8 gemv] {k}: {v}")


@pytest.fixture(scope="module")
def hip():
    from g2vlm_amd import hip as h
    h.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return h


def dev(t):
    return t.cuda()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(); g.manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def record(name, chk):
    D.record(name, chk, store=MEASURED)


REAL = [("qkv", 2048, 1536), ("o", 1536, 1536), ("gu", 17920, 1536), ("down", 1536, 8960), ("lm", 151936, 1536)]
RAGGED = [("qkv", 7, 256), ("qkv", 300, 1536), ("lm", 1000, 256), ("gu", 96, 256), ("gu", 992, 1536),
          ("o", 7, 256), ("o", 300, 2064), ("o", 1000, 9216), ("down", 7, 9216), ("down", 300, 8960), ("down", 1000, 2064),
          ("bias", 7, 2064), ("bias", 1000, 256), ("bias", 300, 9216)]


@pytest.mark.parametrize("form,N,K", REAL + RAGGED, ids=lambda v: str(v))
def test_batch1_entry_every_form_against_fp64(hip, form, N, K):
    """g2v_gemv_pg_fp8 over 8 different activation vectors: zero flagged elements."""
    c = Case(form, 8, N, K, seed=100 + N % 97 + K % 89)
    got = c.run_fp8(hip, batched=False)
    chk = c.check(hip, got)
    record("batch1 " + form, chk)
    assert chk.count == 0, chk.report(what=f"gemv_pg_fp8 {form} N={N} K={K}")


@pytest.mark.parametrize("B", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("form,N,K", REAL + RAGGED, ids=lambda v: str(v))
def test_batched_entry_every_form_against_fp64(hip, form, N, K, B):
    """g2v_gemv_pg_batch_fp8 at B = 1, 2, 3, 5, 8: zero flagged elements, outputs pre-filled with NaN sentinels."""
    c = Case(form, B, N, K, seed=200 + N % 97 + K % 89 + B)
    got = c.run_fp8(hip, batched=True)
    chk = c.check(hip, got)
    record("batched " + form, chk)
    assert chk.count == 0, chk.report(what=f"gemv_pg_batch_fp8 {form} B={B} N={N} K={K}")


@pytest.mark.parametrize("batched", [False, True], ids=["batch1", "batched"])
@pytest.mark.parametrize("form,N,K", REAL + [("o", 1000, 2064), ("bias", 300, 9216)], ids=lambda v: str(v))
def test_against_the_bf16_kernels_on_the_dequantised_weights(hip, form, N, K, batched):
    """Both results lie in the same admissible sets, so they differ only where more than one value is admissible (34-57 % of
    the elements) and then by one bf16 ulp: rel < 2^-7 is the derived worst case (every element off by one ulp).
    Measured: rel between 0 (bit-identical: down, the bias forms) and 1.1e-5 (o at 1000 x 2064); gate/up 4.7e-6, lm_head 2.7e-6."""
    c = Case(form, 8, N, K, seed=300 + N % 97 + K % 89)
    a, b = c.run_fp8(hip, batched), c.run_bf16(hip, batched)
    if c.res0 is not None:
        a, b = a - c.res0, b - c.res0
    r = rel(a, b)
    MEASURED[f"vs bf16 {'batched' if batched else 'batch1'} {form} {N}x{K}"] = f"rel {r:.3e}"
    assert torch.isfinite(a.float()).all() and r < 2.0 ** -7, r


def test_repeated_launches_are_bit_identical(hip):
    """20 launches of each entry point, every real form."""
    for form, N, K in REAL[:4]:
        c = Case(form, 8, N, K, seed=400)
        for batched in (False, True):
            first = c.run_fp8(hip, batched)
            for _ in range(19):
                assert torch.equal(c.run_fp8(hip, batched).view(torch.int16 if first.dtype == torch.bfloat16 else torch.int32),
                                   first.view(torch.int16 if first.dtype == torch.bfloat16 else torch.int32)), (form, batched)


@pytest.mark.parametrize("B", [2, 3, 5, 8])
def test_a_row_of_the_batched_kernel_does_not_depend_on_its_neighbours(hip, B):
    for form, N, K in REAL[:4]:
        c = Case(form, B, N, K, seed=500 + B)
        a = c.run_fp8(hip, True)
        x_keep = c.x.clone()
        c.x = c.x.clone()
        c.x[1:] = dev(rnd(B - 1, K, seed=777)).to(c.x.dtype)
        b = c.run_fp8(hip, True)
        assert torch.equal(a[0], b[0]), form
        assert not torch.equal(a[1], b[1]), form
        c.x = x_keep


def test_b1_through_the_batched_entry_against_the_batch1_entry(hip):
    """B = 1 through the batched entry does NOT share its summation order with the batch-1 entry: at K <= 1536 the batched
    kernel streams a pair of rows in three passes (the middle pass is split between the two rows and summed first), at
    K > 1536 it cuts K over the waves of a block; the batch-1 kernel gives a wave the whole row in chunk order.  So no
    rel < 1e-6 is asserted (that bound is for a shared order); both entries pass the fp64 check above, and here they must agree
    to the derived bound of every element off by one bf16 ulp of the Linear, rel < 2^-7 on the increment of the residual.
    Measured: bit-identical (rel 0) for both forms on these operands."""
    for form, N, K in (("o", 1536, 1536), ("down", 1536, 8960)):
        c = Case(form, 1, N, K, seed=600)
        a, b = c.run_fp8(hip, True), c.run_fp8(hip, False)
        r = rel(a - c.res0, b - c.res0)
        MEASURED[f"B=1 batched vs batch1 {form}"] = f"rel {r:.3e}"
        assert r < 2.0 ** -7, (form, r)
