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
27-56 % of the elements have more than one admissible value.

The launch table (the tests named test_table8_*).  Every row of decode_check.TABLE8 - every batch depth, trip count, block size,
B, pair-form edge and long-K wave count of the e4m3 plan; tests/test_fp8_decode_check_cpu.py shows that the table reaches them
and that the check flags planted mistakes where they are planted - runs through its entry point with the route pinned in
ROUTES8 asserted first, per-row weight magnitudes (the scale of row n differs from that of rows n +- 1 and n +- 16, asserted on
every Case), targets pre-filled with sentinels and two guard rows behind them; a fused norm is read back through the bf16
identity form and passes check_norm at zero flags.
Measured on an MI355X: zero flags in all 175 rows and no route changed, so csrc/ is unchanged; implied accumulation error at
most 1.3e-8 T (pg8 1.2e-8, pgb8 1.3e-8); 14-50 % of the elements have more than one admissible value; the read-back norms at
most 0.065 of their bound with at most 0.39 % multi-valued elements.  SwiGLU at most 1.70 ulp (pg8 1.66, pgb8 1.70; ULP_BOUND
2.0), against 0.50 on the rows of N(0, 1 / K) above: with gate rows of up to 2^7 times that magnitude, gates reach -87 and
__expf's error, which grows with its argument, moves a few bf16(silu) by one ulp.  The 175 rows and the 12 other tests of the
table take 6.8 s together; the tests from before it take 26 s."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_check as D  # noqa: E402
import rowop_check as R  # noqa: E402
from decode_check import Case  # noqa: E402

pytestmark = pytest.mark.gpu
MEASURED = {}
TABLE8_MEASURED = {}
WORST = {}
SECONDS = {"table8": 0.0, "before": 0.0}


@pytest.fixture(scope="module", autouse=True)
def measured():
    yield
    for k, v in sorted(MEASURED.items()):
        print(f"[fp8 gemv] {k}: {v}")
    for k, v in sorted(TABLE8_MEASURED.items()):
        print(f"[fp8 gemv table] {k}: n {v['n']} multi {v['multi'] / max(v['n'], 1):.2%} implied error {v['max_d']:.2e} T "
              f"swiglu {v['max_ulps']:.2f} ulp")
    for k, v in sorted(WORST.items()):
        print(f"[fp8 gemv table] {k}: " + " ".join(f"{a} {b:.3e}" for a, b in sorted(v.items())))
    print(f"[fp8 gemv] seconds: the tests of the launch table {SECONDS['table8']:.1f}, the tests from before it {SECONDS['before']:.1f}")
    D._EYE.clear()


@pytest.fixture(autouse=True)
def seconds(request):
    t0 = time.perf_counter()
    yield
    SECONDS["table8" if request.node.name.startswith("test_table8") else "before"] += time.perf_counter() - t0


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


# ------------------------------------------------------------------------------------------------ the e4m3 launch table
def bits(t):
    return R.bits(t)


def table8_case(row):
    """The operands of a row of decode_check.TABLE8: per-row magnitudes, so the scale of every row differs from its neighbours'."""
    entry, form, B, N, K = row
    c = Case(form, B, N, K, seed=D.case_seed(row), row_scales=True)
    s = c.s.cpu()
    for d in (1, 16):
        assert bool((s[d:] != s[:-d]).all()), (row, d)
    return c


def operand8(hip, c, entry):
    """The activation the kernel multiplies: a fused norm is read back through the bf16 identity form of the same entry (the
    e4m3 kernels sum the squares in that kernel's lane layout and order) and itself checked against the fp64 RMSNorm."""
    A = c.activation(hip, "pgb" if D.ENTRIES[entry][0] else "pg")
    torch.cuda.synchronize()
    if c.norm:
        r = D.check_norm(A, c.x, c.nw)
        w = WORST.setdefault("norm " + entry, {})
        w["ratio"], w["multi_share"] = max(w.get("ratio", 0.0), r.max_ratio), max(w.get("multi_share", 0.0), r.multi_share)
        assert r.count == 0, r.report(what=f"norm read back for {entry} K={c.K}")
        assert r.multi_share <= R.MULTI_CAP, r.multi_share
    return A


@pytest.mark.parametrize("row", D.TABLE8, ids=D.case_id)
def test_table8_every_launch_plan_against_fp64(hip, row):
    """The pinned route, then zero flags with TAU and ULP_BOUND unchanged and no quantisation allowance; nothing stored behind the
    B rows."""
    entry, form, B, N, K = row
    assert hip.gemv_pg_route(*D.route_args(row)) == D.ROUTES8[row], row
    c = table8_case(row)
    A = operand8(hip, c, entry)
    got = c.run(hip, entry)
    chk = c.check(hip, got, A=A)
    D.record(f"{entry} {form}", chk, store=TABLE8_MEASURED)
    print(f"[fp8 gemv table] {D.case_id(row)}: flagged {chk.count} multi {chk.multi / chk.n:.2%} implied error {chk.max_d:.2e} T "
          f"swiglu {chk.max_ulps:.2f} ulp")
    assert chk.count == 0, chk.report(what=D.case_id(row))
    assert c.guard_clean(), "a row behind the B outputs was stored"


def flip_sign(c, n, lo_k, hi_k):
    """Negates the weight (n, k) of the quantised and of the dequantised matrix, k in [lo_k, hi_k) where the smallest |x| over
    the scenes times |w| is largest; returns k."""
    x, w = c.x.float().abs().min(0).values[lo_k:hi_k], c.wd[n, lo_k:hi_k].float().abs()
    k = lo_k + int((x * w).argmax())
    assert int(c.q[n, k]) & 0x7F
    c.q[n, k] = c.q[n, k] ^ 0x80
    c.wd[n, k] = -c.wd[n, k]
    return k


def one_output_moves(hip, c, entry, n, lo_k, hi_k):
    a = c.run(hip, entry).clone()
    assert c.guard_clean()
    flip_sign(c, n, lo_k, hi_k)
    b = c.run(hip, entry)
    changed = bits(a) != bits(b)
    assert changed[:, n].all() and int(changed.sum()) == c.B, (changed.nonzero().tolist()[:10], n)
    chk = c.check(hip, b)
    assert chk.count == 0, chk.report(what="after the flip")
    assert c.guard_clean()


@pytest.mark.parametrize("B,N", [(2, 16385), (4, 16385), (7, 8193)])
def test_table8_one_weight_byte_of_the_last_ragged_pair_moves_exactly_its_output(hip, B, N):
    """Pair form, NB = 2 and 4 (4 + 1 pairs) and NB = 8 (2 + 1): the sign of one weight byte in the second row of the last pair of
    wave 0's short batch is negated; that output changes in every scene, every other bit of the output stays, and the changed
    output still passes the check."""
    K = 256
    row = ("pgb8", "bias", B, N, K)
    form, threads, rb, kch = hip.gemv_pg_route(*D.route_args(row))
    uq, ur = divmod((N + 1) // 2, 2048)
    assert form == 2 and ur >= 1 and uq + 1 > rb and (uq + 1) % rb         # wave 0 has uq + 1 pairs: two trips, the last ragged
    one_output_moves(hip, table8_case(row), "pgb8", 2 * uq + 1, 0, K)


@pytest.mark.parametrize("B,N", [(3, 2100), (6, 1600)])
def test_table8_one_weight_byte_in_the_last_wave_s_share_moves_exactly_its_output(hip, B, N):
    """Long-K form at K = 8960 (S = 9; wave 8 holds k >= 8192), R = 8 with per = 9 (8 + 1) and R = 4 with per = 7 (4 + 3): the last
    row of block 0's short pass."""
    K = 8960
    form, threads, rb, kch = hip.gemv_pg_route(B, N, K, False, False, True)
    per = (N + 255) // 256
    assert (form, kch) == (3, 9) and per > rb and per % rb
    c = Case("bias", B, N, K, seed=900 + B, row_scales=True)
    one_output_moves(hip, c, "pgb8", per - 1, 8192, K)


TRIPS8 = [("pg8", "qkv", 8, 9217, 256), ("pgb8", "o", 4, 16385, 256), ("pgb8", "gu", 7, 8224, 256), ("pgb8", "down", 3, 2100, 2064)]


@pytest.mark.parametrize("row", TRIPS8, ids=D.case_id)
def test_table8_repeated_launches_of_a_shape_with_several_trips_are_bit_identical(hip, row):
    """One shape per kernel whose waves (blocks, in the long-K form) run two or more trips: 8 + 5 rows, 4 + 1 and 2 + 1 pairs,
    8 + 1 rows."""
    entry, form, B, N, K = row
    c = Case(form, B, N, K, seed=D.case_seed(row), row_scales=True)
    first = c.run(hip, entry).clone()
    for _ in range(3):
        assert torch.equal(bits(c.run(hip, entry)), bits(first)), row


@pytest.mark.parametrize("row", TRIPS8[1:], ids=D.case_id)
def test_table8_a_scene_of_a_shape_with_several_trips_does_not_depend_on_its_neighbours(hip, row):
    entry, form, B, N, K = row
    c = Case(form, B, N, K, seed=D.case_seed(row), row_scales=True)
    a = c.run(hip, entry).clone()
    c.x = c.x.clone()
    c.x[1:] = dev(rnd(B - 1, K, seed=777)).to(c.x.dtype)
    b = c.run(hip, entry)
    assert torch.equal(bits(a[0]), bits(b[0])), row
    for z in range(1, B):
        assert not torch.equal(bits(a[z]), bits(b[z])), (row, z)
