"""CPU (no GPU): the element-wise GEMM check of tests/gemm_check.py against an honest emulation and planted errors.

An honest emulation - a CPU fp32 matmul of the bf16 operands followed by the documented epilogue - must give zero flags for
every epilogue, the RES_F32 variants and cancellation-heavy rows.  Each planted error must be flagged where it was planted and
nowhere else, while the loose check the older GEMM tests use (assert_bf16_close of tests/test_kernels_gpu.py, copied here;
a global rel-L2 for fp32 outputs) accepts the same output.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_check as G  # noqa: E402


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def assert_bf16_close(got, ref, rl=4e-3, ulps=2.0):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape
    assert torch.isfinite(got).all()
    r = rel(got, ref)
    assert r < rl, f"rel-L2 {r}"
    tol = ulps * 2.0 ** -8 * ref.abs().clamp_min(ref.abs().max() * 2 ** -7)
    bad = ((got - ref).abs() > tol)
    assert bad.float().mean() < 2e-3, f"{int(bad.sum())} of {bad.numel()} elements off by > {ulps} bf16 ulp"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(); g.manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def operands(M, N, K, seed, cancel_rows=()):
    """A, W, bias (bf16); rows in cancel_rows cancel: their second K half is minus the first, and W's second K half is its
    first half perturbed by ~2^-6, so v* is ~1 % of T there."""
    A = rnd(M, K, seed=seed)
    W = rnd(N, K, seed=seed + 1, scale=K ** -0.5)
    h = K // 2
    W[:, h:] = W[:, :h] * (1 + 2.0 ** -6 * rnd(N, h, seed=seed + 2))
    for r in cancel_rows:
        A[r, h:] = -A[r, :h]
    return A.bfloat16(), W.bfloat16(), rnd(N, seed=seed + 3, scale=0.1).bfloat16()


def acc32(A, W):
    return A.float() @ W.float().T


def emulate(A, W, bias, epi, res=None, gamma=None, round_gamma=False, acc=None):
    """The documented epilogue applied to a CPU fp32 accumulation."""
    acc = acc32(A, W) if acc is None else acc
    if epi == G.EPI_SWIGLU:
        M, N = acc.shape
        gv = acc.view(M, N // 32, 2, 16)
        gt, up = gv[:, :, 0].reshape(M, N // 2).bfloat16().float(), gv[:, :, 1].reshape(M, N // 2).bfloat16().float()
        return (F.silu(gt).bfloat16().float() * up).bfloat16()
    v = (acc + (bias.float() if bias is not None else 0.0)).bfloat16()
    if epi == G.EPI_BF16:
        return v
    if epi == G.EPI_GELU:
        return F.gelu(v.float()).bfloat16()
    if epi == G.EPI_QUICKGELU:
        u = (v.float() * 1.702).bfloat16().float()
        return (v.float() * torch.sigmoid(u).bfloat16().float()).bfloat16()
    if epi == G.EPI_RES_F32:
        return G.res_f32(v, res, gamma, round_gamma)
    return G.res_bf16(v, res)


RES_F32_VARIANTS = {"gamma_round": (True, True, True), "gamma": (True, True, False), "res_only": (True, False, False),
                    "neither": (False, False, False), "gamma_no_res": (False, True, False)}


@pytest.mark.parametrize("epi", ["bf16", "gelu", "quickgelu", "swiglu", "res_bf16"] + [f"res_f32_{k}" for k in RES_F32_VARIANTS])
def test_honest_emulation_passes(epi):
    M, N, K = 96, 256, 512
    A, W, b = operands(M, N, K, seed=10, cancel_rows=(3, 40, 41))
    res = rnd(M, N, seed=20)
    gam = 1 + 0.1 * rnd(N, seed=21)
    kw = {}
    if epi.startswith("res_f32"):
        has_res, has_gam, rg = RES_F32_VARIANTS[epi[len("res_f32_"):]]
        e = G.EPI_RES_F32
        kw = dict(res=res if has_res else None, gamma=gam if has_gam else None, round_gamma=rg)
    else:
        e = {"bf16": G.EPI_BF16, "gelu": G.EPI_GELU, "quickgelu": G.EPI_QUICKGELU, "swiglu": G.EPI_SWIGLU, "res_bf16": G.EPI_RES_BF16}[epi]
        if e == G.EPI_RES_BF16:
            kw = dict(res=res.bfloat16())
    bias = None if e == G.EPI_SWIGLU else b
    got = emulate(A, W, bias, e, **kw)
    chk = G.check_gemm(got, A, W, bias, e, **kw)
    assert chk.count == 0, chk.report(what=epi)
    assert chk.max_d <= G.TAU
    # the cancellation rows do produce several admissible values
    lo, hi, nc = G.admissible(*G.linear64(A[[3, 40, 41]], W, bias))
    assert int((nc > 2).sum()) > 0


def test_reference_matches_exact_products():
    """linear64 is exact for small integer-valued operands (every partial sum is an integer below 2^53)."""
    g = torch.Generator(); g.manual_seed(5)
    A = torch.randint(-8, 9, (7, 64), generator=g).bfloat16()
    W = torch.randint(-8, 9, (9, 64), generator=g).bfloat16()
    v, T = G.linear64(A, W)
    ref = A.long() @ W.long().T
    assert torch.equal(v.long(), ref) and torch.equal(T.long(), A.long().abs() @ W.long().abs().T)


def test_key_is_monotone_and_invertible():
    x = torch.tensor([-3.0, -1.0, -2.0 ** -100, -0.0, 0.0, 2.0 ** -100, 1.0, 1.0078125, 3.0]).bfloat16()
    k = G.key(x)
    assert bool((k[1:] >= k[:-1]).all()) and int(k[3]) == int(k[4]) == 0
    assert int(G.key(torch.tensor([1.0078125]).bfloat16())) - int(G.key(torch.tensor([1.0]).bfloat16())) == 1
    assert torch.equal(G.from_key(k).float(), x.float())


# ------------------------------------------------------------------------------------------------ planted errors
M0, N0, K0 = 1500, 512, 320     # the issue's example shape: one 16 x 16 fragment is 0.03 % of the output


def _planted(epi, mutate, region, kw=None, loose=None, min_frac=0.9):
    """mutate(acc, A, W, bias) -> the wrong output; region = bool [M, N] where the error was planted.  Asserts: the
    honest output passes, the wrong one is flagged inside `region` only, on at least min_frac of the elements whose value
    changed (a one-ulp error stays admissible where v* lies within delta of the rounding boundary), and the loose check
    accepts it."""
    kw = kw or {}
    A, W, b = operands(M0, N0, K0, seed=30)
    acc = acc32(A, W)
    honest = emulate(A, W, b, epi, acc=acc, **kw)
    assert G.check_gemm(honest, A, W, b, epi, **kw).count == 0
    wrong = mutate(acc, A, W, b)
    chk = G.check_gemm(wrong, A, W, b, epi, **kw)
    changed = (wrong.float() != honest.float())
    assert not bool((chk.bad & ~region).any()), "flagged outside the planted region: " + chk.report(what="planted")
    assert not bool((chk.bad & ~changed).any())
    n_changed = int((changed & region).sum())
    assert n_changed > 0 and chk.count >= min_frac * n_changed, (chk.count, n_changed)
    if loose is None:
        ref = F.linear(A, W, b)                                  # torch's CPU bf16 Linear, as the older tests use
        assert_bf16_close(wrong, ref)
    else:
        loose(wrong, A, W, b)
    return chk


def _frag(r, c):
    m = torch.zeros((M0, N0), dtype=torch.bool)
    m[16 * r:16 * r + 16, 16 * c:16 * c + 16] = True
    return m


def test_planted_neighbour_column_bias():
    r, c = 37, 11
    def mutate(acc, A, W, b):
        bb = b.float().clone()
        bias_rows = bb.expand(M0, N0).clone()
        cols = torch.arange(16 * c, 16 * c + 16)
        bias_rows[16 * r:16 * r + 16, cols] = bb[cols + 1]
        return (acc + bias_rows).bfloat16()
    chk = _planted(G.EPI_BF16, mutate, _frag(r, c))
    assert chk.first()[0] // 16 == r and chk.first()[1] // 16 == c


def test_planted_dropped_term():
    row, k = 777, 123
    def mutate(acc, A, W, b):
        a2 = A.clone()
        a2[row, k] = 0
        return (acc32(a2, W) + b.float()).bfloat16()
    region = torch.zeros((M0, N0), dtype=torch.bool); region[row] = True
    chk = _planted(G.EPI_BF16, mutate, region)
    assert chk.flagged_rows() == [row]


def test_planted_truncation_instead_of_rne():
    r, c = 50, 20
    def mutate(acc, A, W, b):
        x = acc + b.float()
        v = x.bfloat16()
        trunc = (x.view(torch.int32) & ~0xFFFF).view(torch.float32).bfloat16()
        out = v.clone()
        out[16 * r:16 * r + 16, 16 * c:16 * c + 16] = trunc[16 * r:16 * r + 16, 16 * c:16 * c + 16]
        return out
    chk = _planted(G.EPI_BF16, mutate, _frag(r, c), min_frac=0.6)      # one ulp, on the ~half of the elements that round up
    assert chk.count >= 64


def test_planted_gamma_round_skipped_for_one_group():
    """Two groups of one RES_F32 launch (MoT o / down): GAMMA_ROUND_BF16 ignored for the rows of the second group."""
    split = 1100
    res = rnd(M0, N0, seed=40)
    gam = 1 + 0.1 * rnd(N0, seed=41)
    kw = dict(res=res, gamma=gam, round_gamma=True)
    def mutate(acc, A, W, b):
        out = emulate(A, W, b, G.EPI_RES_F32, acc=acc, **kw)
        out[split:] = emulate(A[split:], W, b, G.EPI_RES_F32, acc=acc[split:], res=res[split:], gamma=gam, round_gamma=False)
        return out
    region = torch.zeros((M0, N0), dtype=torch.bool); region[split:] = True
    def loose(wrong, A, W, b):
        assert rel(wrong, res + (F.linear(A, W, b) * gam).bfloat16()) < 2e-3
    _planted(G.EPI_RES_F32, mutate, region, kw, loose)


def test_planted_fma_contraction_of_unrounded_gamma():
    """DINO layer scale without rounding: res + lin * gamma contracted into one fma (the fold common.h warns about)."""
    res = rnd(M0, N0, seed=42)
    gam = 1 + 0.1 * rnd(N0, seed=43)
    kw = dict(res=res, gamma=gam, round_gamma=False)
    def mutate(acc, A, W, b):
        v = (acc + b.float()).bfloat16()
        return (v.double() * gam.double() + res.double()).float()     # one rounding: the fused multiply-add
    region = torch.ones((M0, N0), dtype=torch.bool)
    def loose(wrong, A, W, b):
        assert rel(wrong, F.linear(A, W, b) * gam + res) < 2e-3
    _planted(G.EPI_RES_F32, mutate, region, kw, loose)


def test_check_f32_bound():
    A, W, b = rnd(64, 1024, seed=50), rnd(96, 1024, seed=51, scale=1 / 32), rnd(96, seed=52)
    got = (A @ W.T + b)
    bad, ratio = G.check_f32(got, A, W, b)
    assert not bool(bad.any()) and ratio < 1
    got[5, 7] += 1e-3 * float(got[5].abs().max())
    bad, _ = G.check_f32(got, A, W, b)
    assert bad.nonzero().tolist() == [[5, 7]]
