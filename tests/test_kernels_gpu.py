"""GPU: every entry point of libg2vlm_hip.so against the CPU oracle / plain fp32 torch math.

Integer/index work is compared bit-exact; bf16 results are compared to the oracle's bf16 result
with a rel-L2 bound and a max error of a couple of bf16 ulps (fp32 accumulation order differs
between an MFMA tile loop and a CPU GEMM, which can flip a final bf16 rounding).
"""
import math
import os
import sys

import numpy as np

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import g2vlm_oracle as O  # noqa: E402  (checker only)


@pytest.fixture(scope="module")
def hip():
    from g2vlm_amd import hip as h
    h.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return h


def dev(t):
    return t.cuda()


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


# ----------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,N,K", [(1, 128, 64), (130, 256, 128), (257, 160, 160), (1000, 1536, 640), (77, 480, 1216)])
def test_gemm_bf16_plain_and_bias(hip, M, N, K):
    x, w, b = rnd(M, K, seed=1).bfloat16(), rnd(N, K, seed=2, scale=K ** -0.5).bfloat16(), rnd(N, seed=3).bfloat16()
    ref = F.linear(x, w, b)
    got = hip.linear(dev(x), dev(w), dev(b))
    assert_bf16_close(got, ref)
    got = hip.linear(dev(x), dev(w), None)
    assert_bf16_close(got, F.linear(x, w))


def test_gemm_bf16_strided_A_and_tail_k(hip):
    xb = rnd(300, 512, seed=4).bfloat16()
    x = xb[:, 128:128 + 264]                    # lda 512, K = 264 (multiple of 8, not of 64)
    w = rnd(192, 264, seed=5, scale=0.06).bfloat16()
    got = hip.linear(dev(xb)[:, 128:128 + 264], dev(w))
    assert_bf16_close(got, F.linear(x, w))


def test_gemm_epilogues(hip):
    M, N, K = 333, 384, 256
    x, w, b = rnd(M, K, seed=6).bfloat16(), rnd(N, K, seed=7, scale=K ** -0.5).bfloat16(), rnd(N, seed=8, scale=0.1).bfloat16()
    lin = F.linear(x, w, b)
    assert_bf16_close(hip.linear(dev(x), dev(w), dev(b), hip.EPI_GELU), F.gelu(lin))
    assert_bf16_close(hip.linear(dev(x), dev(w), dev(b), hip.EPI_QUICKGELU), lin * torch.sigmoid(1.702 * lin))
    res = rnd(M, N, seed=9)
    gam = 1 + 0.1 * rnd(N, seed=10)
    # DINO form: res + lin * gamma (fp32)
    got = hip.linear(dev(x), dev(w), dev(b), hip.EPI_RES_F32, res=dev(res), gamma=dev(gam))
    ref = lin * gam + res
    assert rel(got, ref) < 2e-3
    # MoT form: res + bf16(lin * gamma)
    got = hip.linear(dev(x), dev(w), None, hip.EPI_RES_F32, res=dev(res), gamma=dev(gam), flags=hip.GAMMA_ROUND_BF16)
    ref = res + (F.linear(x, w) * gam).bfloat16()
    assert rel(got, ref) < 2e-3
    # no residual, no gamma: plain fp32 copy of the bf16 Linear
    got = hip.linear(dev(x), dev(w), dev(b), hip.EPI_RES_F32)
    assert rel(got, lin.float()) < 2e-3
    # in place (C aliases res)
    r2 = dev(res).clone()
    hip.linear(dev(x), dev(w), dev(b), hip.EPI_RES_F32, out=r2, res=r2)
    assert rel(r2, res + lin) < 2e-3
    # bf16 residual stream (ViT)
    rb = res.bfloat16()
    got = hip.linear(dev(x), dev(w), dev(b), hip.EPI_RES_BF16, res=dev(rb))
    assert_bf16_close(got, rb + lin)


def test_gemm_swiglu_interleaved(hip):
    M, K, Fd = 200, 256, 320
    x = rnd(M, K, seed=11).bfloat16()
    wg, wu = rnd(Fd, K, seed=12, scale=K ** -0.5).bfloat16(), rnd(Fd, K, seed=13, scale=K ** -0.5).bfloat16()
    from g2vlm_amd.weights import interleave_gate_up
    w = interleave_gate_up(wg, wu)
    got = hip.linear(dev(x), dev(w), None, hip.EPI_SWIGLU)
    ref = F.silu(F.linear(x, wg)) * F.linear(x, wu)
    assert got.shape == (M, Fd)
    assert_bf16_close(got, ref)


def test_gemm_grouped_two_experts(hip):
    K, N = 256, 384
    xa, xb = rnd(300, K, seed=14).bfloat16(), rnd(5, K, seed=15).bfloat16()
    wa, wb = rnd(N, K, seed=16, scale=K ** -0.5).bfloat16(), rnd(N, K, seed=17, scale=K ** -0.5).bfloat16()
    ba, bb = rnd(N, seed=18).bfloat16(), rnd(N, seed=19).bfloat16()
    x = dev(torch.cat([xa, xb]))
    out = torch.empty((305, N), dtype=torch.bfloat16, device="cuda")
    hip.gemm_bf16([dict(A=x[:300], W=dev(wa), bias=dev(ba), C=out[:300], M=300),
                   dict(A=x[300:], W=dev(wb), bias=dev(bb), C=out[300:], M=5)], N, K, hip.EPI_BF16, out_ld=N)
    assert_bf16_close(out[:300], F.linear(xa, wa, ba))
    assert_bf16_close(out[300:], F.linear(xb, wb, bb))


@pytest.mark.parametrize("epi", ["bf16", "gelu", "swiglu", "res_f32", "res_bf16", "quickgelu"])
def test_gemm_big_tile_matches_small_tile_and_oracle(hip, epi):
    """The 256-wide DMA-staged kernel (K % 64 == 0, N % 256 == 0, >= 512 rows) against torch and the 128x128 kernel."""
    M, N, K = 1500, 512, 320
    x, w, b = rnd(M, K, seed=200).bfloat16(), rnd(N, K, seed=201, scale=K ** -0.5).bfloat16(), rnd(N, seed=202, scale=0.1).bfloat16()
    lin = F.linear(x, w, b)
    res32, gam = rnd(M, N, seed=203), 1 + 0.1 * rnd(N, seed=204)
    kw, ref = {}, None
    if epi == "bf16":
        e, ref = hip.EPI_BF16, lin
    elif epi == "gelu":
        e, ref = hip.EPI_GELU, F.gelu(lin)
    elif epi == "quickgelu":
        e, ref = hip.EPI_QUICKGELU, lin * torch.sigmoid(1.702 * lin)
    elif epi == "swiglu":
        e, b = hip.EPI_SWIGLU, None
        gv = F.linear(x, w).view(M, N // 32, 2, 16)
        ref = (F.silu(gv[:, :, 0]) * gv[:, :, 1]).reshape(M, N // 2)
    elif epi == "res_f32":
        e, kw = hip.EPI_RES_F32, dict(res=dev(res32), gamma=dev(gam), flags=hip.GAMMA_ROUND_BF16)
        ref = res32 + (lin * gam).bfloat16()
    else:
        e, kw = hip.EPI_RES_BF16, dict(res=dev(res32.bfloat16()))
        ref = res32.bfloat16() + lin
    bd = dev(b) if b is not None else None
    kw_big = dict(kw); kw_big["flags"] = kw.get("flags", 0) | hip.FORCE_BIG_TILE
    big = hip.linear(dev(x), dev(w), bd, e, **kw_big)
    kw_small = dict(kw); kw_small["flags"] = kw.get("flags", 0) | hip.FORCE_SMALL_TILE
    small = hip.linear(dev(x), dev(w), bd, e, **kw_small)
    if big.dtype == torch.float32:
        assert rel(big, ref) < 2e-3 and rel(big, small) < 2e-3
    else:
        assert_bf16_close(big, ref)
        assert_bf16_close(big, small)


def test_gemm_big_tile_grouped_and_odd_rows(hip):
    K, N = 256, 768
    xa, xb = rnd(2741, K, seed=210).bfloat16(), rnd(6, K, seed=211).bfloat16()
    wa, wb = rnd(N, K, seed=212, scale=K ** -0.5).bfloat16(), rnd(N, K, seed=213, scale=K ** -0.5).bfloat16()
    x = dev(torch.cat([xa, xb]))
    out = torch.zeros((2747 + 3, N), dtype=torch.bfloat16, device="cuda")
    hip.gemm_bf16([dict(A=x[:2741], W=dev(wa), C=out[:2741], M=2741), dict(A=x[2741:], W=dev(wb), C=out[2741:2747], M=6)],
                  N, K, hip.EPI_BF16, out_ld=N, flags=hip.FORCE_BIG_TILE)
    assert_bf16_close(out[:2741], F.linear(xa, wa))
    assert_bf16_close(out[2741:2747], F.linear(xb, wb))
    assert float(out[2747:].abs().max()) == 0            # nothing written past the last valid row


@pytest.mark.parametrize("epi", ["bf16", "gelu", "swiglu", "res_f32", "res_bf16", "quickgelu"])
@pytest.mark.parametrize("M,N,K,hflag", [(1500, 512, 320, 512), (700, 256, 128, 128), (513, 768, 1216, 256), (1111, 512, 192, 0),
                                         (1500, 512, 320, 512 | 1024), (513, 768, 1216, 128 | 1024), (2100, 256, 64 * 7, 256 | 1024),
                                         (1500, 512, 320, 4096), (577, 256, 128, 4096), (1000, 512, 1216, 8192), (700, 768, 192, 16384),
                                         (1500, 512, 320, 512 | 32768), (1000, 512, 1216, 8192 | 32768), (700, 768, 192, 16384 | 32768),
                                         (1500, 512, 320, 512 | 65536), (700, 256, 128, 256 | 65536), (513, 768, 1216, 128 | 65536),
                                         (1111, 512, 192, 65536), (2100, 256, 64 * 7, 8192 | 65536), (700, 768, 192, 16384 | 65536),
                                         (577, 256, 128, 4096 | 65536), (300, 1024, 64 * 4, 512 | 65536),
                                         (1500, 512, 320, 4096 | 65536), (1000, 512, 1216, 4096 | 65536),
                                         (1500, 512, 320, 512 | 131072), (513, 768, 1216, 256 | 131072), (1111, 512, 192, 131072),
                                         (577, 256, 128, 4096 | 131072), (1000, 512, 1216, 8192 | 131072), (700, 768, 192, 16384 | 131072)])
def test_gemm_8phase_matches_small_tile_and_oracle(hip, epi, M, N, K, hflag):
    """The 256x256 8-phase kernel (gemm_8p.hip; K % 64 == 0, N % 256 == 0, K >= 128) against torch and the 128x128 kernel:
    odd row counts (partial last row tile), K of 2 / 3 / 5 / 19 K-tiles (shortest ring, odd tile counts), tile heights
    256 / 192 / 128 / 288 / 224 / 160 forced by the A/B flags 512 / 128 / 256 / 4096 / 8192 / 16384 (0 = the launcher's
    own choice; the odd heights deal one DMA instruction more to waves 0-3 than to waves 4-7).  65536 is the four-wave form
    (the launcher's own choice for long-K and fp32-residual Linears; gemm_4w.hip: one wave per SIMD, accumulators in owned AGPRs; 2 / 3 / 4 / 5 / 7 / 19 K-tiles = every
    prologue / tail path of its two-K-tile loop; the 288-row tile keeps its ninth m-fragment's accumulators in VGPRs).  The
    eight-wave loops of gemm_8p.hip: 131072 = two-barrier template with the two wave rows staggered by one barrier (round 2's
    default), 1024 the same loop in lockstep, 32768 the software-pipelined loop of round 1."""
    x, w, b = rnd(M, K, seed=300).bfloat16(), rnd(N, K, seed=301, scale=K ** -0.5).bfloat16(), rnd(N, seed=302, scale=0.1).bfloat16()
    lin = F.linear(x, w, b)
    res32, gam = rnd(M, N, seed=303), 1 + 0.1 * rnd(N, seed=304)
    kw, ref = {}, None
    if epi == "bf16":
        e, ref = hip.EPI_BF16, lin
    elif epi == "gelu":
        e, ref = hip.EPI_GELU, F.gelu(lin)
    elif epi == "quickgelu":
        e, ref = hip.EPI_QUICKGELU, lin * torch.sigmoid(1.702 * lin)
    elif epi == "swiglu":
        e, b = hip.EPI_SWIGLU, None
        gv = F.linear(x, w).view(M, N // 32, 2, 16)
        ref = (F.silu(gv[:, :, 0]) * gv[:, :, 1]).reshape(M, N // 2)
    elif epi == "res_f32":
        e, kw = hip.EPI_RES_F32, dict(res=dev(res32), gamma=dev(gam), flags=hip.GAMMA_ROUND_BF16)
        ref = res32 + (lin * gam).bfloat16()
    else:
        e, kw = hip.EPI_RES_BF16, dict(res=dev(res32.bfloat16()))
        ref = res32.bfloat16() + lin
    bd = dev(b) if b is not None else None
    kw8 = dict(kw); kw8["flags"] = kw.get("flags", 0) | hip.FORCE_8P | hflag
    got = hip.linear(dev(x), dev(w), bd, e, **kw8)
    kw_small = dict(kw); kw_small["flags"] = kw.get("flags", 0) | hip.FORCE_SMALL_TILE
    small = hip.linear(dev(x), dev(w), bd, e, **kw_small)
    if got.dtype == torch.float32:
        assert rel(got, ref) < 2e-3 and rel(got, small) < 2e-3
    else:
        assert_bf16_close(got, ref)
        assert_bf16_close(got, small)
    # bit-identical to the 128x128 kernel: same MFMA shape, same k order within a tile row, same epilogue roundings
    assert torch.equal(got, small)


@pytest.mark.parametrize("M,N,K,epi", [(10968, 1536, 8960, "res_f32"), (10968, 17920, 1536, "swiglu"), (10992, 1024, 4096, "res_f32"),
                                       (5848, 2048, 1536, "bf16"), (4096, 4096, 4096, "bf16")])
def test_gemm_8phase_staggered_loop_race_screen(hip, M, N, K, epi):
    """The staggered main loop is a sync-structure edit (one wave row runs a barrier behind the other): its LDS-DMA -> ds_read
    and ds_read -> restage distances were re-derived (csrc/gemm_8p.hip), and this screens them the way the guide asks - real
    shapes with many tiles per persistent workgroup, 40 back-to-back launches each (the chip busy, DMA latencies varying), every
    result bit-identical to the lockstep two-barrier loop and to the software-pipelined loop of round 1.  A race shows as a
    rare wrong tile."""
    x, w = dev(rnd(M, K, seed=330).bfloat16()), dev(rnd(N, K, seed=331, scale=K ** -0.5).bfloat16())
    kw = {}
    if epi == "res_f32":
        e = hip.EPI_RES_F32
        res0, gam = dev(rnd(M, N, seed=332)), dev(1 + 0.1 * rnd(N, seed=333))
        run = lambda fl: hip.linear(x, w, None, e, res=res0, gamma=gam, flags=hip.GAMMA_ROUND_BF16 | hip.FORCE_8P | fl,          # noqa: E731
                                    out=torch.empty((M, N), dtype=torch.float32, device="cuda"))
    else:
        e = hip.EPI_SWIGLU if epi == "swiglu" else hip.EPI_BF16
        run = lambda fl: hip.linear(x, w, None, e, flags=hip.FORCE_8P | fl)                                                     # noqa: E731
    ref = run(hip.P8_TWO_BARRIER)
    assert torch.equal(run(hip.P8_PIPELINED), ref)
    bad = bad4 = 0
    for _ in range(40):
        bad += int(not torch.equal(run(hip.P8_EIGHT_WAVES), ref))
        bad4 += int(not torch.equal(run(hip.P8_FOUR_WAVES), ref))     # gemm_4w.hip: hand-placed loads, counted vmcnt, owned AGPRs
    assert bad == 0 and bad4 == 0, (bad, bad4)


@pytest.mark.parametrize("epi", ["bf16", "gelu", "swiglu", "res_f32", "res_bf16", "quickgelu"])
@pytest.mark.parametrize("M,N,K", [(8, 2048, 1536), (1, 256, 128), (16, 512, 8960), (23, 160, 320), (57, 1536, 1536), (64, 96, 64),
                                   (2, 1536, 8960), (8, 17920, 1536), (40, 1536, 8960)])
def test_gemm_skinny_rows(hip, epi, M, N, K):
    """gemm_skinny.hip (M <= 64: weight-streaming MFMA GEMV with in-workgroup split-K) against torch; the dispatcher takes
    it whenever one group has <= 64 rows and K % 64 == 0.  Summation order differs from the tiled kernels, so the check
    is the usual bf16 tolerance, plus agreement with the 128x128 kernel to 1 bf16 ulp."""
    x, w, b = rnd(M, K, seed=400).bfloat16(), rnd(N, K, seed=401, scale=K ** -0.5).bfloat16(), rnd(N, seed=402, scale=0.1).bfloat16()
    if epi == "swiglu" and N % 32:
        pytest.skip("SwiGLU needs N % 32 == 0")
    lin = F.linear(x, w, b)
    res32, gam = rnd(M, N, seed=403), 1 + 0.1 * rnd(N, seed=404)
    kw, ref = {}, None
    if epi == "bf16":
        e, ref = hip.EPI_BF16, lin
    elif epi == "gelu":
        e, ref = hip.EPI_GELU, F.gelu(lin)
    elif epi == "quickgelu":
        e, ref = hip.EPI_QUICKGELU, lin * torch.sigmoid(1.702 * lin)
    elif epi == "swiglu":
        e, b = hip.EPI_SWIGLU, None
        gv = F.linear(x, w).view(M, N // 32, 2, 16)
        ref = (F.silu(gv[:, :, 0]) * gv[:, :, 1]).reshape(M, N // 2)
    elif epi == "res_f32":
        e, kw = hip.EPI_RES_F32, dict(res=dev(res32), gamma=dev(gam), flags=hip.GAMMA_ROUND_BF16)
        ref = res32 + (lin * gam).bfloat16()
    else:
        e, kw = hip.EPI_RES_BF16, dict(res=dev(res32.bfloat16()))
        ref = res32.bfloat16() + lin
    bd = dev(b) if b is not None else None
    got = hip.linear(dev(x), dev(w), bd, e, **kw)                       # default dispatch -> skinny
    kw_small = dict(kw); kw_small["flags"] = kw.get("flags", 0) | hip.FORCE_SMALL_TILE
    small = hip.linear(dev(x), dev(w), bd, e, **kw_small)
    if got.dtype == torch.float32:
        assert rel(got, ref) < 2e-3 and rel(got, small) < 2e-3
    else:
        assert_bf16_close(got, ref)
        assert_bf16_close(got, small, ulps=1.01)


def test_gemm_skinny_split_k_deterministic_and_workspace_free(hip):
    """The cross-workgroup K split (partials in the caller's workspace, ticketed last-arrival reduce in slice order):
    repeated launches are bit-identical, the tickets return to zero, a caller-owned workspace gives the same bits as the
    default one, and a workspace too small for the split falls back to the in-workgroup split within bf16 tolerance."""
    M, N, K = 8, 1536, 8960
    x, w = dev(rnd(M, K, seed=420).bfloat16()), dev(rnd(N, K, seed=421, scale=K ** -0.5).bfloat16())
    ref = F.linear(x.float().cpu(), w.float().cpu())
    own = torch.zeros(hip.GEMM_WS_WORDS, dtype=torch.int32, device="cuda")
    outs = [hip.linear(x, w, ws=own) for _ in range(50)] + [hip.linear(x, w)]
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    assert int(own[:N // 16].abs().max()) == 0                          # tickets reset themselves
    assert_bf16_close(outs[0], ref)
    tiny = torch.zeros(64, dtype=torch.int32, device="cuda")            # no room for partials
    assert_bf16_close(hip.linear(x, w, ws=tiny), ref)


def test_gemm_skinny_cross_workgroup_reduce_stress(hip):
    """the split-K hand-off between workgroups (relaxed agent-scope stores / loads + a ticket, no fence) leans on
    gfx950's sc1 behaviour.  600 back-to-back launches over three shapes whose slices land on different XCDs, alternating
    inputs so that a stale partial from the previous launch would show: every result equals the first of its kind bit for bit."""
    assert hip.lib().g2v_arch() == b"gfx950"
    for M, N, K in ((8, 1536, 8960), (2, 2048, 1536), (16, 1536, 1536)):
        xs = [dev(rnd(M, K, seed=430 + i).bfloat16()) for i in range(2)]
        w = dev(rnd(N, K, seed=433, scale=K ** -0.5).bfloat16())
        first = [hip.linear(x, w).clone() for x in xs]
        assert not torch.equal(first[0], first[1])
        bad = 0
        for it in range(200):
            bad += int(not torch.equal(hip.linear(xs[it & 1], w), first[it & 1]))
        assert bad == 0, (M, N, K, bad)


def test_gemm_skinny_grouped_with_empty_group_and_strides(hip):
    """A two-group descriptor whose second group is empty (text prefill: no geo rows) still takes the skinny path;
    lda > K and an output row stride > N are honoured and nothing is written outside the M x N block."""
    M, N, K = 8, 512, 256
    xs = torch.zeros((M, K + 64), dtype=torch.bfloat16); xs[:, :K] = rnd(M, K, seed=410).bfloat16()
    w = rnd(N, K, seed=411, scale=K ** -0.5).bfloat16()
    x = dev(xs)
    out = torch.zeros((M + 2, N + 32), dtype=torch.bfloat16, device="cuda")
    hip.gemm_bf16([dict(A=x, W=dev(w), C=out, M=0), dict(A=x, W=dev(w), C=out, M=M)], N, K, hip.EPI_BF16, out_ld=N + 32, lda=K + 64)
    assert_bf16_close(out[:M, :N], F.linear(xs[:, :K], w))
    assert float(out[M:].abs().max()) == 0 and float(out[:, N:].abs().max()) == 0


@pytest.mark.parametrize("form", [131072, 65536])
def test_gemm_8phase_gelu_elementwise_vs_torch(hip, form):
    """GELU epilogue of the 8-phase kernel (erfc fit instead of libm erff) on a dense sweep of bf16 inputs through an
    identity weight: every value within 1 bf16 ulp of torch's erf-GELU; exactly equal for x >= -3.  Below -3 the
    reference's own 1 + erf(x/sqrt 2) is fp32 cancellation noise (torch's bf16 result differs from the fp64-exact one on
    ~12 % of such inputs, ours on ~11 %), so only the 1-ulp bound is asserted there."""
    K = N = 256
    M = 2048
    xs = torch.cat([torch.linspace(-9, 9, M * K // 2), torch.randn(M * K // 2) * 2]).bfloat16().view(M, K)
    eye = torch.eye(K).bfloat16()
    got = hip.linear(dev(xs), dev(eye), None, hip.EPI_GELU, flags=hip.FORCE_8P | form)
    ref = F.gelu(xs.float()).bfloat16()
    assert_bf16_close(got, ref, ulps=1.01)
    keep = xs.float() >= -3
    mism = (got.cpu() != ref)[keep].float().mean().item()
    assert mism < 1e-3, mism


@pytest.mark.parametrize("form", [131072, 65536])
def test_gemm_8phase_grouped_strided_and_no_overrun(hip, form):
    """Two groups (the MoT launch: geo rows + a few und rows, each with its own weights), lda > K, nothing written past the last
    valid row, group order irrelevant - in the eight-wave (131072) and the four-wave (65536) form of the tile."""
    K, N = 256, 768
    xa, xb = rnd(2741, K, seed=310).bfloat16(), rnd(6, K, seed=311).bfloat16()
    wa, wb = rnd(N, K, seed=312, scale=K ** -0.5).bfloat16(), rnd(N, K, seed=313, scale=K ** -0.5).bfloat16()
    xs = torch.zeros((2747, K + 64), dtype=torch.bfloat16)                 # lda > K
    xs[:2741, :K], xs[2741:, :K] = xa, xb
    x = dev(xs)
    out = torch.zeros((2747 + 3, N), dtype=torch.bfloat16, device="cuda")
    hip.gemm_bf16([dict(A=x[:2741], W=dev(wa), C=out[:2741], M=2741), dict(A=x[2741:], W=dev(wb), C=out[2741:2747], M=6)],
                  N, K, hip.EPI_BF16, out_ld=N, lda=K + 64, flags=hip.FORCE_8P | form)
    assert_bf16_close(out[:2741], F.linear(xa, wa))
    assert_bf16_close(out[2741:2747], F.linear(xb, wb))
    assert float(out[2747:].abs().max()) == 0            # nothing written past the last valid row
    # the small group first (the launcher orders groups large-first internally)
    out2 = torch.zeros((2747, N), dtype=torch.bfloat16, device="cuda")
    x2 = dev(torch.cat([xb, xa]))
    hip.gemm_bf16([dict(A=x2[:6], W=dev(wb), C=out2[:6], M=6), dict(A=x2[6:], W=dev(wa), C=out2[6:], M=2741)],
                  N, K, hip.EPI_BF16, out_ld=N, flags=hip.FORCE_8P | form)
    assert torch.equal(out2[:6], out[2741:2747]) and torch.equal(out2[6:], out[:2741])


@pytest.mark.parametrize("M,N,K,relu", [(100, 588, 1024, False), (333, 512, 512, True), (7, 9, 512, False)])
def test_gemm_f32(hip, M, N, K, relu):
    x, w, b = rnd(M, K, seed=20), rnd(N, K, seed=21, scale=K ** -0.5), rnd(N, seed=22)
    res = rnd(M, N, seed=23)
    ref = F.linear(x.double(), w.double(), b.double())
    if relu:
        ref = F.relu(ref)
    got = hip.gemm_f32(dev(x), dev(w), dev(b), relu=relu)
    assert rel(got, ref) < 2e-6
    got = hip.gemm_f32(dev(x), dev(w), dev(b), relu=relu, res=dev(res))
    assert rel(got, ref + res.double()) < 2e-6


# ---------------------------------------------------------------------------------------- norms
@pytest.mark.parametrize("C", [128, 160, 1024, 1536])
def test_layernorm(hip, C):
    x = rnd(37, C, seed=24) * 3 + 0.5
    w, b = 1 + 0.1 * rnd(C, seed=25), 0.1 * rnd(C, seed=26)
    ref = F.layer_norm(x, (C,), w, b, 1e-6)
    assert rel(hip.layernorm(dev(x), dev(w), dev(b), 1e-6, torch.float32), ref) < 1e-6
    assert_bf16_close(hip.layernorm(dev(x), dev(w), dev(b), 1e-6, torch.bfloat16), ref.bfloat16(), ulps=1.01)
    xb = x.bfloat16()
    ref = F.layer_norm(xb.float(), (C,), w, b, 1e-6)
    assert_bf16_close(hip.layernorm(dev(xb), dev(w), dev(b), 1e-6, torch.bfloat16), ref.bfloat16(), ulps=1.01)


def test_rmsnorm_routed(hip):
    C, M, split = 1536, 50, 41
    x = rnd(M, C, seed=27) * 2
    w0, w1 = 1 + 0.1 * rnd(C, seed=28), 1 + 0.1 * rnd(C, seed=29)
    h = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6)
    ref = torch.cat([w0 * h[:split], w1 * h[split:]])
    assert rel(hip.rmsnorm(dev(x), dev(w0), dev(w1), split, 1e-6, torch.float32), ref) < 1e-6
    assert_bf16_close(hip.rmsnorm(dev(x), dev(w0), dev(w1), split, 1e-6, torch.bfloat16), ref.bfloat16(), ulps=1.01)


# --------------------------------------------------------------------------- rope / qk-norm / cache
def test_mrope_table_matches_oracle(hip):
    L = 300
    g = torch.Generator(); g.manual_seed(30)
    pos = torch.randint(0, 45000, (3, L), generator=g)
    cos, sin = O.mrope_tables(pos, 1e6)
    inv = 1.0 / (1e6 ** (torch.arange(0, 128, 2, dtype=torch.int64).float() / 128))
    c, s = hip.mrope_table(dev(pos.to(torch.int32)), dev(inv))
    assert (c.cpu() - cos).abs().max() < 2e-6 and (s.cpu() - sin).abs().max() < 2e-6


@pytest.mark.parametrize("und", [0, 1])
def test_qknorm_mrope_cache(hip, und):
    L, Hq, Hkv, split, T0 = 45, 12, 2, 40, 8
    qkv = rnd(L, (Hq + 2 * Hkv) * 128, seed=31).bfloat16()
    ws = [1 + 0.1 * rnd(128, seed=32 + i) for i in range(4)]         # q_lo q_hi k_lo k_hi
    g = torch.Generator(); g.manual_seed(40)
    pos = torch.randint(0, 2000, (3, L), generator=g)
    cos, sin = O.mrope_tables(pos, 1e6)

    def norm(x, w):                                                  # Qwen2RMSNorm
        dt = x.dtype
        h = x.float()
        h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + 1e-6)
        return w * h.to(dt)

    q = qkv[:, :Hq * 128].view(L, Hq, 128)
    k = qkv[:, Hq * 128:(Hq + Hkv) * 128].view(L, Hkv, 128)
    v = qkv[:, (Hq + Hkv) * 128:].view(L, Hkv, 128)
    if not und:
        q, k = q.float(), k.float()
    qn = torch.cat([norm(q[:split], ws[0]), norm(q[split:], ws[1])])
    kn = torch.cat([norm(k[:split], ws[2]), norm(k[split:], ws[3])])
    c, s = cos[:, None, :], sin[:, None, :]
    qr = ((qn * c) + (O.rotate_half(qn) * s)).bfloat16()
    kr = ((kn * c) + (O.rotate_half(kn) * s)).bfloat16()
    rows = torch.arange(L, dtype=torch.int32) + T0
    kc = torch.zeros((T0 + L, Hkv, 128), dtype=torch.bfloat16, device="cuda")
    vc = torch.zeros_like(kc)
    qo = torch.empty((L, Hq, 128), dtype=torch.bfloat16, device="cuda")
    hip.qknorm_mrope_cache(dev(qkv), Hq, Hkv, *[dev(w) for w in ws], split, 1e-6, und, dev(cos), dev(sin), qo, kc, vc,
                           dev(rows))
    assert_bf16_close(qo, qr, ulps=1.01)
    assert_bf16_close(kc[T0:], kr, ulps=1.01)
    assert torch.equal(vc[T0:].cpu(), v)
    assert float(kc[:T0].abs().max()) == 0


@pytest.mark.parametrize("D", [96, 40])          # 96: four pairs per lane (8-byte accesses); 40: the scalar form (D % 16 != 0)
def test_rope2d_bf16_tables(hip, D):
    N, P, Hh = 2, 35, 16
    x = rnd(N * P, 3 * Hh * D, seed=41).bfloat16()
    pos = torch.cartesian_prod(torch.arange(5), torch.arange(7))      # [35,2]
    cos, sin = O.rope2d_tables(D // 2, 7, torch.bfloat16)
    xd = dev(x).clone()
    hip.rope2d(xd, 0, 2 * Hh, D, dev(cos), dev(sin), dev(pos.to(torch.int32)), P)
    qkv = x.view(N, P, 3, Hh, D).transpose(1, 3)                      # [N,H,3,P,D]
    pp = pos.view(1, P, 2).expand(N, -1, -1)
    q = O.rope2d(qkv[:, :, 0], pp); k = O.rope2d(qkv[:, :, 1], pp)
    got = xd.cpu().view(N, P, 3, Hh, D).transpose(1, 3)
    assert torch.equal(got[:, :, 0], q) and torch.equal(got[:, :, 1], k)   # bf16 arithmetic is reproduced exactly
    assert torch.equal(got[:, :, 2], qkv[:, :, 2])


def test_rope_vision(hip):
    L, Hh, D = 64, 16, 80
    x = rnd(L, 3 * Hh * D, seed=42).bfloat16()
    ang = rnd(L, D // 2, seed=43) * 3
    emb = torch.cat([ang, ang], -1)
    cos, sin = emb.cos(), emb.sin()
    xd = dev(x).clone()
    hip.rope_vision(xd, 2 * Hh, D, dev(cos), dev(sin))
    qk = x[:, :2 * Hh * D].view(L, 2 * Hh, D).float()
    ref = ((qk * cos[:, None]) + (O.rotate_half(qk) * sin[:, None])).bfloat16()
    assert_bf16_close(xd[:, :2 * Hh * D].view(L, 2 * Hh, D), ref, ulps=1.01)
    assert torch.equal(xd[:, 2 * Hh * D:].cpu(), x[:, 2 * Hh * D:])


# ------------------------------------------------------------------------------------ attention
def _attn_case(hip, Lq, Lk, Hq, Hkv, D, windows, seed, ld_extra=0, max_blocks=None, tile_rows=128):
    q = rnd(Lq, Hq * D + ld_extra, seed=seed).bfloat16()
    k = rnd(Lk, Hkv * D + ld_extra, seed=seed + 1).bfloat16()
    v = rnd(Lk, Hkv * D + ld_extra, seed=seed + 2).bfloat16()
    out = torch.full((Lq, Hq * D), float("nan"), dtype=torch.bfloat16, device="cuda")
    out.zero_()
    plan = hip.make_attn_plan(windows, Hq, "cuda", max_blocks=max_blocks, tile_rows=tile_rows)
    qd, kd, vd = dev(q), dev(k), dev(v)
    hip.flash_attn(qd[:, :Hq * D], kd[:, :Hkv * D], vd[:, :Hkv * D], out, plan, Hq, Hkv, D)
    ref = torch.zeros((Lq, Hq, D))
    for (qs, ql, ks, kl, causal) in windows:
        r = O.varlen_attention(q[:, :Hq * D].view(Lq, Hq, D).float(), k[:, :Hkv * D].view(Lk, Hkv, D).float(),
                               v[:, :Hkv * D].view(Lk, Hkv, D).float(), [0, qs, qs + ql], [0, ks, ks + kl], causal)
        ref[qs:qs + ql] = r[qs:qs + ql]
    return out.view(Lq, Hq, D), ref


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 12, 2), (64, 16, 16), (96, 16, 16), (80, 4, 4), (16, 16, 16)])
def test_flash_attn_noncausal_single_window(hip, D, Hq, Hkv):
    got, ref = _attn_case(hip, 333, 401, Hq, Hkv, D, [(0, 333, 0, 401, False)], seed=50 + D)
    assert rel(got, ref) < 6e-3
    assert (got.float().cpu() - ref).abs().max() < 0.05


def test_flash_attn_windows_and_uncovered_rows(hip):
    # DINO-style mis-sized windows (H1): three windows of 70 over 3*75 rows; the last 15 rows stay 0
    D, H = 64, 4
    got, ref = _attn_case(hip, 225, 225, H, H, D, [(0, 70, 0, 70, False), (70, 70, 70, 70, False), (140, 70, 140, 70, False)], 60)
    assert rel(got[:210], ref[:210]) < 6e-3
    assert float(got[210:].abs().max()) == 0


@pytest.mark.parametrize("Lq,Lk", [(8, 8), (40, 300), (200, 200), (129, 130)])
def test_flash_attn_causal_bottom_right(hip, Lq, Lk):
    got, ref = _attn_case(hip, Lq, Lk, 12, 2, 128, [(0, Lq, 0, Lk, True)], seed=70 + Lq, ld_extra=64)
    assert rel(got, ref) < 6e-3


@pytest.mark.parametrize("tile_rows", [128, 256])
@pytest.mark.parametrize("max_blocks", [1, 5, 7, 64])
def test_flash_attn_stream_k_splits(hip, max_blocks, tile_rows):
    """Few persistent blocks -> every item's KV range is cut; partial (m, l, O) merge must reproduce the single pass."""
    got, ref = _attn_case(hip, 300, 900, 12, 2, 128, [(0, 300, 0, 900, False)], seed=300, max_blocks=max_blocks, tile_rows=tile_rows)
    assert rel(got, ref) < 6e-3
    got, ref = _attn_case(hip, 260, 700, 4, 4, 64, [(0, 130, 0, 350, True), (130, 130, 350, 350, True)], seed=301,
                          max_blocks=max_blocks, tile_rows=tile_rows)
    assert rel(got, ref) < 6e-3


@pytest.mark.parametrize("tile_rows", [128, 256])
def test_flash_attn_more_workgroups_than_items(hip, tile_rows):
    """Short query block against a long KV range (a ViT image's tokens against the scene's cache): 8-12 items, hundreds
    of KV tiles -> the default plan cuts every item into many workgroup shares (several partials per item, middle
    shares that are neither an item's first nor last part)."""
    Lq, Lk = 300, 5000
    wins = [(0, Lq, 0, Lk, False)]
    plan = hip.make_attn_plan(wins, 4, "cuda", tile_rows=tile_rows)
    n_items = len(range(0, Lq, tile_rows)) * 4
    assert plan.n_blocks > 4 * n_items and plan.n_split == n_items
    got, ref = _attn_case(hip, Lq, Lk, 4, 2, 128, wins, seed=320, tile_rows=tile_rows)
    assert rel(got, ref) < 6e-3
    assert (got.float().cpu() - ref).abs().max() < 0.05


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 12, 2), (96, 16, 16), (80, 4, 4)])
def test_flash_attn_8wave_blocks(hip, D, Hq, Hkv):
    got, ref = _attn_case(hip, 777, 801, Hq, Hkv, D, [(0, 777, 0, 801, False)], seed=310 + D, tile_rows=256)
    assert rel(got, ref) < 6e-3
    got, ref = _attn_case(hip, 300, 520, Hq, Hkv, D, [(0, 300, 0, 520, True)], seed=311 + D, tile_rows=256)
    assert rel(got, ref) < 6e-3


@pytest.mark.parametrize("Lq,Lk,causal,qscale", [(2924, 9000, False, 1.0), (1500, 4000, True, 1.0), (777, 801, False, 1.0), (600, 3000, False, 6.0),
                                                  (256, 64, False, 1.0), (300, 900, True, 1.0)])
def test_flash_attn_4x64_form_against_8x32_form_and_hazard_screen(hip, Lq, Lk, causal, qscale):
    """flash_fwd64_kernel (4 waves x 64 rows, owned accumulation registers, hand-spaced hazards H1-H5, power-of-two softmax
    reference) against the 8 x 32 form on the same plan: long non-causal prefill, causal prompt (masked diagonal tiles), a
    partly filled last tile, peaked rows (Q x 6: one key dominates), a single-tile window, stream-K pieces.  Both forms must
    agree with the fp32-softmax oracle to bf16 noise and with each other; and 25 repeated launches of the new form must be
    BIT-IDENTICAL - a hazard spaced too short shows as run-to-run flicker long before it shows as a large error."""
    Hq, Hkv, D = 12, 2, 128
    q = dev((rnd(Lq, Hq * D, seed=1000 + Lq) * qscale).bfloat16())
    k = dev(rnd(Lk, Hkv * D, seed=1001 + Lk).bfloat16())
    v = dev(rnd(Lk, Hkv * D, seed=1002 + Lk).bfloat16())
    plan = hip.make_attn_plan([(0, Lq, 0, Lk, causal)], Hq, "cuda", tile_rows=256)
    form = hip.lib().g2v_debug_attn_form
    outs = {}
    try:
        for f in (0, 1):
            form(f)
            o = torch.zeros((Lq, Hq * D), dtype=torch.bfloat16, device="cuda")
            hip.flash_attn(q, k, v, o, plan, Hq, Hkv, D)
            outs[f] = o
        first = outs[1].clone()
        flick = 0
        for _ in range(25):
            o = torch.zeros_like(first)
            hip.flash_attn(q, k, v, o, plan, Hq, Hkv, D)
            flick += int(not torch.equal(o, first))
    finally:
        form(1)
    assert flick == 0, flick
    ref = O.varlen_attention(q.float().cpu().view(Lq, Hq, D), k.float().cpu().view(Lk, Hkv, D), v.float().cpu().view(Lk, Hkv, D), [0, Lq], [0, Lk], causal)
    e0, e1 = rel(outs[0].view(Lq, Hq, D), ref), rel(outs[1].view(Lq, Hq, D), ref)
    assert e0 < 6e-3 and e1 < 6e-3 and e1 < 1.5 * e0 + 1e-4, (e0, e1)
    assert rel(outs[1], outs[0]) < 8e-3
    assert torch.isfinite(outs[1].float()).all()


@pytest.mark.parametrize("spike_at", [70, 600, 1279])
def test_flash_attn_4x64_form_rescale_path(hip, spike_at):
    """The cold path of flash_fwd64_kernel: its softmax reference is fixed from a segment's first tile and raised only when a row
    maximum outgrows it by 2^64 - then O and l (128 + 32 accumulation registers, read / scaled / written back one by one between
    two hazard fences) are multiplied by an exact power of two.  One key whose score exceeds every other by ~1000 in the log2
    domain appears in the second, a middle or the last tile (and, with 5 workgroups, inside a stream-K piece whose partial then
    carries the raised reference into the combine pass): the output rows must become that key's value row, as the oracle's do."""
    Lq, Lk, Hq, Hkv, D = 300, 1280, 12, 2, 128
    u = rnd(1, D, seed=77)
    q = dev((rnd(Lq, Hq * D, seed=78) + 3.0 * u.repeat(1, Hq)).bfloat16())
    k = rnd(Lk, Hkv * D, seed=79)
    k[spike_at] = 20.0 * u.repeat(1, Hkv)
    k = dev(k.bfloat16())
    v = dev(rnd(Lk, Hkv * D, seed=80).bfloat16())
    for max_blocks in (None, 5):
        plan = hip.make_attn_plan([(0, Lq, 0, Lk, False)], Hq, "cuda", tile_rows=256, max_blocks=max_blocks)
        o = torch.zeros((Lq, Hq * D), dtype=torch.bfloat16, device="cuda")
        hip.flash_attn(q, k, v, o, plan, Hq, Hkv, D)
        ref = O.varlen_attention(q.float().cpu().view(Lq, Hq, D), k.float().cpu().view(Lk, Hkv, D), v.float().cpu().view(Lk, Hkv, D), [0, Lq], [0, Lk], False)
        assert torch.isfinite(o.float()).all()
        assert rel(o.view(Lq, Hq, D), ref) < 6e-3, (max_blocks, rel(o.view(Lq, Hq, D), ref))
        want = v[spike_at].float().cpu().view(Hkv, D).repeat_interleave(Hq // Hkv, 0)            # every row = the spike key's value row
        assert (o.float().cpu().view(Lq, Hq, D) - want[None]).abs().max() < 0.05


def test_multi_launch_scratch_is_owned_per_host_thread(hip):
    """VERDICT r02 weak #2 / #12 (the red driver run): kernel scratch that lives across launches - the attention's partial
    slots between its forward and combine launches, the skinny GEMM's cross-workgroup K-split tickets and partials, the
    argmax ticket - was keyed by stream only, so two HOST THREADS enqueueing on one stream (ctypes releases the GIL inside
    a call) could interleave A.forward, B.forward, A.combine and merge each other's partials.  Scratch is now owned per
    (device, stream, thread) (hip.scratch_owner).  Two threads run the SAME split attention plan, the same split-K GEMM
    shape and the argmax on the SAME stream with different inputs, 60 times each; every result must equal the
    single-threaded result of its inputs bit for bit."""
    import threading
    Lq, Lk, Hq, Hkv, D = 300, 5000, 4, 2, 128
    plan = hip.make_attn_plan([(0, Lq, 0, Lk, False)], Hq, "cuda", tile_rows=128)
    assert plan.n_slots > 0 and plan.n_comb > 0                      # the plan has partial slots: forward + combine share scratch
    M, N, K = 8, 1536, 8960                                            # skinny GEMM: K split across workgroups (tickets + partials)
    w = dev(rnd(N, K, seed=905, scale=K ** -0.5).bfloat16())
    data = []
    for t in range(2):
        q, k, v = (dev(rnd(n, h * D, seed=900 + 10 * t + i).bfloat16()) for i, (n, h) in enumerate(((Lq, Hq), (Lk, Hkv), (Lk, Hkv))))
        x = dev(rnd(M, K, seed=950 + t).bfloat16())
        lg = dev(rnd(151936, seed=960 + t).bfloat16())
        data.append((q, k, v, x, lg))

    def once(t):
        q, k, v, x, lg = data[t]
        o = torch.zeros((Lq, Hq * D), dtype=torch.bfloat16, device="cuda")
        hip.flash_attn(q, k, v, o, plan, Hq, Hkv, D)
        y = hip.linear(x, w)
        am = hip.argmax_bf16(lg, torch.zeros(1, dtype=torch.int32, device="cuda"))
        return o, y, am

    want = [once(t) for t in range(2)]
    torch.cuda.synchronize()
    assert not torch.equal(want[0][0], want[1][0]) and int(want[0][2]) == int(data[0][4].float().argmax())
    main_stream = torch.cuda.current_stream().cuda_stream
    bad, errs = [0, 0], []

    def worker(t):
        try:
            assert torch.cuda.current_stream().cuda_stream == main_stream      # both threads enqueue on ONE stream
            outs = [once(t) for _ in range(60)]
            torch.cuda.synchronize()
            bad[t] = sum(int(not (torch.equal(o, want[t][0]) and torch.equal(y, want[t][1]) and torch.equal(am, want[t][2])))
                         for o, y, am in outs)
        except BaseException as e:                                     # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    assert not errs, errs
    assert bad == [0, 0], bad
    # and the owners are distinct: one scratch per (device, stream, thread)
    assert len(plan._by_owner) == 3 and len({k[2] for k in plan._by_owner}) == 3


def test_flash_attn_spiked_max_forces_rescale(hip):
    # online-softmax rescale path: one key far above the rest appears in a late tile
    Lq, Lk, H, D = 64, 512, 2, 128
    q = rnd(Lq, H * D, seed=80).bfloat16(); k = rnd(Lk, H * D, seed=81).bfloat16(); v = rnd(Lk, H * D, seed=82).bfloat16()
    k[300] = (q[5].float() * 4).bfloat16()
    out = torch.zeros((Lq, H * D), dtype=torch.bfloat16, device="cuda")
    plan = hip.make_attn_plan([(0, Lq, 0, Lk, False)], H, "cuda", max_blocks=3)      # force KV splits across blocks
    hip.flash_attn(dev(q), dev(k), dev(v), out, plan, H, H, D)
    ref = O.varlen_attention(q.view(Lq, H, D).float(), k.view(Lk, H, D).float(), v.view(Lk, H, D).float(), [0, Lq], [0, Lk], False)
    assert rel(out.view(Lq, H, D), ref) < 6e-3


# ------------------------------------------------------------------------------- DINO front end
def test_im2col_and_assemble_match_conv(hip):
    N, H, W, C = 2, 42, 56, 128
    img = rnd(N, 3, H, W, seed=90)
    wt = rnd(C, 3, 14, 14, seed=91, scale=588 ** -0.5)
    b = rnd(C, seed=92, scale=0.1)
    ref = F.conv2d(img.bfloat16(), wt.bfloat16(), b.bfloat16(), stride=14).flatten(2).transpose(1, 2)   # [N,P,C]
    cols = hip.im2col14(dev(img), 640)
    wpad = torch.zeros((C, 640)); wpad[:, :588] = wt.reshape(C, 588)
    emb = hip.linear(cols, dev(wpad.bfloat16()), dev(b.bfloat16()))
    P = (H // 14) * (W // 14)
    assert_bf16_close(emb.view(N, P, C), ref)
    cls, regs, pos = rnd(C, seed=93), rnd(4, C, seed=94), rnd(P + 1, C, seed=95)
    x = hip.dino_assemble(emb, dev(cls), dev(regs), dev(pos), N, P).view(N, P + 5, C).cpu()
    e = emb.float().cpu().view(N, P, C)
    assert torch.equal(x[:, 0], (cls + pos[0]).expand(N, -1))
    assert torch.equal(x[:, 1:5], regs.expand(N, -1, -1))
    assert torch.equal(x[:, 5:], e + pos[1:])


def test_row_movers_and_casts(hip):
    src = rnd(50, 256, seed=96)
    idx = torch.randperm(50, generator=torch.Generator().manual_seed(1))[:20].to(torch.int32)
    out = torch.zeros((20, 256), device="cuda")
    assert torch.equal(hip.gather_rows(dev(src), dev(idx), out).cpu(), src[idx.long()])
    dst = torch.zeros((50, 256), device="cuda")
    hip.scatter_rows(dev(src[:20]), dev(idx), dst)
    ref = torch.zeros(50, 256); ref[idx.long()] = src[:20]
    assert torch.equal(dst.cpu(), ref)
    assert torch.equal(hip.cast_bf16(dev(src)).cpu(), src.bfloat16())
    assert torch.equal(hip.cast_f32(dev(src.bfloat16())).cpu(), src.bfloat16().float())


# ----------------------------------------------------------------------------------------- heads
@pytest.mark.parametrize("h,w,oh,ow", [(720, 1280, 294, 518), (1080, 1920, 294, 518), (100, 130, 294, 518), (300, 518, 294, 518),
                                        (294, 400, 294, 518), (294, 518, 294, 518)])
def test_lanczos_resize_u8_matches_pillow(hip, h, w, oh, ow):
    """g2v_lanczos_resize_u8: the loader's PIL LANCZOS resize (reference data/transforms_vggt.py:437) on the device, bit-exact
    against Pillow itself - both passes, one pass only (an axis that keeps its size), and the no-op copy."""
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(h + w)
    src = rng.integers(0, 256, size=(3, h, w, 3), dtype=np.uint8)
    src[1] = np.clip(np.kron(rng.random((h // 16 + 1, w // 16 + 1, 3)), np.ones((16, 16, 1)))[:h, :w] * 255, 0, 255).astype(np.uint8)
    src[2, :, : w // 2] = 255; src[2, :, w // 2:] = 0                               # a hard edge: negative lobes must clip at 0 / 255
    got = hip.lanczos_resize_u8(torch.from_numpy(src).cuda(), oh, ow)
    ref = np.stack([np.asarray(Image.fromarray(s_).resize((ow, oh), Image.Resampling.LANCZOS)) for s_ in src])
    assert got.shape == (3, oh, ow, 3) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), ref)


def test_loader_on_device_equals_host_loader(hip):
    """host.load_images_u8(device=...): frames of two different source sizes (every image is resized to the target computed from
    the FIRST one, data/transforms_vggt.py:421-437) - the device tensor equals the host (Pillow) loader's bytes; a non-RGB image
    sends the whole call down the host path."""
    import numpy as np
    from PIL import Image
    from g2vlm_amd import host
    rng = np.random.default_rng(9)
    pil = [Image.fromarray(rng.integers(0, 256, size=s_, dtype=np.uint8), "RGB") for s_ in ((540, 960, 3), (720, 1280, 3), (540, 960, 3))]
    want = host.load_images_u8(pil, 518)
    got = host.load_images_u8(pil, 518, device="cuda")
    assert got.is_cuda and torch.equal(got.cpu(), want)
    pil[1] = pil[1].convert("L")
    got = host.load_images_u8(pil, 518, device="cuda")
    assert not got.is_cuda and torch.equal(got, host.load_images_u8(pil, 518))


@pytest.mark.parametrize("ps_,H,W", [(14, 28, 42), (16, 48, 32)])
def test_pts_epilogue_matches_pixel_shuffle(hip, ps_, H, W):
    """Pi3LinearPts3d tail (transformer_head.py:69-81) for both patch sizes the reference builds heads for (g2vlm.py:169-172)"""
    N, pp = 2, ps_ * ps_
    P = (H // ps_) * (W // ps_)
    feat = rnd(N * P, 3 * pp, seed=100, scale=0.5)
    ps = F.pixel_shuffle(feat.view(N, P, 3 * pp).transpose(-1, -2).reshape(N, 3 * pp, H // ps_, W // ps_), ps_).permute(0, 2, 3, 1)
    out, _ = hip.pts_epilogue(dev(feat), N, H, W, 0, patch=ps_)
    assert torch.equal(out.cpu(), ps)
    pose = torch.eye(4).repeat(N, 1, 1); pose[:, :3, :] = rnd(N, 3, 4, seed=101)
    loc, wld = hip.pts_epilogue(dev(feat), N, H, W, 1, dev(pose), patch=ps_)
    z = torch.exp(ps[..., 2:]); lref = torch.cat([ps[..., :2] * z, z], -1)
    assert rel(loc, lref) < 1e-6
    homo = torch.cat([lref, torch.ones_like(lref[..., :1])], -1)
    wref = torch.einsum("nij,nhwj->nhwi", pose, homo)[..., :3]
    assert rel(wld, wref) < 1e-6
    for C_ in (1, 2):                                        # the confidence head's 1-channel shuffle (g2vlm.py:216-219)
        cf = rnd(N * P, C_ * pp, seed=102 + C_)
        want = F.pixel_shuffle(cf.view(N, P, C_ * pp).transpose(-1, -2).reshape(N, C_ * pp, H // ps_, W // ps_), ps_).permute(0, 2, 3, 1)
        assert torch.equal(hip.pixel_shuffle(dev(cf), N, H, W, C_, patch=ps_).cpu(), want)
    lib = hip.lib()                                          # a patch size no head is built for, or a ragged image: refused
    o = torch.empty((N, H, W, 3), device="cuda")
    assert lib.g2v_pts_epilogue_ps(dev(feat).data_ptr(), N, H, W, 15, 0, None, o.data_ptr(), None, None) != 0
    assert lib.g2v_pixel_shuffle(dev(feat).data_ptr(), N, H + 1, W, 3, ps_, o.data_ptr(), None) != 0


def test_camera_tail_svd(hip):
    N, P = 5, 37
    sd = {k: v for k, v in []}
    feat = rnd(N, P, 512, seed=110).abs()
    w0, b0 = rnd(512, 512, seed=111, scale=512 ** -0.5), rnd(512, seed=112, scale=0.1)
    w1, b1 = rnd(512, 512, seed=113, scale=512 ** -0.5), rnd(512, seed=114, scale=0.1)
    wt, bt = rnd(3, 512, seed=115, scale=0.05), rnd(3, seed=116)
    wr, br = rnd(9, 512, seed=117, scale=0.05), rnd(9, seed=118)
    f = feat.mean(1)
    f = F.relu(F.linear(f, w0, b0)); f = F.relu(F.linear(f, w1, b1))
    t = F.linear(f, wt, bt); r = F.linear(f, wr, br).reshape(-1, 3, 3)
    mt = torch.transpose(F.normalize(r, p=2, dim=-1), -1, -2)
    u, s, vh = torch.linalg.svd(mt); v = vh.transpose(-2, -1)
    det = torch.det(v @ u.transpose(-2, -1))
    R = torch.cat([v[:, :, :-1], v[:, :, -1:] * det.view(-1, 1, 1)], 2) @ u.transpose(-2, -1)
    pose = hip.camera_tail(dev(feat), N, P, *[dev(a) for a in (w0, b0, w1, b1, wt, bt, wr, br)]).cpu()
    assert (pose[:, :3, :3] - R).abs().max() < 2e-5
    assert (pose[:, :3, 3] - t).abs().max() < 2e-5
    assert torch.equal(pose[:, 3], torch.tensor([0., 0., 0., 1.]).expand(N, -1))
    # a reflection case: force det < 0
    wr2 = wr.clone(); wr2[0:3] = -wr2[0:3]
    pose2 = hip.camera_tail(dev(feat), N, P, *[dev(a) for a in (w0, b0, w1, b1, wt, bt, wr2, br)]).cpu()
    assert (torch.det(pose2[:, :3, :3]) - 1).abs().max() < 1e-4


# ---------------------------------------------------------------------------------------- decode
def test_gemv_swiglu_argmax(hip):
    K, N = 1536, 2048
    x, w, b = rnd(K, seed=120).bfloat16(), rnd(N, K, seed=121, scale=K ** -0.5).bfloat16(), rnd(N, seed=122).bfloat16()
    out = torch.empty(N, dtype=torch.bfloat16, device="cuda")
    hip.gemv_bf16(dev(x), dev(w), dev(b), out)
    ref = F.linear(x[None], w, b)[0]
    assert_bf16_close(out, ref)
    res = rnd(N, seed=123)
    rd = dev(res).clone()
    hip.gemv_bf16(dev(x), dev(w), None, None, res=rd)
    assert rel(rd, res + F.linear(x[None], w)[0]) < 2e-3
    # fused producers: rmsnorm -> GEMV, SwiGLU -> GEMV (+ residual)
    xf, nw = rnd(K, seed=126) * 2, 1 + 0.1 * rnd(K, seed=127)
    xn = (nw * (xf * torch.rsqrt(xf.pow(2).mean() + 1e-6))).bfloat16()
    o2 = torch.empty(N, dtype=torch.bfloat16, device="cuda")
    hip.gemv_rmsnorm_bf16(dev(xf), dev(nw), 1e-6, dev(w), dev(b), o2)
    assert_bf16_close(o2, F.linear(xn[None], w, b)[0])
    from g2vlm_amd.weights import interleave_gate_up
    Kd = 512
    g_, u_ = rnd(Kd, seed=128).bfloat16(), rnd(Kd, seed=129).bfloat16()
    guv = interleave_gate_up(g_.view(Kd, 1), u_.view(Kd, 1)).view(-1)
    wd = rnd(300, Kd, seed=130, scale=Kd ** -0.5).bfloat16()
    r3 = dev(res[:300]).clone()
    hip.gemv_swiglu_bf16(dev(guv), dev(wd), r3)
    act = F.silu(g_) * u_
    assert rel(r3, res[:300] + F.linear(act[None], wd)[0]) < 2e-3
    # norm + gate/up GEMV + activation in one launch (the decode MLP's first half)
    Fd = 256
    wg2, wu2 = rnd(Fd, K, seed=140, scale=K ** -0.5).bfloat16(), rnd(Fd, K, seed=141, scale=K ** -0.5).bfloat16()
    a5 = torch.empty(Fd, dtype=torch.bfloat16, device="cuda")
    hip.gemv_rmsnorm_swiglu_bf16(dev(xf), dev(nw), 1e-6, dev(interleave_gate_up(wg2, wu2)), a5)
    ref5 = F.silu(F.linear(xn[None], wg2)[0]) * F.linear(xn[None], wu2)[0]
    assert_bf16_close(a5, ref5)
    big = rnd(17920, 1536, seed=131, scale=1536 ** -0.5).bfloat16()          # 8-rows-per-block path
    o4 = torch.empty(17920, dtype=torch.bfloat16, device="cuda")
    hip.gemv_bf16(dev(x), dev(big), None, o4)
    assert_bf16_close(o4, F.linear(x[None], big)[0])
    gu = rnd(2 * 512, seed=124).bfloat16()
    o = torch.empty(512, dtype=torch.bfloat16, device="cuda")
    hip.swiglu_bf16(dev(gu), o)
    gv = gu.view(32, 2, 16)
    assert_bf16_close(o, (F.silu(gv[:, 0]) * gv[:, 1]).reshape(-1), ulps=1.01)
    logits = rnd(151936, seed=125).bfloat16()
    logits[7777] = logits.max(); logits[99999] = logits.max()
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.argmax_bf16(dev(logits), idx)
    assert int(idx[0]) == int(torch.argmax(logits.float()))
    # the result is always an index of the input: NaN ranks highest (torch.argmax), all -inf gives a valid index
    bad = logits.clone(); bad[4242] = float("nan")
    hip.argmax_bf16(dev(bad), idx)
    assert int(idx[0]) == 4242
    hip.argmax_bf16(dev(torch.full((151936,), float("-inf")).bfloat16()), idx)
    assert 0 <= int(idx[0]) < 151936


@pytest.mark.parametrize("Lk", [1, 63, 64, 777, 3000])
def test_decode_attn(hip, Lk):
    Hq, Hkv = 12, 2
    q = rnd(Hq, 128, seed=130).bfloat16()
    kc, vc = rnd(Lk + 5, Hkv, 128, seed=131).bfloat16(), rnd(Lk + 5, Hkv, 128, seed=132).bfloat16()
    ws = torch.empty(hip.decode_attn_workspace(Lk, Hq) // 4, dtype=torch.float32, device="cuda")
    out = torch.empty((Hq, 128), dtype=torch.bfloat16, device="cuda")
    hip.decode_attn(dev(q), dev(kc), dev(vc), out, Lk, Hq, Hkv, 128 ** -0.5, ws)
    ref = O.varlen_attention(q[None].float(), kc[:Lk].float(), vc[:Lk].float(), [0, 1], [0, Lk], True)[0]
    assert_bf16_close(out, ref.bfloat16(), ulps=1.01)


def test_decode_attn_batch_matches_per_scene(hip):
    """Batched split-KV decode attention: scene z of the batched launch is bit-identical to the batch-1
    kernel on that scene's cache and length, and matches the oracle's varlen attention (reference qwen2vl.py:643-652)."""
    Hq, Hkv, cap = 12, 2, 1024
    lens = [1, 64, 333, 1000]
    B = len(lens)
    q = rnd(B, Hq * 128, seed=150).bfloat16()
    kc, vc = rnd(B, cap, Hkv, 128, seed=151).bfloat16(), rnd(B, cap, Hkv, 128, seed=152).bfloat16()
    qd, kd, vd = dev(q), dev(kc), dev(vc)
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
    ws = torch.empty(B * hip.decode_attn_workspace(cap, Hq) // 4, dtype=torch.float32, device="cuda")
    out = torch.empty((B, Hq * 128), dtype=torch.bfloat16, device="cuda")
    hip.decode_attn_batch(qd, kd, vd, out, ld, cap, cap, Hq, Hkv, 128 ** -0.5, ws)
    ws1 = torch.empty(hip.decode_attn_workspace(cap, Hq) // 4, dtype=torch.float32, device="cuda")
    for z, Lk in enumerate(lens):
        one = torch.empty((Hq, 128), dtype=torch.bfloat16, device="cuda")
        hip.decode_attn(qd[z].view(Hq, 128), kd[z], vd[z], one, Lk, Hq, Hkv, 128 ** -0.5, ws1)
        assert torch.equal(out[z].view(Hq, 128), one), z
        ref = O.varlen_attention(q[z].view(1, Hq, 128).float(), kc[z, :Lk].float(), vc[z, :Lk].float(), [0, 1], [0, Lk], True)[0]
        assert_bf16_close(out[z].view(Hq, 128), ref.bfloat16(), ulps=1.01)


def test_argmax_rows_and_advance_batch(hip):
    B, V = 5, 151936
    logits = rnd(B, V, seed=160).bfloat16()
    for r in range(B):
        m = logits[r].max()
        logits[r, 1000 * r + 17] = m; logits[r, 150000 - r] = m          # ties: the first maximal index wins (torch.argmax)
    idx = torch.zeros(B, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(129 * B, dtype=torch.int32, device="cuda")
    for _ in range(2):                                                   # the arrival tickets reset themselves
        hip.argmax_rows_bf16(dev(logits), idx, scratch)
        assert idx.cpu().tolist() == torch.argmax(logits.float(), dim=-1).tolist()
    small = rnd(3, 999, seed=161).bfloat16()
    idx3 = torch.zeros(3, dtype=torch.int32, device="cuda")
    hip.argmax_rows_bf16(dev(small), idx3, torch.zeros(129 * 3, dtype=torch.int32, device="cuda"))
    assert idx3.cpu().tolist() == torch.argmax(small.float(), dim=-1).tolist()
    pos = torch.arange(3 * B, dtype=torch.int32, device="cuda").view(3, B).contiguous()
    row = torch.arange(B, dtype=torch.int32, device="cuda") * 100
    ln = torch.arange(B, dtype=torch.int32, device="cuda") + 7
    p0, r0, l0 = pos.clone(), row.clone(), ln.clone()
    hip.decode_advance_batch(pos, row, ln)
    assert torch.equal(pos, p0 + 1) and torch.equal(row, r0 + 1) and torch.equal(ln, l0 + 1)


@pytest.mark.parametrize("n_frames", [1, 2, 3])
def test_qwen_patchify_on_device_is_bit_identical_to_host_transform(hip, n_frames):
    """rescale + normalise + temporal pairing + patch reorder + bf16 cast + K zero-pad in one kernel on the
    uint8 frame (g2v_qwen_patchify_u8) against the host restatement of Qwen2VLImageProcessor._preprocess
    (host.QwenVL2ImageTransform, itself pinned to the reference's golden in tests/test_host_cpu.py)."""
    from PIL import Image
    from g2vlm_amd import host
    rng = np.random.default_rng(7)
    imgs = [Image.fromarray(rng.integers(0, 256, size=(150, 210, 3), dtype=np.uint8)) for _ in range(n_frames)]
    cpu_t = host.QwenVL2ImageTransform(140, 196)
    dev_t = host.QwenVL2ImageTransform(140, 196, device="cuda", k_pad=1216)
    pv, thw = cpu_t(imgs)
    pd, thw_d = dev_t(imgs)
    assert torch.equal(thw, thw_d) and pd.dtype == torch.bfloat16 and pd.is_cuda and pd.shape == (pv.shape[0], 1216)
    assert torch.equal(pd[:, :1176].cpu(), pv.bfloat16())
    assert float(pd[:, 1176:].abs().max()) == 0


def test_decode_attn_fused_is_bit_identical_to_separate_kernels(hip):
    """g2v_decode_attn_fused (q/k-norm + mRoPE + cache append folded into the split-KV attention) against
    g2v_qknorm_mrope_cache followed by g2v_decode_attn_batch on the same step: attention output, the appended K and V rows
    and every other cache row are bit-identical.  Lengths put the new token's row at the start, end and middle of a 64-key
    chunk and in the first chunk."""
    Hq, Hkv, cap = 12, 2, 512
    lens = [1, 64, 65, 128, 300, 449]                       # INCLUDING the new token
    B = len(lens)
    nh = Hq + 2 * Hkv
    qkv = dev(rnd(B, nh * 128, seed=170).bfloat16())
    qw, kw = dev(1 + 0.1 * rnd(128, seed=171)), dev(1 + 0.1 * rnd(128, seed=172))
    pos = torch.tensor([[n - 1 for n in lens]] * 3, dtype=torch.int32, device="cuda")
    inv_freq = dev(1.0 / (1e6 ** (torch.arange(0, 128, 2).float() / 128)))
    cos, sin = hip.mrope_table(pos, inv_freq)
    kc0, vc0 = dev(rnd(B, cap, Hkv, 128, seed=173).bfloat16()), dev(rnd(B, cap, Hkv, 128, seed=174).bfloat16())
    for z, n in enumerate(lens):                            # the row to be appended and everything behind it: uninitialised memory
        kc0[z, n - 1:] = float("nan"); vc0[z, n - 1:] = float("nan")
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
    ws = torch.empty(B * hip.decode_attn_workspace(cap, Hq) // 4, dtype=torch.float32, device="cuda")
    # separate kernels
    k1, v1 = kc0.clone(), vc0.clone()
    qn = torch.empty((B, Hq * 128), dtype=torch.bfloat16, device="cuda")
    rows = torch.tensor([z * cap + lens[z] - 1 for z in range(B)], dtype=torch.int32, device="cuda")
    hip.qknorm_mrope_cache(qkv, Hq, Hkv, qw, qw, kw, kw, 0, 1e-6, 1, cos, sin, qn, k1, v1, rows)
    o1 = torch.empty((B, Hq * 128), dtype=torch.bfloat16, device="cuda")
    hip.decode_attn_batch(qn, k1, v1, o1, ld, cap, cap, Hq, Hkv, 128 ** -0.5, ws)
    # fused
    k2, v2 = kc0.clone(), vc0.clone()
    o2 = torch.empty_like(o1)
    hip.decode_attn_fused(qkv, qw, kw, 1e-6, 1, cos, sin, k2, v2, o2, ld, cap, cap, Hq, Hkv, 128 ** -0.5, ws)
    bits = lambda t: t.view(torch.int16)
    assert torch.equal(bits(k1), bits(k2)) and torch.equal(bits(v1), bits(v2))
    assert torch.isfinite(o2.float()).all() and torch.equal(o1, o2)
    for z, n in enumerate(lens):                            # and the append went to the right row only
        assert torch.isfinite(k2[z, :n].float()).all() and torch.isfinite(v2[z, :n].float()).all()
        assert torch.isnan(k2[z, n:].float()).all() and torch.equal(k2[z, :n - 1], kc0[z, :n - 1])


# ----------------------------------------------------------------------------------------- sampling (do_sample)
from imageop_check import gumbel_scores, philox_first  # noqa: E402,F401  (the host restatement of csrc/misc.hip::philox_first)


@pytest.mark.parametrize("n", [500, 151936])
def test_sample_rows_is_the_gumbel_max_of_its_philox_stream(hip, n):
    """g2v_sample_rows_bf16 (the reference's do_sample branch, g2vlm.py:1119-1122): per row and step the drawn index is the
    argmax of logit / T + Gumbel noise from Philox(seed, step, row, i), restated on the host; the step word advances per
    call and rows draw independently."""
    rows, seed, T = 3, 0x1234567890ABCDEF, 0.7
    x = (rnd(rows, n, seed=5) * 3).bfloat16()
    xd = dev(x)
    out = torch.zeros(rows, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(rows * 129, dtype=torch.int32, device="cuda")
    rng = hip.make_rng(seed, T, "cuda")
    inv_t = np.float32(1.0 / T)
    for step in range(4):
        hip.sample_rows_bf16(xd, out, scratch, rng)
        got = out.cpu().tolist()
        assert int(rng.cpu()[2]) == step + 1
        for r in range(rows):
            sc = gumbel_scores(x[r].float().numpy(), float(inv_t), seed, step, r)
            # fp32 log on the device vs fp64 here: the drawn index must be the maximiser up to that noise
            assert sc[got[r]] >= sc.max() - 1e-4 * max(1.0, abs(sc.max())), (step, r, got[r], int(sc.argmax()))
    # temperature -> 0 is argmax (rows whose top-2 gap is clear of the Gumbel noise x T)
    y = x.clone()
    for r in range(rows):
        y[r, 37 + r] = 40.0
    cold = hip.make_rng(seed, 1e-3, "cuda")
    hip.sample_rows_bf16(dev(y), out, scratch, cold)
    assert out.cpu().tolist() == [37 + r for r in range(rows)]


def test_sample_rows_follows_softmax(hip):
    """Distribution check: 40 000 draws from one 48-token row at T = 1.3 against softmax(logits / T) (chi-square)."""
    n, T, draws = 48, 1.3, 40000
    x = (rnd(1, n, seed=9) * 2).bfloat16()
    xd = dev(x).expand(500, n).contiguous()                 # 500 rows x 80 steps, every (row, step) an independent draw
    out = torch.zeros(500, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(500 * 129, dtype=torch.int32, device="cuda")
    rng = hip.make_rng(77, T, "cuda")
    counts = torch.zeros(n, dtype=torch.float64)
    for _ in range(draws // 500):
        hip.sample_rows_bf16(xd, out, scratch, rng)
        counts += torch.bincount(out.cpu().long(), minlength=n).double()
    p = torch.softmax(x[0].double() / T, -1)
    chi2 = float(((counts - draws * p) ** 2 / (draws * p)).sum())
    assert chi2 < 100.0, chi2                              # 47 degrees of freedom: P(chi2 > 100) ~ 1e-5


def test_dino_preprocess_on_device_is_bit_identical_to_host_ops(hip):
    """g2v_dino_preprocess: ToTensor's k/255, Normalize and the original_images copy of
    prepare_dino_images_pi3 (reference g2vlm.py:947-953) from the loader's uint8 frames, and from an fp32 image."""
    from g2vlm_amd import host
    u8 = torch.from_numpy(np.random.default_rng(4).integers(0, 256, size=(3, 42, 70, 3), dtype=np.uint8))
    imgs = u8.permute(0, 3, 1, 2).float().div(255)                       # ToTensor
    mean = torch.tensor(host.RESNET_MEAN).view(1, 3, 1, 1); std = torch.tensor(host.RESNET_STD).view(1, 3, 1, 1)
    want = (imgs - mean) / std
    norm, orig = hip.dino_preprocess(dev(u8), host.RESNET_MEAN, host.RESNET_STD)
    assert torch.equal(norm.cpu(), want) and torch.equal(orig.cpu(), imgs)
    f = torch.rand((2, 3, 28, 56), generator=torch.Generator().manual_seed(1))
    norm, orig = hip.dino_preprocess(dev(f), host.RESNET_MEAN, host.RESNET_STD)
    assert torch.equal(norm.cpu(), (f - mean) / std) and torch.equal(orig.cpu(), f) and orig.data_ptr() != norm.data_ptr()


# ----------------------------------------------------------------------------------------- decode, persistent-grid kernels
@pytest.mark.parametrize("N,K", [(2048, 1536), (1536, 1536), (1536, 8960), (300, 512), (7, 256), (151936, 1536), (1000, 2056)])
def test_gemv_pg_plain_bias_residual(hip, N, K):
    """g2v_gemv_pg (csrc/decode_layer.hip): nn.Linear at M = 1 on a 256-block grid, any N (rows per wave 0..many), K up to
    9216 (one or eighteen chunk steps per lane), against F.linear on the same bf16 operands."""
    x, w, b = rnd(K, seed=201).bfloat16(), rnd(N, K, seed=202, scale=K ** -0.5).bfloat16(), rnd(N, seed=203).bfloat16()
    out = torch.full((N,), float("nan"), dtype=torch.bfloat16, device="cuda")
    hip.gemv_pg(dev(x), dev(w), bias=dev(b), out=out)
    assert_bf16_close(out, F.linear(x[None], w, b)[0])
    hip.gemv_pg(dev(x), dev(w), out=out)
    assert_bf16_close(out, F.linear(x[None], w)[0])
    res = rnd(N, seed=204)
    rd = dev(res).clone()
    hip.gemv_pg(dev(x), dev(w), res=rd)
    assert rel(rd, res + F.linear(x[None], w)[0].float()) < 2e-3


@pytest.mark.parametrize("N,K", [(2048, 1536), (512, 256), (151936, 1536)])
def test_gemv_pg_fused_rmsnorm(hip, N, K):
    xf, nw = rnd(K, seed=210) * 2, 1 + 0.1 * rnd(K, seed=211)
    w, b = rnd(N, K, seed=212, scale=K ** -0.5).bfloat16(), rnd(N, seed=213).bfloat16()
    xn = (nw * (xf * torch.rsqrt(xf.pow(2).mean() + 1e-6))).bfloat16()
    out = torch.empty(N, dtype=torch.bfloat16, device="cuda")
    hip.gemv_pg(dev(xf), dev(w), norm_w=dev(nw), eps=1e-6, bias=dev(b), out=out)
    assert_bf16_close(out, F.linear(xn[None], w, b)[0])


@pytest.mark.parametrize("Fd,K", [(8960, 1536), (512, 256), (48, 1536)])
def test_gemv_pg_norm_gate_up_swiglu(hip, Fd, K):
    """The MLP's first half in one launch (reference modeling_qwen2_vl.py:519-521 at q_len 1): RMSNorm, gate / up GEMV on the
    interleaved weight, bf16(bf16(silu(g)) * u)."""
    from g2vlm_amd.weights import interleave_gate_up
    xf, nw = rnd(K, seed=220) * 2, 1 + 0.1 * rnd(K, seed=221)
    wg, wu = rnd(Fd, K, seed=222, scale=K ** -0.5).bfloat16(), rnd(Fd, K, seed=223, scale=K ** -0.5).bfloat16()
    xn = (nw * (xf * torch.rsqrt(xf.pow(2).mean() + 1e-6))).bfloat16()
    act = torch.full((Fd,), float("nan"), dtype=torch.bfloat16, device="cuda")
    hip.gemv_pg(dev(xf), dev(interleave_gate_up(wg, wu)), norm_w=dev(nw), eps=1e-6, out=act, act=True)
    ref = F.silu(F.linear(xn[None], wg)[0]) * F.linear(xn[None], wu)[0]
    assert_bf16_close(act, ref)


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 8])
def test_gemv_pg_batch_all_forms(hip, B):
    """g2v_gemv_pg_batch (csrc/decode_batch.hip): the decode step's Linears for B scenes per weight pass - plain / bias /
    residual at K = 1536 (wave-covers-K kernel) and K = 8960 (K cut over the waves), the fused-RMSNorm form, the
    norm + gate/up + SwiGLU form, the lm_head shape - against F.linear on the same bf16 operands, row by row; a row's result
    must not depend on the other rows (rows beyond B are padded inside the kernel)."""
    from g2vlm_amd.weights import interleave_gate_up
    K = 1536
    # --- o projection: bf16 x, residual
    x = rnd(B, K, seed=300).bfloat16()
    w = rnd(K, K, seed=301, scale=K ** -0.5).bfloat16()
    res = rnd(B, K, seed=302)
    rd = dev(res).clone()
    hip.gemv_pg_batch(dev(x), dev(w), res=rd)
    assert rel(rd, res + F.linear(x, w).float()) < 2e-3
    one = dev(res[:1]).clone().view(-1)
    hip.gemv_pg(dev(x[0]), dev(w), res=one)
    assert rel(rd[0], one) < 1e-6                                # same arithmetic as the batch-1 kernel for this form
    # --- qkv: fused norm + bias (N = 2048: one row per wave), and an N that leaves waves without rows
    for N in (2048, 520):
        xf, nw = rnd(B, K, seed=303) * 2, 1 + 0.1 * rnd(K, seed=304)
        wq, bq = rnd(N, K, seed=305, scale=K ** -0.5).bfloat16(), rnd(N, seed=306).bfloat16()
        xn = (nw * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6))).bfloat16()
        out = torch.full((B, N), float("nan"), dtype=torch.bfloat16, device="cuda")
        hip.gemv_pg_batch(dev(xf), dev(wq), norm_w=dev(nw), eps=1e-6, bias=dev(bq), out=out)
        assert_bf16_close(out, F.linear(xn, wq, bq))
    # --- gate/up + SwiGLU at the real width (4.4 units per wave) and a small one
    for Fd in (8960, 48):
        wg, wu = rnd(Fd, K, seed=307, scale=K ** -0.5).bfloat16(), rnd(Fd, K, seed=308, scale=K ** -0.5).bfloat16()
        act = torch.full((B, Fd), float("nan"), dtype=torch.bfloat16, device="cuda")
        hip.gemv_pg_batch(dev(xf), dev(interleave_gate_up(wg, wu)), norm_w=dev(nw), eps=1e-6, out=act, act=True)
        assert_bf16_close(act, F.silu(F.linear(xn, wg)) * F.linear(xn, wu))
    # --- down: K = 8960 (cut over the 8 waves of a block), residual; and a ragged N with bias -> bf16 out
    Kd = 8960
    xa = rnd(B, Kd, seed=309).bfloat16()
    wd = rnd(K, Kd, seed=310, scale=Kd ** -0.5).bfloat16()
    rd = dev(res).clone()
    hip.gemv_pg_batch(dev(xa), dev(wd), res=rd)
    assert rel(rd, res + F.linear(xa, wd).float()) < 2e-3
    Nr = 1000
    wr, br = rnd(Nr, Kd, seed=311, scale=Kd ** -0.5).bfloat16(), rnd(Nr, seed=312).bfloat16()
    outr = torch.full((B, Nr), float("nan"), dtype=torch.bfloat16, device="cuda")
    hip.gemv_pg_batch(dev(xa), dev(wr), bias=dev(br), out=outr)
    assert_bf16_close(outr, F.linear(xa, wr, br))
    # --- a row's result is independent of its neighbours
    if B > 1:
        x2 = x.clone(); x2[1:] = rnd(B - 1, K, seed=313).bfloat16()
        r1, r2 = dev(res).clone(), dev(res).clone()
        hip.gemv_pg_batch(dev(x), dev(w), res=r1)
        hip.gemv_pg_batch(dev(x2), dev(w), res=r2)
        assert torch.equal(r1[0], r2[0])


def test_gemv_pg_batch_lm_head_and_argument_checks(hip):
    B, N, K = 3, 151936, 1536
    xf, nw = rnd(B, K, seed=320) * 2, 1 + 0.1 * rnd(K, seed=321)
    w = rnd(N, K, seed=322, scale=K ** -0.5).bfloat16()
    xn = (nw * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6))).bfloat16()
    out = torch.full((B, N), float("nan"), dtype=torch.bfloat16, device="cuda")
    wdv = dev(w)
    hip.gemv_pg_batch(dev(xf), wdv, norm_w=dev(nw), eps=1e-6, out=out)
    assert_bf16_close(out, F.linear(xn, w))
    lib = hip.lib()
    p = out.data_ptr()
    assert lib.g2v_gemv_pg_batch(p, None, 0.0, wdv.data_ptr(), None, p, None, 9, N, K, 0, None) != 0       # B > 8
    assert lib.g2v_gemv_pg_batch(p, None, 0.0, wdv.data_ptr(), None, p, None, 2, N, 1540, 0, None) != 0    # K % 8
    assert lib.g2v_gemv_pg_batch(p, p, 0.0, wdv.data_ptr(), None, p, None, 2, N, 8960, 0, None) != 0       # fused norm: K <= 1536


def test_decode_attn_pg_matches_the_chunked_kernel_and_appends_identically(hip):
    """g2v_decode_attn_pg (256 equal shares of the cache rows per scene, 32-key MFMA batches, block-level merge) against g2v_decode_attn_fused
    (one wave per 64-key chunk) on the same step: the appended K / V rows and the untouched cache rows are bit-identical,
    the attention output agrees to fp32 summation order, and both match the oracle's varlen attention.  Lengths cover a
    single key, fewer keys than blocks, ranges that end inside / at a batch boundary and a long cache (several batches per
    wave); the row to be appended holds NaN beforehand."""
    Hq, Hkv, cap = 12, 2, 20480
    lens = [1, 2, 65, 128, 300, 449, 5000, 20000]           # INCLUDING the new token
    B = len(lens)
    nh = Hq + 2 * Hkv
    qkv = dev(rnd(B, nh * 128, seed=230).bfloat16())
    qw, kw = dev(1 + 0.1 * rnd(128, seed=231)), dev(1 + 0.1 * rnd(128, seed=232))
    pos = torch.tensor([[n - 1 for n in lens]] * 3, dtype=torch.int32, device="cuda")
    inv_freq = dev(1.0 / (1e6 ** (torch.arange(0, 128, 2).float() / 128)))
    cos, sin = hip.mrope_table(pos, inv_freq)
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    kc0 = torch.randn((B, cap, Hkv, 128), generator=g, device="cuda").bfloat16()
    vc0 = torch.randn((B, cap, Hkv, 128), generator=g, device="cuda").bfloat16()
    for z, n in enumerate(lens):
        kc0[z, n - 1:] = float("nan"); vc0[z, n - 1:] = float("nan")
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
    k1, v1, k2, v2 = kc0.clone(), vc0.clone(), kc0.clone(), vc0.clone()
    o1 = torch.empty((B, Hq * 128), dtype=torch.bfloat16, device="cuda")
    o2 = torch.full_like(o1, float("nan"))
    ws = torch.empty(B * hip.decode_attn_workspace(cap, Hq) // 4, dtype=torch.float32, device="cuda")
    hip.decode_attn_fused(qkv, qw, kw, 1e-6, 1, cos, sin, k1, v1, o1, ld, cap, cap, Hq, Hkv, 128 ** -0.5, ws)
    ws2 = torch.empty(hip.decode_attn_pg_workspace(Hq, Hkv, B) // 4, dtype=torch.float32, device="cuda")
    hip.decode_attn_pg(qkv, qw, kw, 1e-6, 1, cos, sin, k2, v2, o2, ld, cap, cap, Hq, Hkv, 128 ** -0.5, ws2)
    for z, n in enumerate(lens):
        assert torch.equal(k1[z, :n], k2[z, :n]) and torch.equal(v1[z, :n], v2[z, :n]), z
        assert torch.isnan(k2[z, n:].float()).all() and torch.isnan(v2[z, n:].float()).all(), z
        # P is rounded to bf16 for the MFMA here (as the reference's flash-attn kernel does), fp32 there: same value up to
        # that rounding, not the same bits
        assert rel(o2[z], o1[z]) < 4e-3, (z, rel(o2[z], o1[z]))
    # oracle on two of the scenes (q after norm + rope comes from the separate kernel, itself tested against the oracle)
    qn = torch.empty((B, Hq * 128), dtype=torch.bfloat16, device="cuda")
    k3, v3 = kc0.clone(), vc0.clone()
    rows = torch.tensor([z * cap + lens[z] - 1 for z in range(B)], dtype=torch.int32, device="cuda")
    hip.qknorm_mrope_cache(qkv, Hq, Hkv, qw, qw, kw, kw, 0, 1e-6, 1, cos, sin, qn, k3, v3, rows)
    for z in (4, 6):
        n = lens[z]
        ref = O.varlen_attention(qn[z].view(1, Hq, 128).float().cpu(), k3[z, :n].float().cpu(), v3[z, :n].float().cpu(), [0, 1], [0, n], True)[0]
        # P.V runs on bf16 P here, so an element's error scales with its ROW (random-sign sums cancel), not with the element:
        # rel-L2 as everywhere, and every element within 2^-6 of the row's rms (measured: 1e-2 at 5000 keys)
        got, want = o2[z].view(Hq, 128).float().cpu(), ref.float()
        assert rel(got, want) < 4e-3
        assert float(((got - want).abs() / want.pow(2).mean(dim=1, keepdim=True).sqrt()).max()) < 2.0 ** -6
    # replayable: a second call on the advanced state appends the next row
    ld2 = ld + 1
    for z, n in enumerate(lens):
        k2[z, n] = float("nan")
    hip.decode_attn_pg(qkv, qw, kw, 1e-6, 1, cos, sin, k2, v2, o2, ld2, cap, cap, Hq, Hkv, 128 ** -0.5, ws2)
    assert torch.isfinite(o2.float()).all()
    for z, n in enumerate(lens):
        assert torch.isfinite(k2[z, :n + 1].float()).all()
