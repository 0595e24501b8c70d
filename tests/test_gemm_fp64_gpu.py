"""GPU: every bf16 GEMM form (csrc/gemm.hip, gemm_big.hip, gemm_8p.hip, gemm_4w.hip, gemm_skinny.hip) and gemm_f32, element
by element against an fp64 reference (tests/gemm_check.py: the rule behind each bound is in its docstring).

A case passes with zero flagged elements: every bf16 Linear value must be an admissible rounding of the fp64 result
(tau = 2^-16 of |A|.|W|^T + |b|), every exact epilogue (bf16, RES_F32 in all four variants, RES_BF16) must reproduce the
IEEE fp32 emulation of one admissible value bit for bit, and every activation epilogue must stay within its ulp bound of the
fp64 function over the admissible values.  Around every output the launch leaves NaN sentinels (bf16 0x7FA5, fp32
0x7FA5A5A5) untouched: padding columns [n, ldc), rows past M and the gap rows between the two groups' C blocks.  Unread input
memory is NaN too: A columns [K, lda), A rows past the last group, the residual's [N, ldres), bias / gamma past N.  Rows of
A and rows of W (output columns) are scaled by powers of two over 2^-12 .. 2^12, so a tile-local bug shows at any magnitude.

Section 1 (test_form_*, test_skinny_*, test_two_groups_*, test_ab_loops): each form forced by its flag at its edges - the
last row tile at M - m0 in {1, HB-1, HB, HB+1, bm-1, bm} for every tile height of the 8-wave and 4-wave forms (HB = bm/2, a
wave row; the MFMA skip of gemm_8p.hip), the 64-row wave boundaries and N / K tails of the 128x128 kernel, M % 32 tails of
the big tile, the skinny kernel's m-tile switches and its cross-workgroup K split, two-group launches, lda > K, ldc > N,
ldres > N and in-place residuals; test_form_256_persistent_two_groups: two groups with more tiles than CUs.  g2v_gemm_route must report the form each case claims.
Section 2 (test_production): each production call site at its engine shape, grouping and aliasing through the default
dispatcher: the route it takes is asserted (ROUTES, table below), and five launches are bit-identical.
Section 3: gemm_f32 at the head shapes: |got - ref| <= K 2^-24 (|A|.|W|^T + |b|) + 2^-23 |ref| per element.

Routes of the production call sites (form, tile height, skinny K split S / KS) with the default G2V_GEMM_4W_MASK (ROUTES;
the route assertions are skipped when G2V_GEMM_FLAGS or G2V_GEMM_4W_MASK is set):

    call site                             rows: C3 / C2 (ViT: 1 / 8 images)   N             K           form       height      S/KS
    DINO patch embed                      N P = 10952 / 1554            1024          640         8p         192 / 128
    DINO qkv, fc1 (GELU)                  N (P+5) = 10992 / 1564        3072, 4096    1024        8p         288, 256 / 128
    DINO dense, fc2 (gamma, in place)     10992 / 1564                  1024          1024, 4096  4w         192 / 128
    dino2llm (no residual, no gamma)      10992 / 1564                  1536          1024        4w         288 / 128
    decoder qkv, cq, fc1 (GELU)           10952 / 1554                  4608, 1536, 6144  1536  8p         288 / 128 (fc1 C2: 160)
    decoder proj, cproj, fc2 (in place)   10952 / 1554                  1536          1536, 6144  4w         288 / 128
    decoder ckv                           P = 1369 / 777                3072          1536        8p / 128x128  128
    decoder out                           10952 / 1554                  1024, 512     1536        8p         192, 128 / 128
    ViT patch, qkv, fc1 (QuickGELU)       2916 / 23328                  1280, 3840, 5120  1216, 1280  8p     128, 192, 256 / 256, 288, 288
    ViT proj (RES_BF16 in place)          2916 / 23328                  1280          1280        8p         128 / 256
    ViT fc2 (RES_BF16 in place)           2916 / 23328                  1280          5120        4w         128 / 256
    ViT merger m0 (GELU), m2              729 / 5832                    5120, 1536    5120        4w, big / 4w   128, 32 / 256, 160
    MoT qkv                               geo + und = 10952+16 / 1554+4 2048          1536        8p         192 / 128
    MoT gate-up (SwiGLU)                  10952+16 / 1554+4             17920         1536        8p         288 / 288
    MoT o, down (gamma geo only, rounded) 10952+16 / 1554+4             1536          1536, 8960  4w         288 / 128
    MoT qkv, o, down, ViT-image prefill   und 731 (geo empty)           2048, 1536    1536, 8960  big        32
    MoT gate-up, ViT-image prefill        und 731                       17920         1536        8p         256
    MoT text prefix qkv, o, gate-up, down und 40 (geo empty)            2048 .. 17920 1536, 8960  skinny     64    8/1, 8/1, 4/1, 4/18
    decode qkv, o, gate-up, lm_head       B = 1 .. 8                    2048 .. 151936  1536      skinny     16    4/1
    decode down                           B = 1 .. 8                    1536          8960        skinny     16    4/6

The rows are derived the way the engine derives them (engine_rows: P patches per view, the two vision markers per view of
host.prepare_image_tokens as the und group).  The big tile serves production only in the ViT-image prefill's narrow Linears
and the one-image merger m2; the 128x128 kernel only the C2 decoders' ckv.

Bounds and measured maxima (MI355X runs of this module; the larger of two runs where they differ).  tau stays 2^-16: the
largest implied accumulation error d measured per form is 7.03e-8 T (8p), 4.82e-8 (4w), 3.94e-8 (128x128), 5.29e-8 (big),
1.38e-8 (skinny), 2.64e-8 (the A/B loops) - about 2^-24 T, 2^8 below tau.  Activation epilogues, largest distance to the fp64
range beyond the floor: GELU 0.5 ulp (every form) -> bound 0.75; QuickGELU 1.53 ulp (big; 1.5 on 8p / 4w, 1.35 on 128x128,
0.99 skinny) -> bound 2 (1.5 x 1.53 capped); SwiGLU 1.75 ulp (every tiled form; 1.42 skinny) -> bound 2 (capped): the device
sigmoid / SiLU and the fp64 function land on different sides of a bf16 rounding point of the intermediate value.  Share of
elements with more than one admissible Linear value: 11 - 38 % per form (K 64 - 8960), 47 - 55 % for SwiGLU (gate or up).
gemm_f32: largest |got - ref| / (K 2^-24 T) = 0.011 (K 512), 0.0062 (K 1024).  The whole module runs in under 30 s on one
MI355X.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_check as G  # noqa: E402
from g2vlm_amd import host  # noqa: E402

pytestmark = pytest.mark.gpu

ROUTE_ENV = bool(os.environ.get("G2V_GEMM_FLAGS") or os.environ.get("G2V_GEMM_4W_MASK"))
STATS = {}                          # (form, epilogue) -> measured maxima, printed at module teardown


@pytest.fixture(scope="module", autouse=True)
def measured_maxima():
    """Prints the measured maxima the module docstring quotes (visible with -s) once the module's tests have run."""
    yield
    for k, v in sorted(STATS.items()):
        if "n" in v:
            v = dict(v, multi_share=v["multi"] / max(v["n"], 1))
        print("STATS", k, {kk: (f"{vv:.3g}" if isinstance(vv, float) else vv) for kk, vv in v.items()})


@pytest.fixture(scope="module")
def hip():
    from g2vlm_amd import hip as h
    h.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return h


def gen(seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    return g


def pow2(n, spread, g):
    """per-row scale factors: powers of two over [-spread, spread] for half the rows, 1 for the rest"""
    e = torch.randint(-spread, spread + 1, (n,), generator=g, device="cuda").double()
    keep = torch.rand(n, generator=g, device="cuda") < 0.5
    return torch.where(keep, torch.zeros_like(e), e).exp2() if spread else torch.ones(n, dtype=torch.float64, device="cuda")


def sentinel(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    if dtype == torch.bfloat16:
        t.view(torch.int16).fill_(G.NAN_BF16)
    else:
        t.view(torch.int32).fill_(G.NAN_F32)
    return t


def is_sentinel(t):
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16) == G.NAN_BF16
    return t.view(torch.int32) == G.NAN_F32


def record(form, epi, chk):
    s = STATS.setdefault((form, G.EPI_NAMES[epi]), dict(max_d=0.0, max_ulps=0.0, multi=0, n=0))
    s["max_d"] = max(s["max_d"], chk.max_d)
    s["max_ulps"] = max(s["max_ulps"], chk.max_ulps)
    s["multi"] += chk.multi
    s["n"] += chk.n


class Launch:
    """One g2v_gemm_bf16 launch with up to two groups, laid out with sentinels:
    A   [sum(M) + 5, lda]   bf16, group i at rows a0[i]; columns >= K and the trailing rows NaN
    C   [sum(M + gap) + 3, ldc], group i at rows c0[i]; everything outside the M x n_out blocks a sentinel
    res separate [M, ldres] per group (NaN past N), or C itself (in place: the block pre-filled with the residual)."""

    def __init__(self, hip, epi, Ms, N, K, lda_pad=0, ldc_pad=0, ldres_pad=0, bias=True, res=True, gammas=None,
                 round_gamma=False, inplace=False, spread=12, seed=0, gap=3):
        self.hip, self.epi, self.Ms, self.N, self.K = hip, epi, list(Ms), N, K
        g = gen(seed)
        self.n_out = N // 2 if epi == G.EPI_SWIGLU else N
        self.lda, self.ldc = K + lda_pad, self.n_out + ldc_pad
        out_dt = torch.float32 if epi == G.EPI_RES_F32 else torch.bfloat16
        rows = sum(Ms)
        Abuf = sentinel((rows + 5, self.lda), torch.bfloat16)
        self.a0 = [sum(Ms[:i]) for i in range(len(Ms))]
        Cbuf = sentinel((sum(m + gap for m in Ms) + 3, self.ldc), out_dt)
        self.c0 = [sum(m + gap for m in Ms[:i]) + gap for i in range(len(Ms))]
        self.groups, self.refs = [], []
        has_res = epi in (G.EPI_RES_F32, G.EPI_RES_BF16) and res
        self.ldres = 0
        if has_res:
            self.ldres = self.ldc if inplace else N + ldres_pad
        for i, M in enumerate(Ms):
            rs = pow2(M, spread, g)
            A = (torch.randn(M, K, generator=g, device="cuda", dtype=torch.float64) * rs[:, None]).bfloat16()
            Abuf[self.a0[i]:self.a0[i] + M, :K] = A
            cs = pow2(N, spread, g)
            W = (torch.randn(N, K, generator=g, device="cuda", dtype=torch.float64) * K ** -0.5 * cs[:, None]).bfloat16()
            b = None
            if bias and epi != G.EPI_SWIGLU:
                bb = sentinel((N + 8,), torch.bfloat16)
                bb[:N] = (torch.randn(N, generator=g, device="cuda", dtype=torch.float64) * 0.3 * cs).bfloat16()
                b = bb[:N]
            gam = None
            if epi == G.EPI_RES_F32 and gammas is not None and gammas[i]:
                gb = sentinel((N + 8,), torch.float32)
                gb[:N] = (1 + 0.1 * torch.randn(N, generator=g, device="cuda")) * torch.where(
                    torch.rand(N, generator=g, device="cuda") < 0.1, -1.0, 1.0)
                gam = gb[:N]
            C = Cbuf[self.c0[i]:self.c0[i] + M]
            r = r_copy = None
            if has_res:
                rv = torch.randn(M, N, generator=g, device="cuda", dtype=torch.float64) * rs[:, None] * cs[None, :]
                rv = rv.to(out_dt)
                if inplace:
                    C[:, :N] = rv
                    r = C
                else:
                    rbuf = sentinel((M + 1, self.ldres), out_dt)
                    rbuf[:M, :N] = rv
                    r = rbuf[:M]
                r_copy = rv.clone()
            # an empty group still carries valid pointers (the views run to the end of their buffers)
            self.groups.append(dict(A=Abuf[self.a0[i]:], W=W, bias=b, C=Cbuf[self.c0[i]:], res=Cbuf[self.c0[i]:] if inplace and has_res else r,
                                    gamma=gam, M=M))
            self.refs.append(dict(A=Abuf[self.a0[i]:self.a0[i] + M, :K], W=W, bias=b, res=r_copy, gamma=gam))
        self.Abuf, self.Cbuf, self.round_gamma = Abuf, Cbuf, round_gamma
        self.flags = hip.GAMMA_ROUND_BF16 if round_gamma else 0

    def args(self, flags, ws):
        return (self.groups, self.N, self.K, self.epi), dict(out_ld=self.ldc, lda=self.lda, ldres=self.ldres,
                                                            flags=self.flags | flags, ws=ws)

    def route(self, flags=0, ws=None):
        a, kw = self.args(flags, ws)
        return self.hip.gemm_route(*a, **kw)

    def run(self, flags=0, ws=None):
        a, kw = self.args(flags, ws)
        self.hip.gemm_bf16(*a, **kw)
        torch.cuda.synchronize()

    def check(self, form, tile=None, what=""):
        """Every group against fp64; every sentinel intact."""
        keep = torch.ones(self.Cbuf.shape, dtype=torch.bool, device="cuda")
        for i, M in enumerate(self.Ms):
            keep[self.c0[i]:self.c0[i] + M, :self.n_out] = False
        assert bool(is_sentinel(self.Cbuf)[keep].all()), f"{what}: output sentinel overwritten"
        for i, M in enumerate(self.Ms):
            rf = self.refs[i]
            got = self.Cbuf[self.c0[i]:self.c0[i] + M, :self.n_out]
            chk = G.check_gemm(got, rf["A"], rf["W"], rf["bias"], self.epi, res=rf["res"], gamma=rf["gamma"],
                               round_gamma=self.round_gamma)
            record(form, self.epi, chk)
            assert chk.count == 0, chk.report(tile, f"{what} group {i}")

    def output(self):
        return self.Cbuf.clone()


EPIS = {"bf16": (G.EPI_BF16, {}), "gelu": (G.EPI_GELU, {}), "quickgelu": (G.EPI_QUICKGELU, {}), "swiglu": (G.EPI_SWIGLU, {}),
        "res_bf16_inplace": (G.EPI_RES_BF16, dict(inplace=True)),
        "res_bf16_ldres": (G.EPI_RES_BF16, dict(ldres_pad=24)),
        "res_f32_gamma_round": (G.EPI_RES_F32, dict(gammas=(True, True), round_gamma=True, ldres_pad=12)),
        "res_f32_gamma_inplace": (G.EPI_RES_F32, dict(gammas=(True, True), inplace=True)),
        "res_f32_res_inplace": (G.EPI_RES_F32, dict(inplace=True)),
        "res_f32_neither": (G.EPI_RES_F32, dict(res=False))}
HEIGHTS = (128, 160, 192, 224, 256, 288)


def hflag(hip, h):
    return {128: hip.P8_H128, 160: hip.P8_H160, 192: hip.P8_H192, 224: hip.P8_H224, 256: hip.P8_H256, 288: hip.P8_H288}[h]


def expect_route(route, form, height=None):
    if ROUTE_ENV:
        return
    assert route[0] == form, route
    if height is not None:
        assert route[1] == height, route


# ----------------------------------------------------------------------------------------------- section 1
def test_reference_on_device_matches_cpu(hip):
    """check_gemm's on-device float64 reference (gemm_check.linear64) against a CPU float64 matmul of the same operands:
    v* and T agree to 1e-12 of T."""
    g = gen(3)
    K = 1536
    A = (torch.randn(200, K, generator=g, device="cuda") * 2).bfloat16()
    W = (torch.randn(300, K, generator=g, device="cuda") * K ** -0.5).bfloat16()
    b = torch.randn(300, generator=g, device="cuda").bfloat16()
    v, T = G.linear64(A, W, b)
    vc, Tc = G.linear64(A.cpu(), W.cpu(), b.cpu())
    assert float(((v.cpu() - vc).abs() / Tc).max()) <= 1e-12
    assert float(((T.cpu() - Tc).abs() / Tc).max()) <= 1e-12


@pytest.mark.parametrize("epi_name", list(EPIS))
@pytest.mark.parametrize("form", ["8p", "4w"])
def test_form_256_every_height(hip, form, epi_name):
    """The 256-column forms at every tile height: the last row tile at M - m0 in {1, HB-1, HB, HB+1, bm-1, bm} (second tile
    row), K of 2 and 3 K-tiles (the minimum and an odd count), two tile columns."""
    epi, kw = EPIS[epi_name]
    fl = hip.FORCE_8P | (hip.P8_EIGHT_WAVES if form == "8p" else hip.P8_FOUR_WAVES)
    for h in HEIGHTS:
        HB = h // 2
        K = 128 if h in (128, 192, 256) else 192
        for j, t in enumerate((1, HB - 1, HB, HB + 1, h - 1, h)):
            M = h + t
            L = Launch(hip, epi, [M], 512, K, lda_pad=64, ldc_pad=16, seed=1000 * h + j, **kw)
            expect_route(L.route(fl | hflag(hip, h)), form, h)
            L.run(fl | hflag(hip, h))
            L.check(form, (h, 256), f"{form} h{h} M{M} K{K} {epi_name}")


@pytest.mark.parametrize("epi_name", list(EPIS))
def test_form_128x128_edges(hip, epi_name):
    """128x128 kernel: rows at the 64-row wave boundaries of the second tile row, N % 128 != 0 (and N % 16 != 0 off SwiGLU),
    K % 64 != 0, lda > K, ldc > N."""
    epi, kw = EPIS[epi_name]
    N = 224 if epi == G.EPI_SWIGLU else 200
    for j, t in enumerate((1, 63, 64, 65, 127, 128)):
        for K in (200, 64):
            L = Launch(hip, epi, [128 + t], N, K, lda_pad=8, ldc_pad=8 if epi != G.EPI_RES_F32 else 4, seed=50 + j, **kw)
            expect_route(L.route(hip.FORCE_SMALL_TILE), "128x128", 128)
            L.run(hip.FORCE_SMALL_TILE)
            L.check("128x128", (128, 128), f"128x128 M{128 + t} N{N} K{K} {epi_name}")


@pytest.mark.parametrize("epi_name", list(EPIS))
def test_form_big_tile_edges(hip, epi_name):
    """gemm_big.hip: M % 32 tails (its tile height is a multiple of 32 chosen by the launcher), K of 3 K-tiles.  At N 512 the
    launcher picks 32-row tiles (the production ViT-prefill launches use that height too); N 2048 with a few thousand rows
    reaches 96, 160, 224 and 288 (3, 5, 7 and 9 m-tiles per wave)."""
    epi, kw = EPIS[epi_name]
    for j, (M, N, h) in enumerate(((1, 512, 32), (31, 512, 32), (33, 512, 32), (289, 512, 32), (545, 512, 32), (1087, 512, 32),
                                   (3001, 2048, 96), (5000, 2048, 160), (7001, 2048, 224), (9000, 2048, 288))):
        L = Launch(hip, epi, [M], N, 192, lda_pad=64, ldc_pad=16, seed=70 + j, **kw)
        r = L.route(hip.FORCE_BIG_TILE)
        expect_route(r, "big", h)
        L.run(hip.FORCE_BIG_TILE)
        L.check("big", (r[1], 256), f"big M{M} N{N} {epi_name}")


def test_ab_loops(hip):
    """The A/B-only main loops get one pass each over every height: the lockstep two-barrier loop, round 1's pipelined loop,
    and the 8-wave form without the wave-row MFMA skip."""
    for name, fl in (("two_barrier", hip.P8_TWO_BARRIER), ("pipelined", hip.P8_PIPELINED),
                     ("no_row_skip", hip.P8_EIGHT_WAVES | hip.P8_NO_ROW_SKIP)):
        for h in HEIGHTS:
            HB = h // 2
            for j, t in enumerate((1, HB + 1, h)):
                L = Launch(hip, G.EPI_BF16, [h + t], 256, 192, lda_pad=64, ldc_pad=16, seed=90 + h + j)
                expect_route(L.route(hip.FORCE_8P | fl | hflag(hip, h)), "8p", h)
                L.run(hip.FORCE_8P | fl | hflag(hip, h))
                L.check("8p_" + name, (h, 256), f"{name} h{h} M{h + t}")


@pytest.mark.parametrize("epi_name", list(EPIS))
def test_skinny_rows(hip, epi_name):
    """Default dispatch for M <= 64: the m-tile switches at 16 / 32, the in-workgroup K split."""
    epi, kw = EPIS[epi_name]
    for j, M in enumerate((1, 15, 16, 17, 32, 33, 63, 64)):
        L = Launch(hip, epi, [M], 256, 640, lda_pad=64, ldc_pad=8, seed=110 + j, **kw)
        r = L.route()
        expect_route(r, "skinny", 16 if M <= 16 else (32 if M <= 32 else 64))
        L.run()
        L.check("skinny", (r[1], 16), f"skinny M{M} {epi_name}")


@pytest.mark.parametrize("K", [4032, 4096, 8960])
def test_skinny_cross_workgroup_split(hip, K):
    """K on both sides of the cross-workgroup threshold (64 k-steps = K 4096) and the down projection's 8960, with a large
    caller workspace, the default one, one that fits exactly KS = 2, and one too small (the in-workgroup fallback)."""
    M, N = 8, 1536
    part = (N // 16) * 256 * 4                     # fp32 partials of one K slice: 96 column groups x one 16-row m-tile
    exact = torch.zeros((65536 + 2 * part) // 4, dtype=torch.int32, device="cuda")
    for name, ws in (("large", torch.zeros(4 << 20, dtype=torch.int32, device="cuda")), ("default", None),
                     ("exact2", exact), ("tiny", torch.zeros(64, dtype=torch.int32, device="cuda"))):
        for epi_name in ("bf16", "res_f32_res_inplace"):
            epi, kw = EPIS[epi_name]
            L = Launch(hip, epi, [M], N, K, lda_pad=64, seed=130 + K, **kw)
            r = L.route(ws=ws)
            if not ROUTE_ENV:
                assert r[0] == "skinny"
                if K < 4096 or name == "tiny":
                    assert r[3] == 1, (name, r)
                elif name == "exact2":
                    assert r[3] == 2, (name, r)
                else:
                    assert r[3] > 2, (name, r)
            L.run(ws=ws)
            L.check("skinny", (16, 16), f"skinny K{K} ws {name} {epi_name} route {r}")


@pytest.mark.parametrize("form", ["8p", "4w", "128x128", "big", "skinny"])
def test_two_groups(hip, form):
    """Two-group launches (the MoT und / geo experts): und M in {1, 6, 16, HB, HB+1} beside geo rows with tails, either
    group empty, either order; bias, residual and gamma per group with gamma on one group only (MoT o / down: in place,
    GAMMA_ROUND_BF16)."""
    fl = {"8p": hip.FORCE_8P | hip.P8_EIGHT_WAVES | hip.P8_H256, "4w": hip.FORCE_8P | hip.P8_FOUR_WAVES | hip.P8_H256,
          "128x128": hip.FORCE_SMALL_TILE, "big": hip.FORCE_BIG_TILE, "skinny": 0}[form]
    geo = 40 if form == "skinny" else 700
    cases = [(geo, u) for u in (1, 6, 16, 128, 129)] + [(geo, 0), (0, 9 if form == "skinny" else 300)]
    if form == "skinny":
        cases = [(0, u) for u in (1, 6, 16, 33)] + [(u, 0) for u in (7, 64)]
    for j, (mg, mu) in enumerate(cases):
        for order in ((0, 1), (1, 0)):
            Ms = [(mg, mu)[o] for o in order]
            gam = tuple((True, False)[o] for o in order)
            for epi_name, epi, kw in (("res_f32_mot", G.EPI_RES_F32, dict(gammas=gam, round_gamma=True, inplace=True, bias=False)),
                                      ("bf16", G.EPI_BF16, {}), ("swiglu", G.EPI_SWIGLU, {})):
                L = Launch(hip, epi, Ms, 512, 256, lda_pad=64, ldc_pad=16 if epi != G.EPI_RES_F32 else 8,
                           seed=150 + 10 * j + order[0], **kw)
                r = L.route(fl)
                if not ROUTE_ENV:
                    assert r[0] == form, (form, Ms, r)
                L.run(fl)
                L.check(form, (r[1], 256), f"{form} groups {Ms} {epi_name}")


@pytest.mark.parametrize("form", ["8p", "4w"])
def test_form_256_persistent_two_groups(hip, form):
    """The persistent tile loop of the 256-column forms at its smallest: two groups with more 128-row tiles than the chip has
    CUs (8 tile columns; 128 ceil(CUs / 8) + 1 rows, so the last tile row holds one row, beside a 6-row group), either order,
    so a workgroup finishes a tile of one group with the first K-tile of a tile of the other group already in flight.  SwiGLU
    and the in-place fp32 residual with gamma."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    fl = hip.FORCE_8P | (hip.P8_EIGHT_WAVES if form == "8p" else hip.P8_FOUR_WAVES) | hip.P8_H128
    rows = (128 * ((n_cu + 7) // 8) + 1, 6)
    assert (sum((m + 127) // 128 for m in rows)) * 8 > n_cu
    for order in ((0, 1), (1, 0)):
        Ms = [rows[o] for o in order]
        for epi_name in ("swiglu", "res_f32_gamma_inplace"):
            epi, kw = EPIS[epi_name]
            L = Launch(hip, epi, Ms, 2048, 128, lda_pad=64, ldc_pad=16, seed=170 + order[0], **kw)
            expect_route(L.route(fl), form, 128)
            L.run(fl)
            L.check(form, (128, 256), f"{form} persistent groups {Ms} {epi_name}")


def test_sensitivity_one_zeroed_element(hip):
    """A single A element zeroed in one row of a real-shape launch (MoT down at C2: 1558 x 1536, K 8960): the check flags that
    row and no other, while the older tests' assert_bf16_close accepts the output."""
    M, N, K, row, k = 1558, 1536, 8960, 777, 4321
    g = gen(7)
    A = (torch.randn(M, K, generator=g, device="cuda") * 0.5).bfloat16()
    W = (torch.randn(N, K, generator=g, device="cuda") * K ** -0.5).bfloat16()
    A0 = A.clone()
    A0[row, k] = 0
    out = hip.linear(A0, W)
    chk = G.check_gemm(out, A, W)
    assert chk.flagged_rows() == [row], chk.report(what="sensitivity")
    from test_gemm_check_cpu import assert_bf16_close
    assert_bf16_close(out.cpu(), torch.nn.functional.linear(A.cpu(), W.cpu()))


# ----------------------------------------------------------------------------------------------- section 2
def engine_rows(n_views, gh, gw):
    """Row counts of one scene as the engine launches them.  The MoT sequence is what host.prepare_image_tokens lays out for
    forward_cache_update_dino: per view <|vision_start|>, the gh x gw patch rows, <|vision_end|>; llm_forward gets
    split = N P, so the geo group is the patch rows and the und group the markers.  The DINOv2 layers and dino2llm run on
    N (P + 5) rows (cls + 4 registers per view), the patch embed and the Pi3 decoders on N P, a decoder's ckv on P."""
    gi, _, _ = host.prepare_image_tokens(0, 0, [(1, gh, gw)] * n_views, {"start_of_image": 0, "end_of_image": 1})
    P, L, und = gh * gw, int(gi["packed_seqlens"][0]), len(gi["packed_text_ids"])
    assert L - und == n_views * P
    return dict(P=P, patch=n_views * P, dino=n_views * (P + 5), geo=L - und, und=und)


def vit_prefill_rows(gh=54, gw=54):
    """forward_cache_update_vit of one image: the merger's gh/2 x gw/2 tokens between two markers, all und (split 0)."""
    gi, _, _ = host.prepare_image_tokens(0, 0, [(1, gh, gw)], {"start_of_image": 0, "end_of_image": 1}, merge=2)
    return int(gi["packed_seqlens"][0])


SCENES = {"C3": engine_rows(8, 37, 37), "C2": engine_rows(2, 21, 37)}     # 8 views 518 x 518, 2 views 294 x 518
VIT_IMAGE = 54 * 54                                                        # ViT patch rows of one image (756 x 756)
TEXT_PREFIX = 40                                                           # rows of a text-prefix prefill (skinny path)
# name: (groups' rows (MoT: [geo, und]), N, K, epilogue, options)
PRODUCTION = {}
for _c, _r in SCENES.items():
    PRODUCTION.update({
        f"dino_patch_{_c}": ([_r["patch"]], 1024, 640, "bf16", {}),
        f"dino_qkv_{_c}": ([_r["dino"]], 3072, 1024, "bf16", {}),
        f"dino_dense_{_c}": ([_r["dino"]], 1024, 1024, "res_f32", dict(gammas=(True,), inplace=True)),
        f"dino_fc1_{_c}": ([_r["dino"]], 4096, 1024, "gelu", {}),
        f"dino_fc2_{_c}": ([_r["dino"]], 1024, 4096, "res_f32", dict(gammas=(True,), inplace=True)),
        f"dino2llm_{_c}": ([_r["dino"]], 1536, 1024, "res_f32", dict(res=False)),
        f"dec_qkv_{_c}": ([_r["patch"]], 4608, 1536, "bf16", {}),
        f"dec_proj_{_c}": ([_r["patch"]], 1536, 1536, "res_f32", dict(inplace=True)),
        f"dec_ckv_{_c}": ([_r["P"]], 3072, 1536, "bf16", {}),
        f"dec_cq_{_c}": ([_r["patch"]], 1536, 1536, "bf16", {}),
        f"dec_cproj_{_c}": ([_r["patch"]], 1536, 1536, "res_f32", dict(inplace=True)),
        f"dec_fc1_{_c}": ([_r["patch"]], 6144, 1536, "gelu", {}),
        f"dec_fc2_{_c}": ([_r["patch"]], 1536, 6144, "res_f32", dict(inplace=True)),
        f"dec_out1024_{_c}": ([_r["patch"]], 1024, 1536, "bf16", {}),
        f"dec_out512_{_c}": ([_r["patch"]], 512, 1536, "bf16", {}),
        f"mot_qkv_{_c}": ([_r["geo"], _r["und"]], 2048, 1536, "bf16", {}),
        f"mot_o_{_c}": ([_r["geo"], _r["und"]], 1536, 1536, "res_f32_mot", {}),
        f"mot_gu_{_c}": ([_r["geo"], _r["und"]], 17920, 1536, "swiglu", {}),
        f"mot_down_{_c}": ([_r["geo"], _r["und"]], 1536, 8960, "res_f32_mot", {}),
    })
for _n in (1, 8):
    PRODUCTION.update({
        f"vit_patch_{_n}": ([_n * VIT_IMAGE], 1280, 1216, "bf16", dict(bias=False)),
        f"vit_qkv_{_n}": ([_n * VIT_IMAGE], 3840, 1280, "bf16", {}),
        f"vit_proj_{_n}": ([_n * VIT_IMAGE], 1280, 1280, "res_bf16", dict(inplace=True)),
        f"vit_fc1_{_n}": ([_n * VIT_IMAGE], 5120, 1280, "quickgelu", {}),
        f"vit_fc2_{_n}": ([_n * VIT_IMAGE], 1280, 5120, "res_bf16", dict(inplace=True)),
        f"vit_m0_{_n}": ([_n * VIT_IMAGE // 4], 5120, 5120, "gelu", {}),
        f"vit_m2_{_n}": ([_n * VIT_IMAGE // 4], 1536, 5120, "bf16", {}),
    })
for _tag, _m in (("vit_prefill", vit_prefill_rows()), ("text_prefix", TEXT_PREFIX)):     # und only: the geo group is empty
    PRODUCTION.update({
        f"mot_qkv_{_tag}": ([0, _m], 2048, 1536, "bf16", {}),
        f"mot_o_{_tag}": ([0, _m], 1536, 1536, "res_f32_mot", {}),
        f"mot_gu_{_tag}": ([0, _m], 17920, 1536, "swiglu", {}),
        f"mot_down_{_tag}": ([0, _m], 1536, 8960, "res_f32_mot", {}),
    })
for _B in range(1, 9):                             # batched decode (decode.Decode._step): no bias on o / down, no gamma
    PRODUCTION[f"decode_qkv_B{_B}"] = ([_B], 2048, 1536, "bf16", {})
    PRODUCTION[f"decode_o_B{_B}"] = ([_B], 1536, 1536, "res_f32", dict(inplace=True, bias=False))
    PRODUCTION[f"decode_gu_B{_B}"] = ([_B], 17920, 1536, "swiglu", {})
    PRODUCTION[f"decode_down_B{_B}"] = ([_B], 1536, 8960, "res_f32", dict(inplace=True, bias=False))
for _B in (1, 8):
    PRODUCTION[f"decode_lm_head_B{_B}"] = ([_B], 151936, 1536, "bf16", dict(bias=False))

# the route each production case takes (g2v_gemm_route with the default G2V_GEMM_4W_MASK, measured on an MI355X)
ROUTES = {
    'dino_patch_C3': ('8p', 192, 1, 1),
    'dino_qkv_C3': ('8p', 288, 1, 1),
    'dino_dense_C3': ('4w', 192, 1, 1),
    'dino_fc1_C3': ('8p', 256, 1, 1),
    'dino_fc2_C3': ('4w', 192, 1, 1),
    'dino2llm_C3': ('4w', 288, 1, 1),
    'dec_qkv_C3': ('8p', 288, 1, 1),
    'dec_proj_C3': ('4w', 288, 1, 1),
    'dec_ckv_C3': ('8p', 128, 1, 1),
    'dec_cq_C3': ('8p', 288, 1, 1),
    'dec_cproj_C3': ('4w', 288, 1, 1),
    'dec_fc1_C3': ('8p', 288, 1, 1),
    'dec_fc2_C3': ('4w', 288, 1, 1),
    'dec_out1024_C3': ('8p', 192, 1, 1),
    'dec_out512_C3': ('8p', 128, 1, 1),
    'mot_qkv_C3': ('8p', 192, 1, 1),
    'mot_o_C3': ('4w', 288, 1, 1),
    'mot_gu_C3': ('8p', 288, 1, 1),
    'mot_down_C3': ('4w', 288, 1, 1),
    'dino_patch_C2': ('8p', 128, 1, 1),
    'dino_qkv_C2': ('8p', 128, 1, 1),
    'dino_dense_C2': ('4w', 128, 1, 1),
    'dino_fc1_C2': ('8p', 128, 1, 1),
    'dino_fc2_C2': ('4w', 128, 1, 1),
    'dino2llm_C2': ('4w', 128, 1, 1),
    'dec_qkv_C2': ('8p', 128, 1, 1),
    'dec_proj_C2': ('4w', 128, 1, 1),
    'dec_ckv_C2': ('128x128', 128, 1, 1),
    'dec_cq_C2': ('8p', 128, 1, 1),
    'dec_cproj_C2': ('4w', 128, 1, 1),
    'dec_fc1_C2': ('8p', 160, 1, 1),
    'dec_fc2_C2': ('4w', 128, 1, 1),
    'dec_out1024_C2': ('8p', 128, 1, 1),
    'dec_out512_C2': ('8p', 128, 1, 1),
    'mot_qkv_C2': ('8p', 128, 1, 1),
    'mot_o_C2': ('4w', 128, 1, 1),
    'mot_gu_C2': ('8p', 288, 1, 1),
    'mot_down_C2': ('4w', 128, 1, 1),
    'vit_patch_1': ('8p', 128, 1, 1),
    'vit_qkv_1': ('8p', 192, 1, 1),
    'vit_proj_1': ('8p', 128, 1, 1),
    'vit_fc1_1': ('8p', 256, 1, 1),
    'vit_fc2_1': ('4w', 128, 1, 1),
    'vit_m0_1': ('4w', 128, 1, 1),
    'vit_m2_1': ('big', 32, 1, 1),
    'vit_patch_8': ('8p', 256, 1, 1),
    'vit_qkv_8': ('8p', 288, 1, 1),
    'vit_proj_8': ('8p', 256, 1, 1),
    'vit_fc1_8': ('8p', 288, 1, 1),
    'vit_fc2_8': ('4w', 256, 1, 1),
    'vit_m0_8': ('4w', 256, 1, 1),
    'vit_m2_8': ('4w', 160, 1, 1),
    'mot_qkv_vit_prefill': ('big', 32, 1, 1),
    'mot_o_vit_prefill': ('big', 32, 1, 1),
    'mot_gu_vit_prefill': ('8p', 256, 1, 1),
    'mot_down_vit_prefill': ('big', 32, 1, 1),
    'mot_qkv_text_prefix': ('skinny', 64, 8, 1),
    'mot_o_text_prefix': ('skinny', 64, 8, 1),
    'mot_gu_text_prefix': ('skinny', 64, 4, 1),
    'mot_down_text_prefix': ('skinny', 64, 4, 18),
    'decode_qkv_B1': ('skinny', 16, 4, 1),
    'decode_o_B1': ('skinny', 16, 4, 1),
    'decode_gu_B1': ('skinny', 16, 4, 1),
    'decode_down_B1': ('skinny', 16, 4, 6),
    'decode_qkv_B2': ('skinny', 16, 4, 1),
    'decode_o_B2': ('skinny', 16, 4, 1),
    'decode_gu_B2': ('skinny', 16, 4, 1),
    'decode_down_B2': ('skinny', 16, 4, 6),
    'decode_qkv_B3': ('skinny', 16, 4, 1),
    'decode_o_B3': ('skinny', 16, 4, 1),
    'decode_gu_B3': ('skinny', 16, 4, 1),
    'decode_down_B3': ('skinny', 16, 4, 6),
    'decode_qkv_B4': ('skinny', 16, 4, 1),
    'decode_o_B4': ('skinny', 16, 4, 1),
    'decode_gu_B4': ('skinny', 16, 4, 1),
    'decode_down_B4': ('skinny', 16, 4, 6),
    'decode_qkv_B5': ('skinny', 16, 4, 1),
    'decode_o_B5': ('skinny', 16, 4, 1),
    'decode_gu_B5': ('skinny', 16, 4, 1),
    'decode_down_B5': ('skinny', 16, 4, 6),
    'decode_qkv_B6': ('skinny', 16, 4, 1),
    'decode_o_B6': ('skinny', 16, 4, 1),
    'decode_gu_B6': ('skinny', 16, 4, 1),
    'decode_down_B6': ('skinny', 16, 4, 6),
    'decode_qkv_B7': ('skinny', 16, 4, 1),
    'decode_o_B7': ('skinny', 16, 4, 1),
    'decode_gu_B7': ('skinny', 16, 4, 1),
    'decode_down_B7': ('skinny', 16, 4, 6),
    'decode_qkv_B8': ('skinny', 16, 4, 1),
    'decode_o_B8': ('skinny', 16, 4, 1),
    'decode_gu_B8': ('skinny', 16, 4, 1),
    'decode_down_B8': ('skinny', 16, 4, 6),
    'decode_lm_head_B1': ('skinny', 16, 4, 1),
    'decode_lm_head_B8': ('skinny', 16, 4, 1),
}


@pytest.mark.parametrize("name", list(PRODUCTION))
def test_production(hip, name):
    Ms_all, N, K, epi_name, kw = PRODUCTION[name]
    want = ROUTES[name]
    kw = dict(kw)
    Ms = [m for m in Ms_all if m]                    # engine.py passes only the non-empty expert groups
    if epi_name == "res_f32_mot":                   # MoT o / down: gamma on the geo group only, rounded, in place, no bias
        epi = G.EPI_RES_F32
        kw.update(gammas=tuple(g for g, m in zip((True, False), Ms_all) if m), round_gamma=True, inplace=True, bias=False)
    else:
        epi = {"bf16": G.EPI_BF16, "gelu": G.EPI_GELU, "quickgelu": G.EPI_QUICKGELU, "swiglu": G.EPI_SWIGLU,
               "res_f32": G.EPI_RES_F32, "res_bf16": G.EPI_RES_BF16}[epi_name]
        if epi == G.EPI_SWIGLU:
            kw["bias"] = False
    L = Launch(hip, epi, Ms, N, K, spread=0, seed=sum(name.encode()) % 1000, gap=0, **kw)
    ws = torch.zeros(hip.GEMM_WS_WORDS, dtype=torch.int32, device="cuda") if max(Ms) <= 64 else None
    r = L.route(ws=ws)
    print(f"ROUTE {name} rows {Ms_all} N {N} K {K}: {r}")
    if not ROUTE_ENV:
        assert tuple(r) == want, r
    inplace = kw.get("inplace", False)
    snap = L.Cbuf.clone()
    outs = []
    for _ in range(5):
        if inplace:
            L.Cbuf.copy_(snap)
        L.run(ws=ws)
        outs.append(L.output())
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16) if o.dtype == torch.bfloat16 else o.view(torch.int32),
                           outs[0].view(torch.int16) if o.dtype == torch.bfloat16 else outs[0].view(torch.int32)), name
    L.check(r[0], (r[1], 256), name)


# ----------------------------------------------------------------------------------------------- section 3
@pytest.mark.parametrize("M,N,K,relu,res,lda_pad", [
    (8 * 1369, 588, 1024, False, False, 0),        # point head 1024 -> 588 (14 x 14 x 3), C3
    (2 * 777, 588, 1024, False, False, 12),        # global head, C2, lda > K
    (8 * 1369, 196, 1024, False, False, 0),        # conf head
    (8 * 1369, 512, 512, True, False, 0),          # camera res-block .1 / .2: ReLU
    (8 * 1369, 512, 512, True, True, 0),           # camera res-block .3: ReLU, then the residual (engine.camera_poses)
    (333, 77, 1028, True, True, 4),                # N tail, K % 16 != 0, lda > K
])
def test_gemm_f32_heads(hip, M, N, K, relu, res, lda_pad):
    g = gen(M + N + K)
    Abuf = torch.full((M, K + lda_pad), float("nan"), device="cuda")
    Abuf[:, :K] = torch.randn(M, K, generator=g, device="cuda")
    A = Abuf[:, :K]
    W = torch.randn(N, K, generator=g, device="cuda") * K ** -0.5
    b = torch.randn(N, generator=g, device="cuda")
    r = torch.randn(M, N, generator=g, device="cuda") if res else None
    got = hip.gemm_f32(A, W, b, relu=relu, res=r)
    bad, ratio = G.check_f32(got, A, W, b, relu, r)
    s = STATS.setdefault(("gemm_f32", f"K{K}"), dict(ratio=0.0))
    s["ratio"] = max(s["ratio"], ratio)
    assert not bool(bad.any()), (int(bad.sum()), ratio)

