"""Operands, launch table and fp64 checks for the GEMVs and attentions of the decode step: csrc/decode.hip (first generation),
csrc/decode_layer.hip (g2v_gemv_pg, g2v_decode_attn_pg), csrc/decode_batch.hip (g2v_gemv_pg_batch) and their e4m3 twins in
csrc/decode_fp8.hip.

A helper module (pytest does not collect it): test_decode_check_cpu.py tests the table and the checks without a GPU,
test_decode_fp64_gpu.py applies them to the bf16 kernels; test_fp8_decode_check_cpu.py and test_fp8_decode_gpu.py do the same
with the e4m3 table (TABLE8) and kernels.

GEMVs.  Every output is checked element by element with gemm_check.check_gemm, unchanged: TAU = 2^-16, ULP_BOUND[EPI_SWIGLU] =
2.0, zero flags, no fraction allowance.  The persistent-grid kernels accumulate with v_dot2 over at most 18 chunk steps per lane,
a 6-step wave sum (wave_sum_dpp or reduce_transpose), in the long-K batched form 8 wave shares added in order, and then round
bfround(v + bias) and add res + v: the arithmetic the e4m3 kernels share and pass at 1.1e-8 T.  The first-generation kernel is
a per-thread fmaf chain of at most K / 256 + 8 terms, a 6-step wave sum and 3 adds: at K = 9216 under 50 x 2^-24 T, below TAU.

The operand of a fused form is the one the kernel multiplied, read back through the entry point under test and a K x K bf16
identity (one nonzero term per output row: the accumulation is exact):
  * fused RMSNorm: the normalised bf16 row.  Not shared across entry points: the first generation sums the squares per thread
    with stride 1024 and adds four wave sums through LDS, gemv_pg and gemv_pgb sum per lane over 3 chunk steps and a DPP wave sum.
    Each readback is checked against rowop_check.rmsnorm64 with rowop_check.check_out at rowop_check.TAU = 2^-19, zero flags.
    The gemv_pg roundings: at most 12 pair adds per lane (3 chunk steps x 4), 6 DPP adds, 4 for divide, + eps, sqrt and
    reciprocal, 2 multiplies, each at most 2^-24 relative, the sum's share halved by the root: (18 / 2 + 4 + 2) x 2^-24 = 15 x
    2^-24 < 2^-20 of |y|.  A case whose share of elements with more than one admissible value exceeds rowop_check.MULTI_CAP fails.
  * the SwiGLU input of gemv_swiglu_bf16: read back with `res` pre-filled with zeros; it must equal hip.swiglu_bf16 on the same
    gate/up vector bit for bit (both evaluate bfround(bfround(siluf_(g)) * u)), and swiglu_bf16 must lie within
    ULP_BOUND[EPI_SWIGLU] bf16 ulps of the fp64 function.

Attention.  attention64 is the fp64 softmax attention of one query token; row_metrics gives the two figures
tests/test_kv8_gpu.py::check_step asserts on the same kernel body: rel-L2 < REL_BOUND = 4e-3 and the worst element <
ELEM_BOUND = 2^-6 of the row's rms.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_check as G  # noqa: E402
import rowop_check as R  # noqa: E402
from g2vlm_amd.weights import interleave_gate_up  # noqa: E402

EPS = 1e-6
REL_BOUND, ELEM_BOUND = 4e-3, 2.0 ** -6
MEASURED = {}
GUARD = 2                                  # sentinel rows behind every target

# entry -> (batched, fp8).  'g1' is the first generation: the form picks the entry point (Case.run)
ENTRIES = {"pg": (False, False), "pgb": (True, False), "g1": (False, False), "pg8": (False, True), "pgb8": (True, True)}
NORM_FORMS = ("qkv", "gu", "lm")
RES_FORMS = ("o", "down", "sw")


def dev(t):
    return t.cuda()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(); g.manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def nan_bf16(*shape):
    return torch.full(shape, G.NAN_BF16, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def guard_flags(full, B):
    """Boolean map over the rows behind the first B of a target: the element no longer holds its sentinel."""
    return ~R.is_sentinel(full[B:])


def record(name, chk, extra="", store=None):
    m = (MEASURED if store is None else store).setdefault(name, dict(n=0, multi=0, max_ulps=0.0, max_d=0.0))
    m["n"] += chk.n; m["multi"] += chk.multi
    m["max_ulps"] = max(m["max_ulps"], chk.max_ulps); m["max_d"] = max(m["max_d"], chk.max_d)


_EYE = {}


def eye(K):
    if K not in _EYE:
        _EYE[K] = torch.eye(K, dtype=torch.bfloat16, device="cuda")
    return _EYE[K]


def normalised_rows(hip, xf, nw, entry="pg"):
    """bf16 [B, K]: the rows the fused-norm kernels of `entry` multiply, read back through that entry's norm form and an
    identity.  The e4m3 kernels sum the squares in gemv_pg's lane layout and order, so they read back through 'pg'."""
    B, K = xf.shape
    out = nan_bf16(B, K)
    if entry in ("pgb", "pgb8"):
        hip.gemv_pg_batch(xf, eye(K), norm_w=nw, eps=EPS, out=out)
    else:
        for b in range(B):
            if entry == "g1":
                hip.gemv_rmsnorm_bf16(xf[b], nw, EPS, eye(K), None, out[b])
            else:
                hip.gemv_pg(xf[b], eye(K), norm_w=nw, eps=EPS, out=out[b])
    return out


def swiglu_rows(hip, gu):
    """bf16 [B, K]: the activation gemv_swiglu_bf16 multiplies for gate/up rows gu bf16 [B, 2K], read back through an identity
    with the fp32 residual pre-filled with zeros (0 + bf16 value: exact)."""
    B, K = gu.shape[0], gu.shape[1] // 2
    res = torch.zeros((B, K), dtype=torch.float32, device="cuda")
    for b in range(B):
        hip.gemv_swiglu_bf16(gu[b], eye(K), res[b])
    back = res.bfloat16()
    assert torch.equal(back.float(), res)
    return back


def check_norm(A, x, nw):
    """rowop_check.Result of the read-back normalised rows A bf16 [B, K] against the fp64 RMSNorm of x fp32 [B, K]."""
    y, T = R.rmsnorm64(x, nw, nw, 0, EPS)
    return R.check_out(A, y, T)


def swiglu64(gu):
    """fp64 bf16(silu(g)) * u of gate/up rows interleaved per 16 (gemm_check.silu_r64: the kernel's intermediate rounding)."""
    v = gu.detach().cpu().double().view(gu.shape[0], -1, 2, 16)
    return (G.silu_r64(v[:, :, 0]) * v[:, :, 1]).reshape(gu.shape[0], -1)


def check_swiglu(got, gu):
    """gemm_check.Check of swiglu_bf16's output bf16 [B, K]: flags what lies more than ULP_BOUND[EPI_SWIGLU] bf16 ulps from the
    fp64 function; max_ulps is the largest distance."""
    got = got.detach().cpu()
    y = swiglu64(gu)
    chk = G.Check(got.shape[0], got.shape[1], got.device, G.EPI_SWIGLU)
    chk.bad = G._activation_bad(chk, got, y, y, torch.zeros_like(y), G.ULP_BOUND[G.EPI_SWIGLU]) | ~torch.isfinite(got.float())
    return chk


def row_exponents(N):
    """int [N]: the exponent of the e4m3 scale row n gets when Case draws per-row magnitudes: 16 consecutive values over the 16
    rows of a gate or up group, rotated by 5 from one group to the next.  Row n differs from n + d for every d a kernel could
    confuse it with: 1 (the pair partner, the next row), 16 (the gate/up partner), 2, 3, 4, 6, 8 and 12 (the same slot of the
    next batch)."""
    n = torch.arange(N)
    return (n % 16 + 5 * (n // 16)) % 16 - 19


def fp8_weight(form, N, K, seed, row_scales=False):
    """(q uint8 [N, K], s fp32 [N], wd bf16 [N, K] = the dequantised matrix) on the CPU, as Case draws them.  row_scales: every
    row is multiplied by the power of two that makes the quantiser's scale of row n exactly 2^row_exponents(N)[n] (a power of
    two commutes with the bf16 rounding and with the quantiser), instead of the random row factors of the 'lm' form."""
    from g2vlm_amd.quant import dequantize_rows, quantize_rows_e4m3
    w = rnd(N, K, seed=seed, scale=K ** -0.5)
    if form == "gu":
        w = interleave_gate_up(w[:N // 2].contiguous(), w[N // 2:].contiguous())
    if row_scales:
        _, s0 = quantize_rows_e4m3(w.bfloat16())
        w = w * (torch.ldexp(torch.ones(N), row_exponents(N)) / s0).unsqueeze(1)
    elif form == "lm":
        w = w * torch.exp(2.0 * rnd(N, seed=seed + 5)).unsqueeze(1)                      # heavy-tailed row scales (synth.peaked_lm_head)
    q, s = quantize_rows_e4m3(w.bfloat16())
    return q, s, dequantize_rows(q, s)


class Case:
    """Operands of one form.  form: 'qkv' (fp32 residual row, RMSNorm, bias, bf16 out), 'o' / 'down' (bf16 x, fp32 residual
    add), 'gu' (RMSNorm, interleaved gate/up rows, SwiGLU), 'lm' (RMSNorm, bf16 out), 'bias' (bf16 x, bias, bf16 out), 'sw'
    (first generation only: x = the gate/up vector bf16 [2K], SwiGLU applied on the fly, fp32 residual add).
    quant: the weight goes through the e4m3 row quantiser (q, s; wd = the dequantised matrix); else wd = the bf16 matrix.
    row_scales (quant only): per-row magnitudes, so that no row shares its scale with a neighbour (fp8_weight)."""

    def __init__(self, form, B, N, K, seed, quant=True, row_scales=False):
        self.form, self.B, self.N, self.K = form, B, N, K
        self.norm = form in NORM_FORMS
        self.act = form == "gu"
        if quant:
            self.q, self.s, self.wd = (dev(t) for t in fp8_weight(form, N, K, seed, row_scales))
        else:                                                    # the bf16 matrices are drawn on the device (a C3 lm_head is 233 M values)
            g = torch.Generator(device="cuda"); g.manual_seed(seed)
            w = torch.randn((N, K), generator=g, device="cuda") * K ** -0.5
            if form == "gu":
                w = interleave_gate_up(w[:N // 2].contiguous(), w[N // 2:].contiguous())
            if form == "lm":
                w = w * torch.exp(2.0 * rnd(N, seed=seed + 5)).unsqueeze(1).to(w.device)  # heavy-tailed row scales (synth.peaked_lm_head)
            self.q = self.s = None
            self.wd = w.bfloat16()
        self.bias = dev(rnd(N, seed=seed + 1, scale=0.1).bfloat16()) if form in ("qkv", "bias") else None
        self.nw = dev(1 + 0.1 * rnd(K, seed=seed + 2)) if self.norm else None
        if form == "sw":
            x = rnd(B, 2 * K, seed=seed + 3)
            x[:, 0] = -88.0                                      # gate 0 (its up value is x[:, 16]): silu's flushed-reciprocal tail
            self.x = dev(x.bfloat16())
        else:
            self.x = dev(rnd(B, K, seed=seed + 3)) if self.norm else dev(rnd(B, K, seed=seed + 3).bfloat16())
        self.res0 = dev(rnd(B, N, seed=seed + 4)) if form in RES_FORMS else None
        self.n_out = N // 2 if self.act else N

    def target(self):
        """The B output rows (bf16 sentinels, or the fp32 residual) with GUARD sentinel rows behind them (self.full)."""
        self.full = R.sentinel((self.B + GUARD, self.n_out), torch.float32 if self.res0 is not None else torch.bfloat16, "cuda")
        if self.res0 is not None:
            self.full[:self.B] = self.res0
        return self.full[:self.B]

    def guard_clean(self):
        """Nothing was stored behind the B rows (a batched kernel runs NB >= B scenes and must not store the padding ones)."""
        return not bool(guard_flags(self.full, self.B).any())

    def kw(self, tgt):
        k = dict(norm_w=self.nw, eps=EPS if self.norm else 0.0, bias=self.bias, act=self.act)
        k["res" if self.res0 is not None else "out"] = tgt
        return k

    def run(self, hip, entry, tgt=None):
        """One launch of the batched entry, B launches of a batch-1 one; returns the target (bf16 out or the fp32 residual)."""
        batched, fp8 = ENTRIES[entry]
        tgt = self.target() if tgt is None else tgt
        w = (self.q, self.s) if fp8 else (self.wd,)
        if entry == "g1":
            for b in range(self.B):
                if self.form == "gu":
                    hip.gemv_rmsnorm_swiglu_bf16(self.x[b], self.nw, EPS, self.wd, tgt[b])
                elif self.norm:
                    hip.gemv_rmsnorm_bf16(self.x[b], self.nw, EPS, self.wd, self.bias, tgt[b])
                elif self.form == "sw":
                    hip.gemv_swiglu_bf16(self.x[b], self.wd, tgt[b])
                elif self.res0 is not None:
                    hip.gemv_bf16(self.x[b], self.wd, self.bias, None, tgt[b])
                else:
                    hip.gemv_bf16(self.x[b], self.wd, self.bias, tgt[b], None)
        elif batched:
            (hip.gemv_pg_batch_fp8 if fp8 else hip.gemv_pg_batch)(self.x, *w, **self.kw(tgt))
        else:
            f = hip.gemv_pg_fp8 if fp8 else hip.gemv_pg
            for b in range(self.B):
                f(self.x[b], *w, **self.kw(tgt[b]))
        torch.cuda.synchronize()
        return tgt

    def run_fp8(self, hip, batched):
        return self.run(hip, "pgb8" if batched else "pg8")

    def run_bf16(self, hip, batched):
        return self.run(hip, "pgb" if batched else "pg")

    def activation(self, hip, entry="pg"):
        """bf16 [B, K]: what the kernel of `entry` multiplies with the weight."""
        if self.norm:
            return normalised_rows(hip, self.x, self.nw, entry)
        if self.form == "sw":
            return swiglu_rows(hip, self.x)
        return self.x

    def check(self, hip, got, entry="pg", A=None):
        A = self.activation(hip, entry) if A is None else A
        epi = G.EPI_SWIGLU if self.act else (G.EPI_RES_F32 if self.res0 is not None else G.EPI_BF16)
        return G.check_gemm(got, A, self.wd, self.bias, epi, res=self.res0)


# ------------------------------------------------------------------------------------------------ the launch table
# (entry, form, B, N, K).  B of a batch-1 entry ('pg', 'g1') = the number of activation vectors, one launch each: always 8
# (tests/test_fp8_decode_cpu.py: one vector can miss a swapped pair).  N chosen by the plan (csrc/decode_dispatch.h) so that
# every batch depth, block size, scenes-per-pass count and long-K pass count runs; test_decode_check_cpu.py confirms each with
# g2v_gemv_pg_route.
PRODUCTION = [("qkv", 2048, 1536), ("o", 1536, 1536), ("gu", 17920, 1536), ("down", 1536, 8960), ("lm", 151936, 1536)]


def _table():
    t = []
    # the five production shapes, once per entry
    t += [("pg", f, 8, N, K) for f, N, K in PRODUCTION] + [("g1", f, 8, N, K) for f, N, K in PRODUCTION]
    t += [("pgb", f, B, N, K) for (f, N, K), B in zip(PRODUCTION, (2, 4, 8, 3, 5))]
    # batch 1, plain, K = 256 (192 threads): depths 1, 2, 3, 4, 5, 6, 8 in one trip; 5 + 4, 6 + 5, 8 + 5, 8 + 8 + 3
    t += [("pg", f, 8, N, 256) for f, N in (("bias", 1), ("o", 1281), ("lm", 2049), ("bias", 2561), ("o", 3585), ("qkv", 4097),
                                            ("bias", 5121), ("o", 6401), ("qkv", 8193), ("bias", 9217), ("lm", 14337))]
    # batch 1, plain, K = 1536 (streaming: ties go to more waves): (threads, depth) = (512, 2), (384, 3), (512, 3), (512, 4),
    # (512, 5), (512, 6), (448, 8), (512, 8), (320, 5), (256, 1)
    t += [("pg", f, 8, N, 1536) for f, N in (("o", 4096), ("qkv", 4097), ("bias", 5377), ("o", 7681), ("lm", 9985), ("o", 11521),
                                             ("bias", 12289), ("qkv", 14081), ("o", 6145), ("bias", 769))]
    # batch 1, act (N = 2F, N % 32 == 0): depths 1 - 5 in one trip, then 3 + 3 | 3 + 2, 4 + 3, 5 + 4
    t += [("pg", "gu", 8, N, 256) for N in (32, 2592, 4128, 5152, 7200, 8224, 10272, 12832)]
    t += [("pg", "gu", 8, N, 1536) for N in (4096, 9248, 12832)]
    # batch 1, long K: one row per batch, one to four trips
    t += [("pg", f, 8, N, K) for K in (1544, 8960, 9216) for f, N in (("bias", 1), ("o", 769), ("down", 1793), ("bias", 2049))]
    # batched, K <= 1536: NB = 2 (B = 1, 2), 4 (B = 3, 4), 8 (B = 5, 7, 8) scenes per weight pass; every N with a bf16 and a
    # fused-norm activation
    plain = ((1, 2049), (2, 4097), (1, 6145), (2, 10241), (1, 12289), (2, 20481),
             (3, 2049), (4, 4097), (3, 6145), (4, 8193), (3, 12289),
             (5, 2049), (7, 4097), (8, 8193), (5, 1), (3, 1), (2, 1))
    for i, (B, N) in enumerate(plain):
        t += [("pgb", ("o", "bias")[i % 2], B, N, 256), ("pgb", ("qkv", "lm")[i % 2], B, N, 256)]
    # batched act: twice these plus 32
    t += [("pgb", "gu", B, N, 256) for B, N in ((1, 32), (2, 4128), (1, 8224), (2, 12320), (1, 20512), (2, 24608), (2, 40992),
                                                 (3, 32), (4, 4128), (3, 8224), (4, 12320), (3, 16416), (4, 24608),
                                                 (5, 32), (7, 4128), (8, 8224), (5, 16416))]
    # batched, long K (form 3): a block owns per = ceil(N / 256) rows (1: blocks past N idle, 2, 6: one pass, 8: 6 + 2)
    Bs = (1, 2, 3, 4, 5, 7, 8)
    for i, K in enumerate((1544, 2064, 8960, 12288)):
        t += [("pgb", f, Bs[(4 * i + j) % 7], N, K) for j, (f, N) in enumerate((("bias", 7), ("o", 300), ("down", 1536), ("o", 2000)))]
    # other K at one small N each
    for K in (8, 256, 512, 520, 1528, 1536):
        t += [("pg", "qkv", 8, 300, K), ("pg", "o", 8, 7, K), ("pg", "gu", 8, 96, K),
              ("pgb", "qkv", 3, 300, K), ("pgb", "o", 5, 7, K), ("pgb", "gu", 2, 96, K)]
    # first generation: 2 rows per block with 1, 4, 5 chunks per trip (K <= 2048, <= 8192, above; 12288 takes two trips), 8 rows
    # per block from N = 8192, the two fused inputs
    for K in (8, 256, 520, 2048, 2056, 8192, 8960, 9216, 12288):
        t += [("g1", "bias", 8, 7, K), ("g1", "o", 8, 300, K)]
    t += [("g1", "bias", 8, 8197, 256), ("g1", "qkv", 8, 7, 8), ("g1", "qkv", 8, 300, 520), ("g1", "lm", 8, 8197, 256),
          ("g1", "qkv", 8, 7, 2056), ("g1", "gu", 8, 32, 8), ("g1", "gu", 8, 96, 520), ("g1", "gu", 8, 992, 1536),
          ("g1", "sw", 8, 7, 16), ("g1", "sw", 8, 300, 528), ("g1", "sw", 8, 1536, 8960), ("g1", "sw", 8, 8197, 256)]
    assert len(set(t)) == len(t)
    return t


TABLE = _table()


# What g2v_gemv_pg_route answered for the persistent-grid rows of TABLE, in order, when the table was written: (form, threads
# per block, RB, KCH).  The GPU test asserts it for every launch, so a change of the plan shows up as a route, not as a depth
# that silently stopped running.
ROUTES = dict(zip([r for r in TABLE if r[0] in ("pg", "pgb")], (
    (1, 256, 2, 3), (1, 192, 2, 3), (1, 448, 5, 3), (1, 384, 1, 18), (1, 384, 8, 3), (2, 512, 1, 3), (2, 512, 1, 3),
    (2, 512, 2, 3), (3, 512, 6, 140), (2, 512, 2, 3), (1, 192, 1, 3), (1, 192, 2, 3), (1, 192, 3, 3), (1, 192, 4, 3),
    (1, 192, 5, 3), (1, 192, 6, 3), (1, 192, 8, 3), (1, 192, 5, 3), (1, 192, 6, 3), (1, 192, 8, 3), (1, 192, 8, 3),
    (1, 512, 2, 3), (1, 384, 3, 3), (1, 512, 3, 3), (1, 512, 4, 3), (1, 512, 5, 3), (1, 512, 6, 3), (1, 448, 8, 3),
    (1, 512, 8, 3), (1, 320, 5, 3), (1, 256, 1, 3), (1, 192, 1, 3), (1, 192, 2, 3), (1, 192, 3, 3), (1, 192, 4, 3),
    (1, 192, 5, 3), (1, 192, 3, 3), (1, 192, 4, 3), (1, 192, 5, 3), (1, 512, 1, 3), (1, 320, 4, 3), (1, 192, 5, 3),
    (1, 192, 1, 18), (1, 256, 1, 18), (1, 512, 1, 18), (1, 192, 1, 18), (1, 192, 1, 18), (1, 256, 1, 18), (1, 512, 1, 18),
    (1, 192, 1, 18), (1, 192, 1, 18), (1, 256, 1, 18), (1, 512, 1, 18), (1, 192, 1, 18), (2, 512, 2, 3), (2, 512, 2, 3),
    (2, 512, 3, 3), (2, 512, 3, 3), (2, 512, 5, 3), (2, 512, 5, 3), (2, 512, 3, 3), (2, 512, 3, 3), (2, 512, 5, 3),
    (2, 512, 5, 3), (2, 512, 5, 3), (2, 512, 5, 3), (2, 512, 2, 3), (2, 512, 2, 3), (2, 512, 3, 3), (2, 512, 3, 3),
    (2, 512, 2, 3), (2, 512, 2, 3), (2, 512, 3, 3), (2, 512, 3, 3), (2, 512, 3, 3), (2, 512, 3, 3), (2, 512, 2, 3),
    (2, 512, 2, 3), (2, 512, 2, 3), (2, 512, 2, 3), (2, 512, 2, 3), (2, 512, 2, 3), (2, 512, 1, 3), (2, 512, 1, 3),
    (2, 512, 1, 3), (2, 512, 1, 3), (2, 512, 1, 3), (2, 512, 1, 3), (2, 512, 1, 3), (2, 512, 2, 3), (2, 512, 3, 3),
    (2, 512, 5, 3), (2, 512, 3, 3), (2, 512, 5, 3), (2, 512, 5, 3), (2, 512, 1, 3), (2, 512, 2, 3), (2, 512, 3, 3),
    (2, 512, 2, 3), (2, 512, 3, 3), (2, 512, 3, 3), (2, 512, 1, 3), (2, 512, 2, 3), (2, 512, 2, 3), (2, 512, 2, 3),
    (3, 512, 6, 25), (3, 512, 6, 25), (3, 512, 6, 25), (3, 512, 6, 25), (3, 512, 6, 33), (3, 512, 6, 33), (3, 512, 6, 33),
    (3, 512, 6, 33), (3, 512, 6, 140), (3, 512, 6, 140), (3, 512, 6, 140), (3, 512, 6, 140), (3, 512, 6, 192),
    (3, 512, 6, 192), (3, 512, 6, 192), (3, 512, 6, 192), (1, 192, 1, 3), (1, 192, 1, 3), (1, 192, 1, 3), (2, 512, 1, 3),
    (2, 512, 1, 3), (2, 512, 1, 3), (1, 192, 1, 3), (1, 192, 1, 3), (1, 192, 1, 3), (2, 512, 1, 3), (2, 512, 1, 3),
    (2, 512, 1, 3), (1, 192, 1, 3), (1, 192, 1, 3), (1, 192, 1, 3), (2, 512, 1, 3), (2, 512, 1, 3), (2, 512, 1, 3),
    (1, 192, 1, 3), (1, 192, 1, 3), (1, 192, 1, 3), (2, 512, 1, 3), (2, 512, 1, 3), (2, 512, 1, 3), (1, 192, 1, 3),
    (1, 192, 1, 3), (1, 192, 1, 3), (2, 512, 1, 3), (2, 512, 1, 3), (2, 512, 1, 3), (1, 192, 1, 3), (1, 192, 1, 3),
    (1, 192, 1, 3), (2, 512, 1, 3), (2, 512, 1, 3), (2, 512, 1, 3),)))
assert len(ROUTES) == sum(r[0] in ("pg", "pgb") for r in TABLE)


# ------------------------------------------------------------------------------------------------ the e4m3 launch table
# The same for the e4m3 entries ('pg8', 'pgb8'), whose plan is not the bf16 one: depths 1, 2, 3, 4, 6, 8, 12 (SwiGLU 1, 2, 3, 4, 6;
# K > 2048: 1, 2), a batched unit is a pair of rows at depths 1, 2, 4 (NB = 8: 1, 2), the long-K batched kernel has S = ceil(K /
# 1024) waves per block and R = 8 rows per pass (NB = 8: 4).  The five production shapes are tests/test_fp8_decode_gpu.py's REAL
# and are not repeated.  Every Case of these rows is drawn with row_scales.  test_fp8_decode_check_cpu.py confirms the coverage.
def _table8():
    t = []
    # batch 1, plain, K = 256 (192 threads): depths 1, 2, 3, 4, 6, 8, 12 in one trip; 8 + 1 and 12 + 1 ragged; 8 + 8 and 12 + 12
    t += [("pg8", f, 8, N, 256) for f, N in (("bias", 1), ("o", 1281), ("lm", 2049), ("bias", 2561), ("o", 3585), ("qkv", 5121),
                                             ("bias", 6401), ("qkv", 9217), ("o", 12801), ("lm", 11521), ("bias", 17921))]
    # the other block sizes: 256, 320, 448, 512 threads at K = 256, 384 and 512 at a streaming K = 1536
    t += [("pg8", f, 8, N, 256) for f, N in (("o", 769), ("bias", 1025), ("qkv", 1537), ("o", 16129))]
    t += [("pg8", "qkv", 8, 8961, 1536), ("pg8", "o", 8, 8192, 1536)]
    # batch 1, act (N = 2F, N % 32 == 0): depths 1, 2, 3, 4, 6 in one trip; 4 + 1 and 6 + 1 ragged; 4 + 4 and 6 + 6
    t += [("pg8", "gu", 8, N, 256) for N in (32, 2592, 4128, 5152, 7200, 10272, 12832, 10784, 17952)]
    t += [("pg8", "gu", 8, N, 1536) for N in (8224, 8192)]
    # batch 1, long K (> 2048): depth 1, depth 2 in one trip, 2 + 1, 2 + 2 (at K >= 8960 the even trips start at N = 4609,
    # a weight of 41 M elements: they run at K = 2064), 384 threads
    t += [("pg8", f, 8, N, 2064) for f, N in (("bias", 1), ("o", 1281), ("down", 2049), ("bias", 2561), ("o", 300))]
    t += [("pg8", f, 8, N, 8960) for f, N in (("down", 1), ("o", 1281), ("bias", 2049))]
    t += [("pg8", f, 8, N, 9216) for f, N in (("bias", 1), ("down", 1281), ("o", 2049), ("bias", 1366))]
    # batch 1, the other K: 16 (the smallest), 512 and 1024 (the last chunk step exactly full / wholly dead), 528 and 1040 (lane 0
    # alone is live in the last step), 1536; 1552 and 2048 are short in e4m3 (two chunk steps, the second partly dead), plain only
    for K in (16, 256, 512, 528, 1024, 1040, 1536):
        t += [("pg8", "qkv", 8, 300, K), ("pg8", "o", 8, 7, K), ("pg8", "gu", 8, 96, K), ("pg8", "bias", 8, 301, K)]
    for K in (1552, 2048):
        t += [("pg8", "o", 8, 300, K), ("pg8", "bias", 8, 7, K), ("pg8", "down", 8, 1281, K)]
    # batched, K <= 1536, units = pairs of rows; every N odd (the last unit has no second row), with a bf16 and a fused-norm
    # activation.  NB = 2 (B = 1, 2) and NB = 4 (B = 3, 4): depths 1, 2, 4 in one trip, 4 + 1, 4 + 4; NB = 8 (B = 5 .. 8): depths
    # 1, 2, then 2 + 1 and 2 + 2
    plain = ((1, 1), (2, 4097), (1, 8193), (2, 16385), (1, 28673),
             (3, 1), (4, 4097), (3, 8193), (4, 16385), (3, 28673),
             (5, 1), (6, 4097), (7, 8193), (8, 12289))
    for i, (B, N) in enumerate(plain):
        t += [("pgb8", ("o", "bias")[i % 2], B, N, 256), ("pgb8", ("qkv", "lm")[i % 2], B, N, 256)]
    # the pair without a second row as the last unit of a wave in a full batch (4 of 4, 2 of 2) and in a ragged last batch (4 + 1,
    # 2 + 1); above it is the only unit of its wave (N = 1, 4097) or part of a short single batch
    t += [("pgb8", "bias", 2, 16383, 256), ("pgb8", "o", 4, 20479, 256), ("pgb8", "qkv", 8, 8191, 256), ("pgb8", "o", 7, 12287, 256),
          ("pgb8", "lm", 3, 8191, 256)]
    # batched act: the same depths and trips
    t += [("pgb8", "gu", B, N, 256) for B, N in ((1, 32), (2, 4128), (1, 8224), (2, 16416), (1, 28704),
                                                  (3, 32), (4, 4128), (3, 8224), (4, 16416), (3, 28704),
                                                  (5, 32), (6, 4128), (7, 8224), (8, 12320))]
    # batched, the other K: slot 1 (chunks 64 ..) is empty up to K = 1024, holds one live lane per half-wave at 1040, all at 1536
    for i, K in enumerate((16, 512, 528, 1024, 1040, 1536)):
        t += [("pgb8", "qkv", 1 + i, 301, K), ("pgb8", "o", 8 - i, 7, K), ("pgb8", "gu", 2 + i, 96, K)]
    # batched, long K (form 3): S = 2, 3, 6 (375 chunks in 384 slots), 9 (560 in 576), 9 (exact), 12 waves; R = 8 rows per pass
    # at NB = 2, 4 and R = 4 at NB = 8; a block owns per = 1 row (blocks past N idle), R rows, R + 1 / R + 3 rows (ragged)
    eps = ("bias", "o", "down")
    for i, K in enumerate((1552, 2064, 6000, 8960, 9216, 12288)):
        for j, N in enumerate((7, 2000, 2100)):
            t.append(("pgb8", eps[(i + j) % 3], 1 + (i + j) % 4, N, K))
        for j, N in enumerate((7, 1000, 1600)):
            t.append(("pgb8", eps[(i + j + 1) % 3], 5 + (i + j) % 4, N, K))
    assert len(set(t)) == len(t)
    return t


TABLE8 = _table8()
# What g2v_gemv_pg_route(..., fp8 = true) answered for the rows of TABLE8, in order, when the table was written: (form, threads
# per block, RB - form 3: the kernel's R -, KCH - form 3: the waves per block S).  Asserted before every launch.
ROUTES8 = dict(zip(TABLE8, (
    (1, 192, 1, 2), (1, 192, 2, 2), (1, 192, 3, 2), (1, 192, 4, 2), (1, 192, 6, 2), (1, 192, 8, 2), (1, 192, 12, 2),
    (1, 192, 8, 2), (1, 192, 12, 2), (1, 192, 8, 2), (1, 192, 12, 2), (1, 256, 1, 2), (1, 320, 1, 2), (1, 448, 1, 2),
    (1, 512, 8, 2), (1, 384, 6, 2), (1, 512, 4, 2), (1, 192, 1, 2), (1, 192, 2, 2), (1, 192, 3, 2), (1, 192, 4, 2),
    (1, 192, 6, 2), (1, 192, 4, 2), (1, 192, 6, 2), (1, 192, 4, 2), (1, 192, 6, 2), (1, 384, 3, 2), (1, 512, 2, 2),
    (1, 192, 1, 9), (1, 192, 2, 9), (1, 192, 2, 9), (1, 192, 2, 9), (1, 192, 1, 9), (1, 192, 1, 9), (1, 192, 2, 9),
    (1, 192, 2, 9), (1, 192, 1, 9), (1, 192, 2, 9), (1, 192, 2, 9), (1, 384, 1, 9), (1, 192, 1, 2), (1, 192, 1, 2),
    (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2),
    (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2),
    (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2),
    (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 1, 2),
    (1, 192, 2, 2), (1, 192, 1, 2), (1, 192, 1, 2), (1, 192, 2, 2), (2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 2, 2),
    (2, 512, 2, 2), (2, 512, 4, 2), (2, 512, 4, 2), (2, 512, 4, 2), (2, 512, 4, 2), (2, 512, 4, 2), (2, 512, 4, 2),
    (2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 2, 2), (2, 512, 2, 2), (2, 512, 4, 2), (2, 512, 4, 2), (2, 512, 4, 2),
    (2, 512, 4, 2), (2, 512, 4, 2), (2, 512, 4, 2), (2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 2, 2), (2, 512, 2, 2),
    (2, 512, 2, 2), (2, 512, 2, 2), (2, 512, 2, 2), (2, 512, 2, 2), (2, 512, 4, 2), (2, 512, 4, 2), (2, 512, 2, 2),
    (2, 512, 2, 2), (2, 512, 2, 2), (2, 512, 1, 2), (2, 512, 2, 2), (2, 512, 4, 2), (2, 512, 4, 2), (2, 512, 4, 2),
    (2, 512, 1, 2), (2, 512, 2, 2), (2, 512, 4, 2), (2, 512, 4, 2), (2, 512, 4, 2), (2, 512, 1, 2), (2, 512, 2, 2),
    (2, 512, 2, 2), (2, 512, 2, 2), (2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 1, 2),
    (2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 1, 2),
    (2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 1, 2), (3, 128, 8, 2),
    (3, 128, 8, 2), (3, 128, 8, 2), (3, 128, 4, 2), (3, 128, 4, 2), (3, 128, 4, 2), (3, 192, 8, 3), (3, 192, 8, 3),
    (3, 192, 8, 3), (3, 192, 4, 3), (3, 192, 4, 3), (3, 192, 4, 3), (3, 384, 8, 6), (3, 384, 8, 6), (3, 384, 8, 6),
    (3, 384, 4, 6), (3, 384, 4, 6), (3, 384, 4, 6), (3, 576, 8, 9), (3, 576, 8, 9), (3, 576, 8, 9), (3, 576, 4, 9),
    (3, 576, 4, 9), (3, 576, 4, 9), (3, 576, 8, 9), (3, 576, 8, 9), (3, 576, 8, 9), (3, 576, 4, 9), (3, 576, 4, 9),
    (3, 576, 4, 9), (3, 768, 8, 12), (3, 768, 8, 12), (3, 768, 8, 12), (3, 768, 4, 12), (3, 768, 4, 12), (3, 768, 4, 12),)))
assert len(ROUTES8) == len(TABLE8)


def case_id(row):
    return "-".join(str(v) for v in row)


def case_seed(row):
    entry, form, B, N, K = row
    return 1000 + 7 * sorted(ENTRIES).index(entry) + N % 97 + K % 89 + B


def route_args(row):
    """Arguments of hip.gemv_pg_route for a persistent-grid row of the table."""
    entry, form, B, N, K = row
    return (B if ENTRIES[entry][0] else 0, N, K, form == "gu", form in NORM_FORMS, ENTRIES[entry][1])


# ------------------------------------------------------------------------------------------------ attention
def attention64(q, K, V, Hkv):
    """fp64 softmax attention of one query token: q [Hq, 128], K / V [L, Hkv, 128] -> [Hq, 128]."""
    Hq = q.shape[0]
    Gq = Hq // Hkv
    out = torch.empty((Hq, 128), dtype=torch.float64)
    for h in range(Hkv):
        p = torch.softmax((q[h * Gq:(h + 1) * Gq].double() @ K[:, h].double().T) * 128 ** -0.5, dim=-1)
        out[h * Gq:(h + 1) * Gq] = p @ V[:, h].double()
    return out


def row_metrics(got, want):
    """(rel-L2 over the slot, worst element error in units of its head row's rms) of got [Hq, 128] against fp64 want."""
    got, want = got.detach().cpu().double(), want.double()
    r = float((got - want).norm() / want.norm().clamp_min(1e-30))
    e = float(((got - want).abs() / want.pow(2).mean(dim=1, keepdim=True).sqrt()).max())
    return r, e
