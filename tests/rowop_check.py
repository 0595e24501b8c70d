"""fp64 references and element-wise checks for the row kernels between one GEMM and the next attention or GEMM:
csrc/norm_rope.hip (layernorm, rmsnorm, mrope_table, qknorm_mrope_cache, rope2d, rope_vision) and the fp32 row movers and the
two casts of csrc/misc.hip.

A helper module (pytest does not collect it): test_rowop_check_cpu.py tests the checks themselves without a GPU, and
test_rowops_fp64_gpu.py applies them to every launch form.  key / from_key / rn / ulp_bf16 / admissible and the NaN
sentinels are gemm_check.py's.

References are float64 on the exact operands the kernel reads (the bf16 or fp32 bits of x, the fp32 weights and tables, eps
as the fp32 value the C entry point receives).  A check returns a boolean map of flagged elements; a case passes with zero
flags, no fraction allowance.

TAU = 2^-19, derived, not measured.  The longest fp32 path to an output is the MAXV = 8 norm: 11 roundings in the per-lane
sum, 6 xor-shuffle adds, 4 for divide / + eps / sqrt / reciprocal, 2 - 3 multiplies, each at most 2^-24 relative, the sum's
share halved by the square root: under 2^-20 of the magnitude term T below; TAU leaves a factor 2.  It stays far below one
bf16 ulp (2^-8 relative), so one wrong term (a lane missing from the sum, another row's weight, a dropped eps, another axis'
angle) moves an output by an ulp or more.

  RMSNorm    y* = w x (mean(x^2) + eps)^-1/2, w by row < split;  T = |y*|
  LayerNorm  y* = (x - mu) r w + b;  T = (|x - mu| + mean|x|) r |w| + |b|   (mean|x| pays for the rounding of mu)
  fp32 output: flag |got - y*| > TAU T.   bf16 output: flag anything outside admissible(y*, T, TAU).
  An all-zero row has T = 0 (RMSNorm) or T = |b| with y* = b (LayerNorm): the output must be exactly 0, exactly b.

qk-norm + mRoPE + cache write.  n* = x r over the 128 dims of a head.  und_rounding = 0: n = n*.  und_rounding = 1: the
kernel rounds n to bf16, so the check carries the interval [RN(n* - TAU |n*|), RN(n* + TAU |n*|)] of admissible bf16 values
(usually one, sometimes two).  The output is linear in the pair (n[d], n[d +- 64]): o* = n w cos + rotate_half(n w) sin is
evaluated at the interval ends, widened by TAU (|n w cos| + |rotate_half(n w) sin|), and `got` must be a bf16 rounding of
that interval.  V rows are copied bit for bit; every cache row not named in kv_rows keeps the bits it had.  The check is a
condition, not a measurement: it reports the share of elements with more than one admissible value and the caller fails a
case whose share exceeds MULTI_CAP = 2 %.

mRoPE table.  f = float(pos) * inv_freq is one IEEE fp32 multiply (reproduced with torch fp32); the reference is cos / sin
in float64 of that fp32 f, the axis of dim d (and d + 64) is t for d < 16, h for d < 40, w otherwise; the d and d + 64 copies
must be bit-equal.  The bound on |got - ref| is the caller's (it depends on the device's cosf / sinf).

Exact ops.  rope_vision is two __fmul_rn and one __fadd_rn per output and one bf16 rounding: emulated with separate torch
fp32 ops, compared with torch.equal.  The casts and the row movers are bit-exact; cast_table() holds the fp32 values at
which a bf16 conversion goes wrong (NaN, +-inf, +-0, subnormals, both tie directions, the bf16 overflow threshold).

Measured on the CPU (test_rowop_check_cpu.py prints them; fp32 emulations of the kernels in their own summation order, over
the input families `3 randn + 0.5`, `100 + randn`, `1e-3 randn`, `1e4 randn`, an all-zero row, C in {4, 160, 516, 1280, 1536,
2048}):
  largest error / (TAU T): LayerNorm 0.103 (fp32 out; 0.056 implied by a bf16 out), RMSNorm 0.114 (0.045), qk-norm + mRoPE
  0.024 (und_rounding 0), 0.0036 (1); asserted < 0.25.
  largest share of bf16 outputs with more than one admissible value in a case of 1000 elements or more: RMSNorm 0.26 %
  (0.10 - 0.26 % per family), LayerNorm 0.72 % (plain 0.63, tiny 0.72, huge 0.56, the zero row 0.16 %) on every family but
  the offset rows (`100 + randn`: T carries mean|x| ~ 100 sigma, measured up to 24 % at TAU; those rows are checked in the
  fp32-output form, and their bf16 form is exempt from the cap); qk-norm + mRoPE 0.27 % (und_rounding 0), 0.37 % (1).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_check import NAN_BF16, NAN_F32, admissible, from_key, key, rn, ulp_bf16  # noqa: E402,F401

TAU = 2.0 ** -19
MULTI_CAP = 0.02
_TINY = 2.0 ** -200


def f32(v):
    """A Python float as the fp32 value a C `float` argument carries."""
    return float(torch.tensor(v, dtype=torch.float32))


def maxv(C):
    """float4 groups per lane of the norm kernels' launch form for a row of C (g2v_layernorm / g2v_rmsnorm dispatch)."""
    return 2 if C <= 512 else 4 if C <= 1024 else 6 if C <= 1536 else 8


def bits(t):
    """The raw bits of a bf16 / fp32 tensor as int16 / int32 (so that NaNs compare)."""
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def sentinel(shape, dtype, device="cpu"):
    t = torch.empty(shape, dtype=dtype, device=device)
    bits(t).fill_(NAN_BF16 if dtype == torch.bfloat16 else NAN_F32)
    return t


def is_sentinel(t):
    """Boolean map: the element still holds the sentinel's bits."""
    return bits(t) == (NAN_BF16 if t.dtype == torch.bfloat16 else NAN_F32)


class Result:
    """Flag map and statistics of one checked output."""

    def __init__(self, bad, multi=0, max_ratio=0.0):
        self.bad = bad
        self.n = bad.numel()
        self.multi = int(multi)             # elements with more than one admissible bf16 value
        self.max_ratio = float(max_ratio)   # largest implied error / (TAU T)

    @property
    def count(self):
        return int(self.bad.sum())

    @property
    def multi_share(self):
        return self.multi / max(self.n, 1)

    def where(self):
        return [tuple(i) for i in self.bad.nonzero().tolist()]

    def flagged_rows(self):
        return sorted(set(self.bad.reshape(self.bad.shape[0], -1).any(1).nonzero().flatten().tolist()))

    def report(self, what=""):
        w = self.where()
        if not w:
            return f"{what}: 0 flagged of {self.n}"
        return f"{what}: {len(w)} of {self.n} elements flagged; first at {w[0]}"


# ---------------------------------------------------------------------------------------------------- norms
def rmsnorm64(x, w_lo, w_hi, split, eps):
    """(y*, T) of the routed RMSNorm: rows [0, split) take w_lo, the rest w_hi."""
    xd = x.detach().cpu().double()
    r = (xd.pow(2).mean(-1, keepdim=True) + f32(eps)).rsqrt()
    lo = (torch.arange(xd.shape[0]) < split)[:, None]
    w = torch.where(lo, w_lo.cpu().double()[None], w_hi.cpu().double()[None])
    y = w * xd * r
    return y, y.abs()


def layernorm64(x, w, b, eps):
    xd = x.detach().cpu().double()
    xc = xd - xd.mean(-1, keepdim=True)
    r = (xc.pow(2).mean(-1, keepdim=True) + f32(eps)).rsqrt()
    wd, bd = w.cpu().double(), b.cpu().double()
    y = xc * r * wd + bd
    T = (xc.abs() + xd.abs().mean(-1, keepdim=True)) * r * wd.abs() + bd.abs()
    return y, T


def _bf16_gap(got, lo, hi):
    """Distance (fp64, >= 0) from the interval [lo, hi] to the set of reals that round to the bf16 `got`."""
    k = key(got)
    gd = got.double()
    e_lo = (gd + from_key(k - 1).double()) / 2
    e_hi = (gd + from_key(k + 1).double()) / 2
    return torch.clamp_min(e_lo - hi, 0) + torch.clamp_min(lo - e_hi, 0)


def check_out(got, y, T, tau=TAU):
    """fp32 `got`: flag |got - y*| > tau T.  bf16 `got`: flag anything outside admissible(y*, T, tau)."""
    got = got.detach().cpu()
    assert got.shape == y.shape, (got.shape, y.shape)
    bound = tau * T
    finite = torch.isfinite(got.float())
    if got.dtype == torch.float32:
        err = (got.double() - y).abs()
        bad = ~(err <= bound)
        multi = 0
    else:
        assert got.dtype == torch.bfloat16
        lo, hi, n = admissible(y, T, tau)
        k = key(got)
        bad = (k < key(lo)) | (k > key(hi)) | ~finite
        multi = (n > 1).sum()
        err = _bf16_gap(got, y, y)
    ratio = torch.where(finite & (bound > 0), err / bound.clamp_min(_TINY), torch.zeros_like(err))
    return Result(bad, multi, ratio.max() if ratio.numel() else 0.0)


# ------------------------------------------------------------------------------ qk-norm + mRoPE + cache write
def _qk_interval(x, w, eps, und, cos, sin, tau):
    """x [L, H, 128] (bf16 bits), w [L, 1, 128] fp32, cos / sin [L, 128] fp32 -> (omin, omax, widening) in fp64."""
    xd = x.double()
    r = (xd.pow(2).mean(-1, keepdim=True) + f32(eps)).rsqrt()
    ns = xd * r
    if und:
        d = tau * ns.abs()
        nlo, nhi = rn(ns - d).double(), rn(ns + d).double()
    else:
        nlo = nhi = ns
    wd = w.double()
    a, b = nlo * wd, nhi * wd
    mlo, mhi = torch.minimum(a, b), torch.maximum(a, b)
    rlo = torch.cat([-mhi[..., 64:], mlo[..., :64]], -1)          # rotate_half = (-x2, x1)
    rhi = torch.cat([-mlo[..., 64:], mhi[..., :64]], -1)
    c, s = cos.double()[:, None, :], sin.double()[:, None, :]
    t1 = torch.stack([mlo * c, mhi * c])
    t2 = torch.stack([rlo * s, rhi * s])
    omin = t1.min(0).values + t2.min(0).values
    omax = t1.max(0).values + t2.max(0).values
    wid = tau * (t1.abs().max(0).values + t2.abs().max(0).values)
    return omin, omax, wid


def _check_interval(got, omin, omax, wid):
    lo, hi = rn(omin - wid), rn(omax + wid)
    k = key(got)
    finite = torch.isfinite(got.float())
    bad = (k < key(lo)) | (k > key(hi)) | ~finite
    gap = _bf16_gap(got, omin, omax)
    ratio = torch.where(finite & (wid > 0), gap / wid.clamp_min(_TINY), torch.zeros_like(gap))
    return bad, int((key(hi) > key(lo)).sum()), float(ratio.max()) if ratio.numel() else 0.0


class QKResult:
    """q: Result over q_out [L, Hq, 128]; k, v: Results over the whole caches [R, Hkv, 128] (rows not named in kv_rows are
    flagged when their bits changed)."""

    def __init__(self, q, k, v, n_rot):
        self.q, self.k, self.v = q, k, v
        self.count = q.count + k.count + v.count
        self.multi_share = (q.multi + k.multi) / max(n_rot, 1)
        self.max_ratio = max(q.max_ratio, k.max_ratio)

    def report(self, what=""):
        return "; ".join([self.q.report(what + " q_out"), self.k.report(what + " k_cache"), self.v.report(what + " v_cache")])


def check_qknorm_mrope_cache(qkv, Hq, Hkv, qw_lo, qw_hi, kw_lo, kw_hi, split, eps, und, cos, sin, kv_rows, q_out, k_before,
                             k_after, v_before, v_after, tau=TAU):
    """qkv bf16 [L, (Hq + 2 Hkv) 128]; the caches [R, Hkv, 128] as they were before and are after the launch."""
    cpu = lambda t: t.detach().cpu()
    qkv, cos, sin, q_out = cpu(qkv), cpu(cos), cpu(sin), cpu(q_out)
    k_before, k_after, v_before, v_after = cpu(k_before), cpu(k_after), cpu(v_before), cpu(v_after)
    rows = cpu(kv_rows).long()
    L = qkv.shape[0]
    x = qkv.view(L, Hq + 2 * Hkv, 128)
    lo = (torch.arange(L) < split)[:, None, None]
    qw = torch.where(lo, cpu(qw_lo).float()[None, None], cpu(qw_hi).float()[None, None])
    kw = torch.where(lo, cpu(kw_lo).float()[None, None], cpu(kw_hi).float()[None, None])
    bq, mq, rq = _check_interval(q_out.view(L, Hq, 128), *_qk_interval(x[:, :Hq], qw, eps, und, cos, sin, tau))
    written = torch.zeros(k_after.shape[0], dtype=torch.bool)
    written[rows] = True
    assert int(written.sum()) == L, "kv_rows must name distinct cache rows"
    bk = bits(k_after) != bits(k_before)                              # rows not named: any changed bit is a flag
    b, mk, rk = _check_interval(k_after[rows], *_qk_interval(x[:, Hq:Hq + Hkv], kw, eps, und, cos, sin, tau))
    bk[rows] = b
    want_v = v_before.clone()
    want_v[rows] = x[:, Hq + Hkv:]
    bv = bits(v_after) != bits(want_v)
    return QKResult(Result(bq, mq, rq), Result(bk, mk, rk), Result(bv), L * (Hq + Hkv) * 128)


# ------------------------------------------------------------------------------------------------ mRoPE table
def mrope_axis():
    d = torch.arange(64)
    return torch.where(d < 16, 0, torch.where(d < 40, 1, 2))


def mrope_table64(pos, inv_freq):
    """pos int [3, L], inv_freq fp32 [64] -> cos, sin float64 [L, 128] of the fp32 argument float(pos) * inv_freq."""
    p = pos.cpu().long()[mrope_axis(), :].T                           # [L, 64]
    f = p.to(torch.float32) * inv_freq.cpu().float()[None]            # one IEEE fp32 multiply
    fd = f.double()
    return torch.cat([fd.cos(), fd.cos()], -1), torch.cat([fd.sin(), fd.sin()], -1)


def check_mrope_table(cs, sn, pos, inv_freq, bound):
    """Returns (flag map [L, 128] over cos or sin, largest |got - ref|).  Flags: error above `bound`, a non-finite value, or
    a d + 64 copy that is not bit-equal to d."""
    cs, sn = cs.detach().cpu(), sn.detach().cpu()
    rc, rs = mrope_table64(pos, inv_freq)
    ec, es = (cs.double() - rc).abs(), (sn.double() - rs).abs()
    bad = ~(ec <= bound) | ~(es <= bound)
    twin = (bits(cs[:, :64]) != bits(cs[:, 64:])) | (bits(sn[:, :64]) != bits(sn[:, 64:]))
    bad = bad | torch.cat([twin, twin], -1)
    err = torch.maximum(ec, es)
    err = torch.where(torch.isfinite(err), err, torch.zeros_like(err))
    return bad, float(err.max()) if err.numel() else 0.0


# -------------------------------------------------------------------------------------------------- exact ops
def rope_vision_emul(x, n_heads, D, cos, sin):
    """x bf16 [L, ld]: columns [0, n_heads D) rotated (fp32: two multiplies, one add, one bf16 rounding), the rest kept."""
    x, cos, sin = x.detach().cpu(), cos.detach().cpu().float(), sin.detach().cpu().float()
    L = x.shape[0]
    t = x[:, :n_heads * D].reshape(L, n_heads, D).float()
    h = D // 2
    rot = torch.cat([-t[..., h:], t[..., :h]], -1)
    a = t * cos[:, None, :]
    b = rot * sin[:, None, :]
    out = x.clone()
    out[:, :n_heads * D] = (a + b).bfloat16().reshape(L, n_heads * D)
    return out


def cast_table():
    """fp32 values at which an fp32 -> bf16 conversion goes wrong, as int32 bit patterns viewed as fp32 (a multiple of 4)."""
    pats = [0x7FC00000, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000,            # NaN, +-inf, +-0
            0x00000001, 0x007FFFFF, 0x80000001, 0x00400000, 0x00008000, 0x00018000, 0x807FFFFF,   # subnormals (and ties among them)
            0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,                        # ties: to even downwards, upwards
            0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,                        # one fp32 ulp either side of a tie
            0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F7FFF, 0xFF7F8000, 0xFF7FFFFF,  # last to round to bf16 max, first to inf
            0x7F7F0000, 0x00800000]                                                # bf16 max itself, smallest normal
    assert len(pats) % 4 == 0
    t = torch.tensor([p - (1 << 32) if p >= (1 << 31) else p for p in pats], dtype=torch.int64).to(torch.int32)
    return t.view(torch.float32)


def cast_nan_table():
    """NaNs whose payload sits in the 16 bits a truncating conversion drops, or that carry a sign: the result must be a NaN."""
    pats = [0x7F800001, 0x7F80FFFF, 0xFF800001, 0xFFC00000, 0x7FFFFFFF, 0x7FA5A5A5, 0x7F808000, 0xFFFFFFFF]
    t = torch.tensor([p - (1 << 32) if p >= (1 << 31) else p for p in pats], dtype=torch.int64).to(torch.int32)
    return t.view(torch.float32)
