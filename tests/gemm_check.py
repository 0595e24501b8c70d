"""fp64 reference and element-wise check for the bf16 GEMM family (csrc/gemm*.hip) and gemm_f32.

A helper module (pytest does not collect it): test_gemm_check_cpu.py tests the check itself without a GPU, and
test_gemm_fp64_gpu.py applies it to every kernel form.

Reference.  v* = A.W^T + b and T = |A|.|W|^T + |b|, in float64 on the exact bf16 operands the kernel reads, row chunk by
row chunk (a C3 gate/up output is 1.6 GB in fp64).

Admissible Linear values.  delta = TAU * T.  Every bf16 value between RN(v* - delta) and RN(v* + delta) is admissible, RN =
fp64 -> fp32 -> bf16 with round-to-nearest-even at both steps.  The fp32 accumulation error of the summation orders these
kernels use (32-deep MFMA dot products, K-tiles and split-K partials in slice order) is typically ~2^-24 T, so TAU = 2^-16
leaves 2^8 of headroom; it stays far below one bf16 ulp of a typical |v*| (T / |v*| ~ 0.64 sqrt(K)), so a dropped or
misplaced product term moves most outputs by one ulp or more.  Usually one value is admissible; near a rounding boundary
two, with cancellation a few more.

Epilogues, evaluated at the admissible values with the rounding points the kernels document (bfround, __fmul_rn, __fadd_rn,
f2bf):
  * EPI_BF16, RES_F32 (gamma with or without GAMMA_ROUND_BF16, with or without residual), RES_BF16 are exact in IEEE fp32
    and emulated with separate torch float32 ops.  With one or two candidates the output must equal the emulated value of
    one of them; with more it must lie between the values at the two ends (each of these maps is monotone).
  * GELU, QuickGELU, SwiGLU carry transcendentals (erfc-fit GELU, device sigmoid, rcp-SiLU).  The output must lie within
    ULP_BOUND[epi] bf16 ulps of the fp64 function - applied with the kernel's intermediate bf16 roundings - over the
    admissible values (both ends and the function's interior extremum, clamped into the interval; for SwiGLU gate and up
    each over their own interval), plus an absolute floor for near-zero outputs: 2^-22 T for GELU / QuickGELU (the
    reference's own 1 + erf cancellation is |x| 2^-24), 2^-30 T_gate T_up for SwiGLU.
  * For EPI_BF16 outputs d = distance from v* to the rounding interval of the returned value / T is recorded; d <= TAU
    is what the check asserts there, and the largest d is reported.

The result is a boolean map of flagged elements; a case passes with zero flags, no fraction allowance.
"""
import math

import torch

TAU = 2.0 ** -16
EPI_BF16, EPI_GELU, EPI_QUICKGELU, EPI_SWIGLU, EPI_RES_F32, EPI_RES_BF16 = range(6)
EPI_NAMES = {EPI_BF16: "bf16", EPI_GELU: "gelu", EPI_QUICKGELU: "quickgelu", EPI_SWIGLU: "swiglu", EPI_RES_F32: "res_f32",
             EPI_RES_BF16: "res_bf16"}
# bf16 ulps allowed for the activation epilogues: 1.5 x the largest measured on an MI355X, never above 2 (test_gemm_fp64_gpu.py)
ULP_BOUND = {EPI_GELU: 0.75, EPI_QUICKGELU: 2.0, EPI_SWIGLU: 2.0}
NAN_BF16 = 0x7FA5                     # sentinel: bf16 NaN with a payload no kernel writes
NAN_F32 = 0x7FA5A5A5                  # its fp32 counterpart
GELU_XMIN = -0.7517915246935645       # argmin of x Phi(x)
SILU_XMIN = -1.2784645427610738       # argmin of x sigmoid(x)
QGELU_XMIN = SILU_XMIN / 1.702        # argmin of x sigmoid(1.702 x)
_TINY = 2.0 ** -100


def key(x):
    """bf16 -> int32, monotone in the value (+0 and -0 share 0): adjacent bf16 values have adjacent keys."""
    b = x.contiguous().view(torch.int16).to(torch.int32)
    m = b & 0x7FFF
    return torch.where(b < 0, -m, m)


def from_key(k):
    b = torch.where(k < 0, (-k) | 0x8000, k)
    b = torch.where(b >= 0x8000, b - 0x10000, b)
    return b.to(torch.int16).view(torch.bfloat16)


def rn(x):
    """fp64 -> fp32 -> bf16, round to nearest even at both steps."""
    return x.float().bfloat16()


def ulp_bf16(y):
    """One bf16 ulp at |y| (fp64)."""
    _, e = torch.frexp(y.abs().clamp_min(_TINY))
    return torch.pow(2.0, (e - 8).double())


def linear64(A, W, bias=None):
    """(v*, T) of a bf16 Linear in float64 on A's device: v* = A.W^T + b, T = |A|.|W|^T + |b|."""
    a, w = A.double(), W.double()
    v, T = a @ w.T, a.abs() @ w.abs().T
    if bias is not None:
        b = bias.double()
        v, T = v + b, T + b.abs()
    return v, T


def admissible(v, T, tau=TAU):
    """(lowest, highest admissible bf16 Linear value, number of admissible values)."""
    d = tau * T
    lo, hi = rn(v - d), rn(v + d)
    return lo, hi, key(hi) - key(lo) + 1


# ---------------------------------------------------------------------------------------- epilogue emulations
def res_f32(v, res, gamma, round_gamma):
    """out(f32) = res + [bf16](v * gamma): __fmul_rn, optional bfround, __fadd_rn (separate fp32 ops, no contraction)."""
    t = v.float()
    if gamma is not None:
        t = t * gamma.float()
        if round_gamma:
            t = t.bfloat16().float()
    r = res.float() if res is not None else torch.zeros_like(t)
    return r + t


def res_bf16(v, res):
    return (res.float() + v.float()).bfloat16()


def gelu64(x):
    return 0.5 * x * (1.0 + torch.special.erf(x * (1.0 / math.sqrt(2.0))))


def quickgelu64(v):
    """v * bf16(sigmoid(bf16(1.702 v))) in fp64 with the kernel's two intermediate roundings (its fp32 product 1.702f * v is
    reproduced exactly)."""
    u = (v.float() * 1.702).bfloat16().double()
    return v * rn(torch.sigmoid(u)).double()


def silu_r64(g):
    """bf16(silu(g)) from the fp64 function."""
    return rn(g * torch.sigmoid(g)).double()


def _range3(f, lo, hi, xe):
    ys = torch.stack([f(lo), f(hi), f(torch.minimum(torch.maximum(torch.full_like(lo, xe), lo), hi))])
    return ys.min(0).values, ys.max(0).values


# ----------------------------------------------------------------------------------------------- the check
class Check:
    """Flag map and statistics of one checked output (accumulated over row chunks)."""

    def __init__(self, rows, cols, device, epi):
        self.bad = torch.zeros((rows, cols), dtype=torch.bool, device=device)
        self.epi = epi
        self.n = rows * cols
        self.multi = 0              # elements with more than one admissible Linear value (SwiGLU: gate or up)
        self.max_d = 0.0            # EPI_BF16: largest implied accumulation error / T
        self.max_ulps = 0.0         # activations: largest distance to the fp64 range in bf16 ulps (beyond the floor)

    @property
    def count(self):
        return int(self.bad.sum())

    def first(self):
        idx = self.bad.nonzero()
        return None if idx.numel() == 0 else (int(idx[0, 0]), int(idx[0, 1]))

    def flagged_rows(self):
        return sorted(set(self.bad.any(1).nonzero().flatten().tolist()))

    def report(self, tile=None, what=""):
        f = self.first()
        if f is None:
            return f"{what}: 0 flagged of {self.n}"
        r, c = f
        s = f"{what}: {self.count} of {self.n} elements flagged; first at row {r} col {c}, fragment ({r // 16}, {c // 16})"
        if tile is not None:
            s += f", tile ({r // tile[0]}, {c // tile[1]}) of {tile[0]}x{tile[1]}"
        return s


def check_gemm(got, A, W, bias=None, epi=EPI_BF16, res=None, gamma=None, round_gamma=False, tau=TAU, ulps=None,
               chunk_rows=None):
    """Element-wise check of one group's output `got` [M, N] ([M, N/2] for SwiGLU; bf16, fp32 for RES_F32) of
    epi(A[M, K] . W[N, K]^T + bias).  res = the residual as it was BEFORE the launch (in-place launches overwrite it),
    gamma fp32 [N].  Returns a Check; the caller asserts check.count == 0."""
    M = A.shape[0]
    N = W.shape[0]
    n_out = N // 2 if epi == EPI_SWIGLU else N
    assert got.shape == (M, n_out), (got.shape, M, n_out)
    dev = got.device
    chk = Check(M, n_out, dev, epi)
    if M == 0:
        return chk
    U = (ulps if ulps is not None else ULP_BOUND.get(epi, 0.0))
    W = W.to(dev)
    bias = bias.to(dev) if bias is not None else None
    gam = gamma.to(dev).float() if gamma is not None else None
    if epi == EPI_SWIGLU:
        j = torch.arange(n_out, device=dev)
        gate_cols = 32 * (j // 16) + j % 16
    step = chunk_rows or max(1, (1 << 24) // max(N, 1))
    for r0 in range(0, M, step):
        r1 = min(M, r0 + step)
        v, T = linear64(A[r0:r1].to(dev), W, bias)
        g = got[r0:r1]
        finite = torch.isfinite(g.float())
        if epi == EPI_SWIGLU:
            vg, Tg = v[:, gate_cols], T[:, gate_cols]
            vu, Tu = v[:, gate_cols + 16], T[:, gate_cols + 16]
            glo, ghi, gn = admissible(vg, Tg, tau)
            ulo, uhi, un = admissible(vu, Tu, tau)
            chk.multi += int(((gn > 1) | (un > 1)).sum())
            smin, smax = _range3(silu_r64, glo.double(), ghi.double(), SILU_XMIN)
            ul, uh = ulo.double(), uhi.double()
            corners = torch.stack([smin * ul, smin * uh, smax * ul, smax * uh])
            ymin, ymax = corners.min(0).values, corners.max(0).values
            floor = 2.0 ** -30 * Tg * Tu
            bad = _activation_bad(chk, g, ymin, ymax, floor, U)
        else:
            lo, hi, nc = admissible(v, T, tau)
            chk.multi += int((nc > 1).sum())
            if epi in (EPI_GELU, EPI_QUICKGELU):
                f, xe = (gelu64, GELU_XMIN) if epi == EPI_GELU else (quickgelu64, QGELU_XMIN)
                ymin, ymax = _range3(f, lo.double(), hi.double(), xe)
                bad = _activation_bad(chk, g, ymin, ymax, 2.0 ** -22 * T, U)
            else:
                if epi == EPI_BF16:
                    flo, fhi = lo, hi
                elif epi == EPI_RES_BF16:
                    rr = res[r0:r1].to(dev)
                    flo, fhi = res_bf16(lo, rr), res_bf16(hi, rr)
                elif epi == EPI_RES_F32:
                    rr = res[r0:r1].to(dev) if res is not None else None
                    flo, fhi = res_f32(lo, rr, gam, round_gamma), res_f32(hi, rr, gam, round_gamma)
                else:
                    raise ValueError(epi)
                gf, flo, fhi = g.float(), flo.float(), fhi.float()
                lo_v, hi_v = torch.minimum(flo, fhi), torch.maximum(flo, fhi)
                ok = torch.where(nc <= 2, (gf == flo) | (gf == fhi), (gf >= lo_v) & (gf <= hi_v))
                bad = ~ok
                if epi == EPI_BF16:
                    k = key(g)
                    gd = g.double()
                    e_lo = (gd + from_key(k - 1).double()) / 2
                    e_hi = (gd + from_key(k + 1).double()) / 2
                    d = (torch.clamp_min(e_lo - v, 0) + torch.clamp_min(v - e_hi, 0)) / T.clamp_min(_TINY)
                    d = torch.where(finite, d, torch.zeros_like(d))
                    chk.max_d = max(chk.max_d, float(d.max()))
                    bad = bad | (d > tau)
        chk.bad[r0:r1] = bad | ~finite
    return chk


def _activation_bad(chk, g, ymin, ymax, floor, U):
    gd = g.double()
    err = torch.clamp_min(ymin - gd, 0) + torch.clamp_min(gd - ymax, 0)
    near = torch.minimum(torch.maximum(gd, ymin), ymax)
    ul = torch.clamp_min(err - floor, 0) / ulp_bf16(near)
    ul = torch.where(torch.isfinite(ul), ul, torch.full_like(ul, float("inf")))
    fin = torch.isfinite(g.float())
    if bool(fin.any()):
        chk.max_ulps = max(chk.max_ulps, float(ul[fin].max()))
    return ul > U


# --------------------------------------------------------------------------------------------------- gemm_f32
def check_f32(got, A, W, bias=None, relu=False, res=None, c=1.0):
    """gemm_f32 (a k-ordered fp32 fma chain): |got - ref| <= c K 2^-24 (S + |b|) + 2^-24 |ref| per element, the last term
    for the rounding of the final residual add (and of the bias add).  Returns (flag map, largest error / (K 2^-24 T))."""
    K = A.shape[1]
    v, T = linear64(A, W, bias)
    if relu:
        v = torch.clamp_min(v, 0)
    if res is not None:
        v = v + res.double()
    u = 2.0 ** -24
    err = (got.double() - v).abs()
    bound = c * K * u * T + 2 * u * v.abs() + _TINY
    bad = ~(err <= bound)
    ratio = float((err / (K * u * T).clamp_min(_TINY)).max())
    return bad, ratio
