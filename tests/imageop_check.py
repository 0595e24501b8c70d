"""fp64 references, exact index restatements and element-wise checks for the pixel-side kernels and the token pickers:
csrc/misc.hip (argmax / Gumbel-max sampler, camera_tail, pts_epilogue, pixel_shuffle, im2col14, dino_assemble) and
swiglu_bf16 of csrc/decode.hip.

A helper module (pytest does not collect it): test_imageop_check_cpu.py tests the checks themselves without a GPU, on fp32
emulations of the kernels in the kernels' own summation order and on injected faults; test_imageops_fp64_gpu.py applies them
to every launch form.  key / rn / admissible and the NaN sentinels are gemm_check.py's; bits / sentinel / is_sentinel /
Result / cast_table / MULTI_CAP are rowop_check.py's.  A check returns a flag map; a case passes with zero flags.
u = 2^-24 throughout.

A. Token pickers.  Reference: torch.argmax of the fp32 values on the CPU - the first maximal index wins, any NaN beats every
number (+inf included) and the first NaN wins, a row of all -inf gives 0, -0.0 == +0.0.  argmax_cases(n) builds the rows:
the unique maximum and pairs of equal maxima on every boundary of the launch (0, n - 1, the wave boundary 63|64, the
256-thread stride 255|256, and with 64 workgroups (n >= 65536) k per - 1 | k per for k = 1, 32, 63, per = ceil(n / 64)), on a
non-increasing and on a constant row; +-0; all -inf; +inf and NaN in both orders in one thread (i, i + 256), in two waves, in
two workgroups; two NaNs.  argmax_emul restates the kernel's merge tree (thread, wave, workgroup, grid) over an ordered
integer key with NaN on top; with nan_as_inf = True it restates the rule the kernel had before (NaN merged as +inf), which
the inf-before-NaN rows must flag.  The sampler's Philox4x32-10 stream and Gumbel scores are restated in float64
(philox_first, gumbel_scores); its criterion is the older test's: the drawn index's score is >= max - 1e-4 max(1, |max|).

B. Camera tail.  B1 (mean -> two 512-wide ReLU layers -> a 3- or 9-row Linear): every stage in fp64 on the fp32 operands,
with a first-order running bound in fp64: mean e = (ceil(P / 4) + 3) u mean|f| (the adds of one of the four partial sums, its
tail, the two combining adds, the divide); each matvec e_out = |W| e_in + 15 u (|W| |v*| + |b|) (8 fma, 6 shuffle adds, the
bias add); ReLU is 1-Lipschitz.  Flag |got - ref| > 2 e (the 2 pays for second-order terms).  The kernel's own nine
pre-SVD values are read back through the translation column (wt, bt = three rows of wr, br: matvec512's arithmetic does not
depend on which call it serves).
B2 (rotation).  Reference: the fp64 nearest rotation U diag(1, 1, det(U V^T)) V^T of A = the row-normalised m9, A = U S V^T
by numpy.linalg.svd.  Bound (28 / gap + 2) u per element, gap = s2 + s3 (det > 0) or s2 - s3 (det < 0): the polar factor's
perturbation bound |dR|_F <= 2 |dA|_F / gap, the fp32 row normalisation gives |dA| <= 4u per element = 7u in Frobenius norm
(14u / gap), times the same factor 2; the double-precision Jacobi is negligible, the final cast costs u / 2.  Callers
assert gap >= 1 / 8 on the reference before launching.  Always: |R^T R - I| <= 8u, |det R - 1| <= 8u, row 3 == [0, 0, 0, 1].
Rank-deficient inputs (a zero row, s2 = s3 = 0 ...) are out of scope: the reference itself is not unique there.

C. Point head tail.  shuffle_map restates out[n, y, x, c] = feat[n P + py gw + px, c PS^2 + iy PS + ix]; with features coded
feat[r, k] = r K + k (exact in fp32) mode 0 and pixel_shuffle must equal the map exactly and a wrong pixel names the element
it read.  Mode 1 against z* = exp(c), local = (a z*, b z*, z*), world = T[:3, :3] local + T[:3, 3] in fp64:
  |z - z*| <= max(2^-21 z*, 2^-126)   (8u: OpenCL's 3-ulp expf limit plus one rounding; the floor allows a flushed subnormal)
  |lx - a z*| <= 9u |a| z*, likewise ly
  |world_r - ref| <= sum_j |T_rj| e_j + 4u (sum_j |T_rj| |p_j| + |T_r3|)
Where z* exceeds the fp32 range z must be +inf and lx, ly, world what fp32 ops give from that z (inf, or NaN where a = 0).
The relative lx / ly bound cannot hold where z* is below the fp32 normal range (one subnormal ulp is a large fraction of z*),
so pts_inputs plants c = -100 and -87.5 on pixels with a = b = 0 (lx = ly = 0 exactly there; z and world carry the floor);
c = 88 sits on a pixel with a = b = 1/4 so that world stays inside the fp32 range, c = 89 on one pixel with a = 0 and one not.

D. DINO front end, exact.  im2col14: out[n P + py gw + px, c 196 + ky 14 + kx] = bf16_RNE(img[n, c, 14 py + ky, 14 px + kx]),
columns >= 588 are +0.  Position-coded images hold the bf16 value whose bit pattern is 0x80 + the flat pixel index (distinct,
exact in bf16), so a wrong element decodes to the pixel that was read.  dino_assemble: class row cls + pos[0], four register
rows copied bit for bit, patch rows one IEEE fp32 add float(bf16 patch) + pos[1 + p] (a torch fp32 add).

E. swiglu_bf16 = bf16(bf16(silu(g)) u).  silu in fp64; the inner bf16 value may be any in admissible(silu*, |silu*|, 2^-21)
(the same 8u as expf above: the kernel's silu is g * rcp(1 + exp(-g)), device exp and rcp plus two roundings); a product of
two bf16 values is exact in fp32, so the output must lie between the bf16 roundings of (candidate * u) at the two ends - the
double rounding is carried as rowop_check carries und_rounding = 1.  The share of elements with more than one admissible
inner value is capped at MULTI_CAP = 2 % on cases of 1000 elements or more.  The planted gate -88 is where the fast form
g * rcp(1 + exp(-g)) loses its reciprocal to a subnormal flush while silu* = -5.3e-37 is a normal bf16 value: an output of
zero there is flagged (siluf_ in common.h, shared by swiglu_bf16 and the decode kernels' fused SwiGLU, takes x < -87
through x exp(x + 44) exp(-44), exact in its argument for a bf16 gate).

Measured on the CPU (test_imageop_check_cpu.py prints them; fp32 emulations in the kernels' order):
  camera B1 largest |got - ref| / e over P in {1, 2, 3, 4, 5, 7, 8, 37} and the three feature families, with
  camera_weights_b1: 0.019 (t), 0.031 (m9); asserted < 0.5 (the check flags at 2).  With weights of mixed signs in every
  layer (camera_weights) the same ratio is 0.001 (4e-5 on rotation_views' weights, which the tests also put under this
  bound) and a patch row missing from the mean is not flagged.
  Rotation largest error / bound 0.031 on the 8 random views (realised smallest gap 0.457, four views of each sign), 0.026
  on the exact-input family; |R^T R - I| 0.91 u, |det R - 1| 0.76 u.
  pts mode 1 largest error / bound: z 0.13, lx / ly 0.21, world 0.26 (torch's expf on the CPU).
  swiglu: share of elements with two admissible inner values 0.20 % (n = 1000), 0.17 % (n = 8960), 0 flags.
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rowop_check import (MULTI_CAP, NAN_BF16, NAN_F32, Result, admissible, bits, cast_table, from_key,  # noqa: E402,F401
                         is_sentinel, key, rn, sentinel)

U = 2.0 ** -24
TAU_SILU = 2.0 ** -21
FLT_MAX = float(torch.finfo(torch.float32).max)
_TINY = 2.0 ** -300


def rnd(*shape, seed=0):
    g = torch.Generator(); g.manual_seed(seed)
    return torch.randn(shape, generator=g)


def same_or_both_nan(a, b):
    return (a == b) | (torch.isnan(a) & torch.isnan(b))


# ------------------------------------------------------------------------------------------ A. token pickers
def philox_first(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10, first output word; numpy uint64 arithmetic restating csrc/misc.hip::philox_first."""
    M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & MASK), np.uint64(k1 & MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = (h1 ^ c1 ^ k0) & MASK, l1, (h0 ^ c3 ^ k1) & MASK, l0
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0


def gumbel_scores(logits_f32, inv_t, seed, step, row):
    n = logits_f32.shape[0]
    r = philox_first(np.arange(n), row, step, 0, seed & 0xFFFFFFFF, seed >> 32)
    u = ((r >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0
    return logits_f32.astype(np.float64) * inv_t - np.log(-np.log(u))


def argmax_ref(x):
    """x [rows, n] (or [n]): torch.argmax of the fp32 values on the CPU."""
    return torch.argmax(x.detach().cpu().float(), dim=-1)


def argmax_blocks(n):
    """Workgroups per row of the launch (g2v_argmax_bf16 / _rows / g2v_sample_rows_bf16) and elements per workgroup."""
    nb = 64 if n >= 65536 else 1
    return nb, -(-n // nb)


_KEY_NAN, _KEY_NONE = 0x7FFFFFFF, -(1 << 31)


def argmax_key(v, nan_as_inf=False):
    """fp32 numpy array -> int64 keys, monotone in the value, -0 == +0, NaN on top (or merged as +inf: the old rule)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    b = v.view(np.int32).astype(np.int64)
    k = np.where(b >= 0, b, b ^ 0x7FFFFFFF)
    k = np.where(v == 0, 0, k)
    return np.where(np.isnan(v), 0x7F800000 if nan_as_inf else _KEY_NAN, k)


def _pick(k, i, axis):
    """Winner of a merge along `axis`: the largest key, the lowest index among equals."""
    top = k.max(axis=axis, keepdims=True)
    ii = np.where(k == top, i, np.int64(1) << 40).min(axis=axis)
    return top.squeeze(axis), ii


def argmax_emul(row, nan_as_inf=False, nb=None):
    """The kernel's merge tree on one fp32 row: per thread over its stride of 256, across the 64 lanes of a wave, across the
    four waves, across the workgroups; the final index is clamped as the kernel clamps it."""
    row = np.asarray(row, dtype=np.float32)
    n = row.shape[0]
    if nb is None:
        nb = argmax_blocks(n)[0]
    per = -(-n // nb)
    keys = argmax_key(row, nan_as_inf)
    bk, bi = [], []
    for b in range(nb):
        lo, hi = b * per, min(n, b * per + per)
        m = max(hi - lo, 0)
        strides = -(-m // 256) if m else 0
        k = np.full((max(strides, 1), 256), _KEY_NONE, dtype=np.int64)
        i = np.full((max(strides, 1), 256), 0x7FFFFFFF, dtype=np.int64)
        k.reshape(-1)[:m] = keys[lo:hi]
        i.reshape(-1)[:m] = np.arange(lo, hi)
        tk, ti = _pick(k, i, 0)                                   # each thread over its strides
        wk, wi = _pick(tk.reshape(4, 64), ti.reshape(4, 64), 1)   # each wave
        k1, i1 = _pick(wk, wi, 0)                                 # the four waves
        bk.append(k1); bi.append(i1)
    _, i2 = _pick(np.array(bk), np.array(bi), 0)
    i2 = int(i2)
    return i2 if 0 <= i2 < n else 0


def argmax_cases(n):
    """[(name, fp32 row [n])]: every winner placement and special of section A at this n (values exact in bf16)."""
    nb, per = argmax_blocks(n)
    decr = (-1 - torch.arange(n, dtype=torch.float64) / n).float().bfloat16().float()      # non-increasing, -1 .. -2
    const = torch.full((n,), -1.5)
    inf, nan = float("inf"), float("nan")
    edges = [(63, 64), (255, 256)] + ([(k * per - 1, k * per) for k in (1, 32, 63)] if nb > 1 else [])
    marks = sorted({i for i in [0, n - 1] + [j for e in edges for j in e] if 0 <= i < n})
    pairs = [e for e in edges if e[1] < n] + ([(0, n - 1)] if n > 1 else [])               # (0, n - 1): last of the last workgroup
    cases = []

    def add(name, base, **at):
        row = base.clone()
        for i, v in at.items():
            row[int(i[1:])] = v
        cases.append((name, row))
    for bn, base in (("decr", decr), ("const", const)):
        for i in marks:
            add(f"{bn} max@{i}", base, **{f"i{i}": 3.0})
        for i, j in pairs:
            add(f"{bn} tie@{i},{j}", base, **{f"i{i}": 3.0, f"i{j}": 3.0})
    if n > 1:
        i, j = n // 3, max(2 * n // 3, n // 3 + 1)
        add(f"-0@{i} +0@{j}", decr, **{f"i{i}": -0.0, f"i{j}": 0.0})
        add(f"+0@{i} -0@{j}", decr, **{f"i{i}": 0.0, f"i{j}": -0.0})
    cases.append(("all -inf", torch.full((n,), -inf)))
    add(f"NaN@{n // 2}", decr, **{f"i{n // 2}": nan})
    spots = [(0, 1), (62, 65), (100, 356)] + ([(5, n - 3), (per - 1, per)] if nb > 1 else [])
    for i, j in spots:                                  # one wave; two waves; one thread (i, i + 256); two workgroups
        if j >= n:
            continue
        add(f"inf@{i} NaN@{j}", decr, **{f"i{i}": inf, f"i{j}": nan})
        add(f"NaN@{i} inf@{j}", decr, **{f"i{i}": nan, f"i{j}": inf})
        extra = {f"i{j + 1}": inf} if j + 1 < n else {}
        add(f"NaN@{i} NaN@{j}", decr, **{f"i{i}": nan, f"i{j}": nan}, **extra)
    return cases


def argmax_matrix(cases, n, pad=8):
    """bf16 [len(cases), n + pad]: the case rows, the padding columns alternately +inf and NaN (they must never win)."""
    x = torch.empty(len(cases), n + pad)
    x[:, n::2] = float("inf")
    x[:, n + 1::2] = float("nan")
    for r, (_, row) in enumerate(cases):
        x[r, :n] = row
    return x.bfloat16()


# --------------------------------------------------------------------------------------------- B. camera tail
def camera_features(N, P, seed):
    """[N, P, 512] fp32: view i of family i % 3: |randn|, 100 + randn, all zero."""
    z = rnd(N, P, 512, seed=seed)
    f = torch.empty(N, P, 512)
    for i in range(N):
        f[i] = (z[i].abs(), 100 + z[i], torch.zeros(P, 512))[i % 3]
    return f


def camera_weights(seed, wr_scale=0.05, br_scale=1.0):
    """(w0, b0, w1, b1, wt, bt, wr, br) of the camera head's tail, fp32, every sign mixed (B2's rotation views)."""
    s = 512 ** -0.5
    return (rnd(512, 512, seed=seed + 1) * s, rnd(512, seed=seed + 2) * 0.1, rnd(512, 512, seed=seed + 3) * s,
            rnd(512, seed=seed + 4) * 0.1, rnd(3, 512, seed=seed + 5) * 0.05, rnd(3, seed=seed + 6),
            rnd(9, 512, seed=seed + 7) * wr_scale, rnd(9, seed=seed + 8) * br_scale)


def camera_weights_b1(seed):
    """B1's weights.  The running bound is a worst-case one: through a layer of mixed signs |W| |v| is ~ sqrt(512) times
    |W v|, three layers of that make the bound thousands of times the kernel's error and wider than the effect of a patch
    row missing from the mean.  So the two hidden layers' weights are non-negative (|randn| / 512: |W| |v| = W v on
    non-negative inputs) and the two heads' lean positive (0.05 randn + 0.03); the biases keep mixed signs (0.5 randn in
    the hidden layers), so that about a tenth of the hidden units sit below zero before their ReLU."""
    return (rnd(512, 512, seed=seed + 1).abs() / 512, rnd(512, seed=seed + 2) * 0.5, rnd(512, 512, seed=seed + 3).abs() / 512,
            rnd(512, seed=seed + 4) * 0.5, rnd(3, 512, seed=seed + 5) * 0.05 + 0.03, rnd(3, seed=seed + 6),
            rnd(9, 512, seed=seed + 7) * 0.05 + 0.03, rnd(9, seed=seed + 8))


def camera_ref64(feat, w0, b0, w1, b1, W, b):
    """fp64 reference of W relu(w1 relu(w0 mean(feat) + b0) + b1) + b and its running first-order bound e, both [N, rows]."""
    f = feat.detach().cpu().double()
    P = f.shape[1]
    v = f.mean(1)
    e = (math.ceil(P / 4) + 3) * U * f.abs().mean(1)
    for Wl, bl, relu in ((w0, b0, True), (w1, b1, True), (W, b, False)):
        Wd, bd = Wl.detach().cpu().double(), bl.detach().cpu().double()
        e = e @ Wd.abs().T + 15 * U * (v.abs() @ Wd.abs().T + bd.abs())
        v = v @ Wd.T + bd
        if relu:
            v = v.clamp_min(0)
    return v, e


def check_camera_linear(got, ref, e):
    """Flag |got - ref| > 2 e; max_ratio = the largest |got - ref| / e."""
    got = got.detach().cpu().double()
    err = (got - ref).abs()
    bad = ~(err <= 2 * e)
    ratio = torch.where(torch.isfinite(err), err / e.clamp_min(_TINY), torch.full_like(err, float("inf")))
    return Result(bad, 0, ratio.max())


def _fma32(a, b, c):
    """fmaf on fp32 tensors through float64 (the product is exact there; the sum is rounded twice, which differs from a true
    fma only on rare ties: this is an emulation of the error size, not of the bits)."""
    return (a.double() * b.double() + c.double()).float()


def _matvec512_emul(W, b, vin, relu, drop_bias=None, skip_relu=None):
    """matvec512 in its own order: per lane 8 fma over k 64 + lane, six xor-shuffle adds, the bias add, ReLU."""
    n_out, N = W.shape[0], vin.shape[0]
    Wk, vk = W.float().view(n_out, 8, 64), vin.view(N, 8, 64)
    s = torch.zeros(N, n_out, 64)
    for k in range(8):
        s = _fma32(Wk[None, :, k, :], vk[:, None, k, :], s)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ o]
    bb = b.float().clone()
    if drop_bias is not None:
        bb[drop_bias] = 0
    out = s[..., 0] + bb
    if relu:
        r = out.clamp_min(0)
        if skip_relu is not None:
            r[:, skip_relu] = out[:, skip_relu]
        out = r
    return out


def camera_emul32(feat, w0, b0, w1, b1, W, b, fault=None, unit=0):
    """The kernel's fp32 arithmetic for one final Linear (W, b) of 3 or 9 rows.  fault: 'drop_last_patch', 'drop_s1',
    'drop_bias' (b0[unit]), 'skip_relu' (first layer's `unit`), 'other_view_mean'."""
    f = feat.float()
    N, P = f.shape[0], f.shape[1]
    s = [torch.zeros(N, 512) for _ in range(4)]
    Pe = P - 1 if fault == "drop_last_patch" else P
    p = 0
    while p + 3 < Pe:
        for j in range(4):
            s[j] = s[j] + f[:, p + j]
        p += 4
    while p < Pe:
        s[0] = s[0] + f[:, p]
        p += 1
    tot = (s[0] + (s[2] + s[3])) if fault == "drop_s1" else ((s[0] + s[1]) + (s[2] + s[3]))
    va = tot / torch.tensor(float(P))
    if fault == "other_view_mean":
        va = va.roll(1, 0)
    vb = _matvec512_emul(w0, b0, va, True, drop_bias=unit if fault == "drop_bias" else None,
                         skip_relu=unit if fault == "skip_relu" else None)
    va = _matvec512_emul(w1, b1, vb, True)
    return _matvec512_emul(W, b, va, False)


def rotation_views():
    """(feat [8, 4, 512], weights) of the eight random views of B2: the rotation head's weights dominate its bias, so every
    view has its own m9.  On the fp64 reference: 4 views with det < 0, 4 with det > 0, smallest gap 0.4566."""
    return rnd(8, 4, 512, seed=0) * 4, camera_weights(0, wr_scale=0.2, br_scale=0.1)


def axis_rotation(axis, angle):
    c, s = math.cos(angle), math.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    M = torch.eye(3, dtype=torch.float64)
    M[i, i], M[i, j], M[j, i], M[j, j] = c, -s, s, c
    return M


def exact_rotation_inputs():
    """[(name, M fp32 [3, 3], name of the input whose reference it must share or None)] of B2's exact-input family."""
    out = [("identity", torch.eye(3), None)]
    for ax in range(3):
        for ang in (0.3, math.pi / 2, 3.0):
            out.append((f"axis{ax} {ang:.3g}", axis_rotation(ax, ang).float(), None))
    base = (axis_rotation(0, 0.7) @ axis_rotation(1, -1.1) @ axis_rotation(2, 2.3)).float()
    out.append(("rows unscaled", base, None))
    out.append(("rows 2^-20, 1, 2^20", base * torch.tensor([2.0 ** -20, 1.0, 2.0 ** 20])[:, None], "rows unscaled"))
    Q = (axis_rotation(2, 0.4) @ axis_rotation(0, 1.9)).double() @ torch.diag(torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64))
    out.append(("reflection Q diag(1, .6, .3)", (Q @ torch.diag(torch.tensor([1.0, 0.6, 0.3], dtype=torch.float64))).float(), None))
    return out


def rotation_ref64(m9):
    """m9 fp32 [N, 9] -> (R [N, 3, 3] fp64: the nearest rotation of the row-normalised m9; gap [N]; det sign [N])."""
    A = m9.detach().cpu().double().view(-1, 3, 3).numpy()
    A = A / np.linalg.norm(A, axis=2, keepdims=True)
    Us, S, Vt = np.linalg.svd(A)
    d = np.where(np.linalg.det(Us @ Vt) < 0, -1.0, 1.0)
    D = np.tile(np.eye(3), (A.shape[0], 1, 1))
    D[:, 2, 2] = d
    return torch.from_numpy(Us @ D @ Vt), torch.from_numpy(S[:, 1] + d * S[:, 2]), torch.from_numpy(d)


def rotation_bound(gap):
    return (28.0 / gap + 2.0) * U


def check_rotation(R_got, R_ref, gap):
    """Flag |R - R*| > (28 / gap + 2) u per element; max_ratio = the largest error / bound."""
    err = (R_got.detach().cpu().double() - R_ref).abs()
    bound = rotation_bound(gap)[:, None, None].expand_as(err)
    ratio = torch.where(torch.isfinite(err), err / bound, torch.full_like(err, float("inf")))
    return Result(~(err <= bound), 0, ratio.max())


def rotation_defects(pose):
    """pose [N, 4, 4] fp32 -> (largest |R^T R - I|, largest |det R - 1|, both in units of u; row 3 == [0, 0, 0, 1])."""
    pose = pose.detach().cpu()
    R = pose[:, :3, :3].double()
    orth = float(((R.transpose(1, 2) @ R) - torch.eye(3, dtype=torch.float64)).abs().max()) / U
    det = float((torch.linalg.det(R) - 1).abs().max()) / U
    row3 = torch.equal(pose[:, 3], torch.tensor([0., 0., 0., 1.]).expand(pose.shape[0], -1))
    return orth, det, row3


def svd_emul(m9, fault=None):
    """svd_orthogonalize of csrc/misc.hip on one view: fp32 row normalisation, one-sided Jacobi in double.  fault:
    'no_flip' (the reflection is returned), 'flip_largest' (the wrong singular direction is flipped)."""
    m = np.asarray(m9, dtype=np.float32).reshape(3, 3)
    A = np.zeros((3, 3))
    for i in range(3):
        nn = np.sqrt(np.float32(m[i, 0] * m[i, 0] + m[i, 1] * m[i, 1] + m[i, 2] * m[i, 2]), dtype=np.float32)
        nn = max(nn, np.float32(1e-12))
        A[i] = (m[i] / nn).astype(np.float32)
    V = np.eye(3)
    for _ in range(30):
        off = 0.0
        for p in range(2):
            for q in range(p + 1, 3):
                al, be, ga = A[:, p] @ A[:, p], A[:, q] @ A[:, q], A[:, p] @ A[:, q]
                off += ga * ga
                if abs(ga) < 1e-300:
                    continue
                zeta = (be - al) / (2.0 * ga)
                tt = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                c = 1.0 / math.sqrt(1.0 + tt * tt)
                s = c * tt
                for M in (A, V):
                    mp, mq = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = c * mp - s * mq, s * mp + c * mq
        if off < 1e-30:
            break
    sig = np.sqrt((A * A).sum(0))
    Us = A * np.where(sig > 1e-150, 1.0 / np.maximum(sig, 1e-300), 0.0)
    j = int(np.argmax(sig)) if fault == "flip_largest" else int(np.argmin(sig))
    d = 1.0 if (np.linalg.det(Us @ V.T) >= 0 or fault == "no_flip") else -1.0
    D = np.ones(3)
    D[j] = d
    return torch.from_numpy(((Us * D) @ V.T).astype(np.float32))


# ----------------------------------------------------------------------------------------- C. point head tail
def shuffle_map(N, H, W, C, ps, fault=None):
    """(row, col) [N, H, W, C] of the feat element that out[n, y, x, c] reads.  fault: 'swap' (iy / ix), 'stride_ps' (channel
    stride PS for PS^2), 'gw_as_gh'."""
    gh, gw = H // ps, W // ps
    P = gh * gw
    n, y, x, c = torch.meshgrid(torch.arange(N), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
    py, iy, px, ix = y // ps, y % ps, x // ps, x % ps
    if fault == "swap":
        iy, ix = ix, iy
    row = n * P + py * (gh if fault == "gw_as_gh" else gw) + px
    col = c * (ps if fault == "stride_ps" else ps * ps) + iy * ps + ix
    return row.clamp_max(N * P - 1), col


def coded_feat(rows, K):
    """feat[r, k] = r K + k, exact in fp32 (below 2^24)."""
    assert rows * K < (1 << 24)
    return torch.arange(rows * K, dtype=torch.float32).view(rows, K)


def check_coded(got, N, H, W, C, ps):
    """Mode 0 / pixel_shuffle on coded features: (flag map, description of the first wrong pixel or '')."""
    row, col = shuffle_map(N, H, W, C, ps)
    K = C * ps * ps
    want = (row * K + col).float()
    got = got.detach().cpu().view(N, H, W, C)
    bad = bits(got) != bits(want)
    msg = ""
    if bool(bad.any()):
        n, y, x, c = bad.nonzero()[0].tolist()
        g = float(got[n, y, x, c])
        rd = f"feat[{int(g) // K}, {int(g) % K}]" if math.isfinite(g) and 0 <= g < N * (H // ps) * (W // ps) * K else repr(g)
        msg = f"out[{n}, {y}, {x}, {c}] read {rd}, not feat[{int(row[n, y, x, c])}, {int(col[n, y, x, c])}]"
    return bad, msg


def pts_inputs(N, H, W, ps, seed):
    """(feat [N P, 3 PS^2] fp32, pose [N, 4, 4] fp32).  c = 0.5 randn with -100, -87.5, 0, 88, 89, 89 planted on the first
    pixels of the last view's last patch; poses: identity, a random rotation with a unit-size translation, one with
    translation 1e3 (view i takes pose i % 3; a lone view takes the random one, so that N = 1 exercises the rotation)."""
    PP = ps * ps
    P = (H // ps) * (W // ps)
    feat = rnd(N * P, 3 * PP, seed=seed)
    feat[:, 2 * PP:] *= 0.5
    r = N * P - 1
    for k, (c, ab) in enumerate(((-100.0, 0.0), (-87.5, 0.0), (0.0, None), (88.0, 0.25), (89.0, 0.0), (89.0, None))):
        feat[r, 2 * PP + k] = c
        if ab is not None:
            feat[r, k] = feat[r, PP + k] = ab
    pose = torch.eye(4).repeat(N, 1, 1)
    for v in range(N):
        i = v + (N == 1)                                       # a lone view takes the random pose, not the identity
        if i % 3:
            q, _ = torch.linalg.qr(rnd(3, 3, seed=seed + 10 + i).double())
            pose[v, :3, :3] = (q * torch.linalg.det(q).sign()).float()
            pose[v, :3, 3] = rnd(3, seed=seed + 20 + i) * (1.0 if i % 3 == 1 else 1e3)
    return feat, pose


class PtsResult:
    def __init__(self, z, xy, world):
        self.z, self.xy, self.world = z, xy, world
        self.count = z.count + xy.count + world.count

    def report(self, what=""):
        return "; ".join([self.z.report(what + " z"), self.xy.report(what + " lx/ly"), self.world.report(what + " world")])


def _ratio(err, bound, skip):
    r = torch.where(skip | (bound <= 0), torch.zeros_like(err), err / bound.clamp_min(_TINY))
    return torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).max()


def check_pts_mode1(feat, pose, N, H, W, ps, local, world):
    """local, world [N, H, W, 3] fp32 of g2v_pts_epilogue_ps mode 1 against the fp64 reference and the bounds of section C."""
    row, col = shuffle_map(N, H, W, 3, ps)
    feat, pose = feat.detach().cpu(), pose.detach().cpu()
    v = feat[row, col]
    a, b, c = v[..., 0].double(), v[..., 1].double(), v[..., 2].double()
    zs = c.exp()
    over = zs > FLT_MAX
    local, world = local.detach().cpu().view(N, H, W, 3), world.detach().cpu().view(N, H, W, 3)
    p = torch.stack([a * zs, b * zs, zs], -1)
    e = torch.stack([9 * U * a.abs() * zs, 9 * U * b.abs() * zs, torch.clamp_min(2.0 ** -21 * zs, 2.0 ** -126)], -1)
    T = pose.double()
    Ta = T[:, :3, :3].abs()
    wref = torch.einsum("nrj,nhwj->nhwr", T[:, :3, :3], p) + T[:, None, None, :3, 3]
    wb = torch.einsum("nrj,nhwj->nhwr", Ta, e) + 4 * U * (torch.einsum("nrj,nhwj->nhwr", Ta, p.abs()) + T[:, None, None, :3, 3].abs())
    # where z* leaves the fp32 range: z = +inf and everything after it as fp32 ops give it
    z32 = torch.full_like(v[..., 2], float("inf"))
    lx32, ly32 = v[..., 0] * z32, v[..., 1] * z32
    l32 = torch.stack([lx32, ly32, z32], -1)
    Tf = pose.float()
    w32 = Tf[:, None, None, :3, 0] * lx32[..., None]
    w32 = Tf[:, None, None, :3, 1] * ly32[..., None] + w32
    w32 = Tf[:, None, None, :3, 2] * z32[..., None] + w32
    w32 = w32 + Tf[:, None, None, :3, 3]
    o3 = over[..., None].expand(N, H, W, 3)
    el = (local.double() - p).abs()
    bad_l = torch.where(o3, ~same_or_both_nan(local, l32), ~(el <= e))
    ew = (world.double() - wref).abs()
    bad_w = torch.where(o3, ~same_or_both_nan(world, w32), ~(ew <= wb))
    return PtsResult(Result(bad_l[..., 2], 0, _ratio(el[..., 2], e[..., 2], over)),
                     Result(bad_l[..., :2], 0, _ratio(el[..., :2], e[..., :2], o3[..., :2])),
                     Result(bad_w, 0, _ratio(ew, wb, o3)))


def pts_emul32(feat, pose, N, H, W, ps, fault=None):
    """pts_epilogue_kernel mode 1 in fp32 (torch's expf, one multiply each for lx / ly, the kernel's fma chain).  fault: the
    index faults of shuffle_map, or 'prev_pose' (view n takes the pose of view n - 1)."""
    row, col = shuffle_map(N, H, W, 3, ps, fault)
    v = feat.float()[row, col]
    a, b, c = v[..., 0], v[..., 1], v[..., 2]
    z = c.exp()
    lx, ly = a * z, b * z
    T = pose.float().roll(1, 0) if fault == "prev_pose" else pose.float()
    w = T[:, None, None, :3, 0] * lx[..., None]
    w = _fma32(T[:, None, None, :3, 1], ly[..., None], w)
    w = _fma32(T[:, None, None, :3, 2], z[..., None], w)
    w = w + T[:, None, None, :3, 3]
    return torch.stack([lx, ly, z], -1), w


# ------------------------------------------------------------------------------------------- D. DINO front end
CODE0 = 0x80                                          # the first normal bf16 bit pattern


def coded_image(N, H, W):
    """[N, 3, H, W] fp32: pixel i (flat) holds the bf16 value with bit pattern 0x80 + i - distinct, finite, exact in bf16."""
    n = N * 3 * H * W
    assert CODE0 + n <= 0x7F80
    return (torch.arange(n, dtype=torch.int32) + CODE0).to(torch.int16).view(torch.bfloat16).float().view(N, 3, H, W)


def special_image(N, H, W):
    """cast_table()'s values tiled over the image."""
    tab = cast_table()
    n = N * 3 * H * W
    return tab.repeat(-(-n // tab.numel()))[:n].clone().view(N, 3, H, W)


def im2col14_ref(img, Kpad, fault=None):
    """bf16 [N P, Kpad]; fault 'swap' transposes ky / kx inside a patch, 'gw_as_gh' walks the patch grid with the wrong width."""
    N, _, H, W = img.shape
    gh, gw = H // 14, W // 14
    t = img.detach().cpu().view(N, 3, gh, 14, gw, 14)
    t = t.permute(0, 2, 4, 1, 5, 3) if fault == "swap" else t.permute(0, 2, 4, 1, 3, 5)
    if fault == "gw_as_gh":
        t = t.transpose(1, 2)
    out = torch.zeros(N * gh * gw, Kpad, dtype=torch.bfloat16)
    out[:, :588] = t.reshape(N * gh * gw, 588).bfloat16()
    return out


def check_im2col14(got, img, Kpad, coded=False):
    """(flag map, description of the first wrong element).  NaN pixels must give a NaN (its payload is not compared)."""
    want = im2col14_ref(img, Kpad)
    got = got.detach().cpu()
    nan = torch.isnan(want.float())
    bad = torch.where(nan, ~torch.isnan(got.float()), bits(got) != bits(want))
    msg = ""
    if bool(bad.any()):
        r, k = bad.nonzero()[0].tolist()
        msg = f"out[{r}, {k}] = {hex(int(bits(got)[r, k]) & 0xFFFF)}, want {hex(int(bits(want)[r, k]) & 0xFFFF)}"
        if coded:
            _, _, H, W = img.shape
            i = (int(bits(got)[r, k]) & 0xFFFF) - CODE0
            msg += f": read img{[i // (3 * H * W), i // (H * W) % 3, i // W % H, i % W]}"
    return bad, msg


def dino_inputs(N, P, C, seed):
    """(patch bf16 [N P, C], cls [C], regs [4, C], pos [P + 1, C]) with NaN payloads, -0 and infinities in the registers."""
    patch = (rnd(N * P, C, seed=seed) * 3).bfloat16()
    cls, regs, pos = rnd(C, seed=seed + 1), rnd(4, C, seed=seed + 2), rnd(P + 1, C, seed=seed + 3) * 0.02
    sp = cast_table()[:8]
    regs.view(-1)[:min(8, 4 * C)] = sp[:min(8, 4 * C)]
    return patch, cls, regs, pos


def dino_assemble_ref(patch, cls, regs, pos, N, P, fault=None):
    """fp32 [N (P + 5), C]; fault 'pos_shift' adds pos[p] instead of pos[1 + p], 'other_view' reads view n - 1's patches."""
    C = cls.shape[0]
    x = torch.empty(N, P + 5, C)
    x[:, 0] = cls.float() + pos[0].float()
    x[:, 1:5] = regs.float()
    pp = patch.detach().cpu().float().view(N, P, C)
    if fault == "other_view":
        pp = pp.roll(1, 0)
    x[:, 5:] = pp + (pos[:P] if fault == "pos_shift" else pos[1:]).float()[None]
    return x.view(N * (P + 5), C)


# ------------------------------------------------------------------------------------------------ E. swiglu
def swiglu_split(gu, n):
    """(gate, up) [n] of the 16-interleaved gu."""
    i = torch.arange(n)
    b, j = i >> 4, i & 15
    return gu[32 * b + j], gu[32 * b + 16 + j]


def swiglu_inputs(n, seed):
    """bf16 [32 ceil(n / 16)]: gates 3 randn with +-20, +-88, +-0 planted on the first six, ups randn; unread elements NaN."""
    m = 32 * (-(-n // 16))
    gu = torch.full((m,), float("nan"))
    i = torch.arange(n)
    gi, ui = 32 * (i >> 4) + (i & 15), 32 * (i >> 4) + 16 + (i & 15)
    gu[gi] = 3 * rnd(n, seed=seed)
    gu[ui] = rnd(n, seed=seed + 1)
    planted = torch.tensor([20.0, -20.0, 88.0, -88.0, 0.0, -0.0])[:n]
    gu[gi[:planted.numel()]] = planted
    return gu.bfloat16()


def check_swiglu(got, gu, n):
    """Result over out [n] bf16: key(got) within the bf16 roundings of (admissible inner value) * u; multi counts elements
    with more than one admissible inner value."""
    g, u = swiglu_split(gu.detach().cpu(), n)
    got = got.detach().cpu()
    gd = g.double()
    s = gd * torch.sigmoid(gd)
    slo, shi, cnt = admissible(s, s.abs(), TAU_SILU)
    o1, o2 = (slo.float() * u.float()).bfloat16(), (shi.float() * u.float()).bfloat16()
    k1, k2, k = key(o1), key(o2), key(got)
    bad = (k < torch.minimum(k1, k2)) | (k > torch.maximum(k1, k2)) | ~torch.isfinite(got.float())
    return Result(bad, (cnt > 1).sum(), 0.0)


def swiglu_emul32(gu, n, fault=None):
    """The kernel in fp32: g * (1 / (1 + exp(-g))), bf16, * u, bf16.  fault: 'one_rounding' (the inner bf16 rounding
    skipped), 'swap' (gate and up exchanged)."""
    g, u = swiglu_split(gu, n)
    if fault == "swap":
        g, u = u, g
    g, u = g.float(), u.float()
    s = g * (1.0 / (1.0 + torch.exp(-g)))
    if fault != "one_rounding":
        s = s.bfloat16().float()
    return (s * u).bfloat16()
