"""Structured score profiles for the prefill attention (csrc/attn.hip): builders, an fp64 reference with derived per-element
bounds, and a torch emulation of flash_fwd_kernel / flash_fwd64_kernel / flash_combine_kernel on the CPU.

A helper module (pytest does not collect it), importable without a GPU.  tests/test_flash_profile_cpu.py proves the bounds on
the emulation and shows which planted errors each family exposes; tests/test_flash_profile_gpu.py applies the builders and the
bounds to the kernels.  It also holds what that module shares with tests/test_attention_gpu.py: ref_fp64, launch, padded_inputs,
forms, heads, attn_form and the row bounds BOUND[D].

Profiles.  A profile is the level L_j of key j's score in log2 units after scale . log2 e (c = D^-1/2 log2 e).  As in
growth_inputs (test_attention_gpu.py) a score is noise + a_i b_j along a common direction with the noise orthogonal to it; here
the direction is the LAST R = 16 coordinates of the head (8 at D = 16), all equal: q rows carry a (R a = 16) there, K rows carry
b_j, the noise is zero there, so L_j = 16 c b_j and bf16 holds the level exactly whenever it holds b_j.  The level-carrying
products are then exact in fp32 and sit in the last k-step of QK^T: the partial sums before it are noise-sized.
  peak    row class i mod R carries coordinate r of the direction block, ONE key j_r carries it too: that key lies `delta` above
          every other score of the class's rows (8, 30, 200; at 200 every other weight underflows: the output IS that V row).  Over
          the variants of one D the peak visits every slot of a full tile, every slot of the partial last tile, key 0, key
          k_len - 1 and, causally, the last allowed key of a row (peak_coverage)
  ramp    b_j = (j - (Lk - 1)) 2^k, exact for Lk <= 256: the level rises by 0.7 .. 1.4 per key, every row selects its last allowed key
  flat    every K row of a kv head is the same row: equal weights.  V column 0 is 1 on key 0 alone, column 1 is 1 on the odd keys:
          the output there is 1 / n and (odd keys) / n for n visible keys
  rise / fall   b_j = (tile(j) - last tile) s and - tile(j) s: the level steps by 0.5, 3, 20, 70, 200 (rounded UP to 5 bits of s, so
          that 6 s is exact in bf16) per 64-key tile and the highest tile sits at level 0; `alt`: only the rows of even 32-row blocks
          carry it.  70 and 200 take flash_fwd64_kernel's cold rescale at every tile, 200 makes alpha underflow, fall leaves the later
          weights far below the first tile's reference.  Causal windows take fall at every step and rise up to 20: a causal row
          that ends below the top tile has its maximum at -step x (tiles below), and the fp32 share grows with that (below)
  offset  every score of a kv head at +250, of the next at -250
  wide    L_j uniform in +-R per key, R = 40, 120
  gauss   plain Gaussian q, k: the control
Every builder asserts its profile on the fp64 scores of the rounded tensors.

Bounds.  The kernels round each weight p_j = 2^(s_j c - m) to bf16 for the P.V MFMA (f2bf / pack_bf16x2: v_cvt_pk_bf16_f32, round
to nearest even, unit roundoff u = 2^-8); V is bf16 and exact; products and sums are fp32; flash_fwd_kernel sums the unrounded p
into l, flash_fwd64_kernel sums the SAME rounded p on the matrix pipe; one division; one rounding of the output to bf16.  With p
the normalised fp64 weights, want = sum p_j v_jd, T_d = sum p_j |v_jd|, Q_d = sum p_j^2 v_jd^2, P2 = sum p_j^2:
  hard   |got - want| <= (1 + EPS) (u (T_d + |want_d|) + u |want_d|).  Every weight off by u in the worst direction: with l from
         the rounded p the error is sum p_j d_j (v_jd - want_d) / (1 + sum p_j d_j), |d_j| <= u, at most u (T_d + |want_d|) (1 + u); with l
         from the unrounded p it is sum p_j d_j v_jd <= u T_d.  u |want_d| is the output's own rounding.
         EPS = 0.10 is the fp32 share, in units of u (one fp32 rounding = 2^-24 = 2^-16 u), at the shapes of the GPU module
         (Lk <= 420: 7 tiles) and LMAX = 300, the largest |row maximum| any family reaches (ramp, causal: 1.41 x 199; offset: 250 +
         noise; every other family's rows have their maximum within +-220 of 0):
           sums        O and l each: 7 tiles x 4 chained MFMAs x 16 terms + 7 rescales + <= 16 fmaf of the combine + the cross-lane
                       add ~ 480 roundings, relative to T_d (O) and to 1 (l): 2 x 480 x 2^-16 = 1.5 %
           scores      a raw score is one chain of fp32 adds; the level enters in the last k-step, so at most 16 products + 1
                       accumulate round at the level's magnitude: 17 x 2^-24 LMAX ln 2 relative in p = 5.4 %
           exponents   m c, (m_old - m_new) c, the fmaf's single rounding (at most |s c - m c| <= LMAX), and the two m . c that meet
                       in the combine's exp2(m_s - M): 5 x 2^-24 LMAX ln 2 = 1.6 % (flash_fwd64_kernel's integer reference makes
                       alpha and m_s - M exact: its share is the fmaf alone)
           exp2        v_exp_f32 is good to 1 ulp: p, alpha and the combine's weight: 3 x 2^-23 = 0.01 %
           division    1 / l and the product: 2.5 x 2^-24 = 0.004 %
           second order  (1 + u)^2 - 1 = 0.8 %
         total 9.3 %.
  exact  flat only: all scores of a row are bit-equal, so are the p, and the rounding of p cancels (rounded l) or is absent (p = 1
         to 2^-24 LMAX: the exponent residue): |got - want| <= (1 + EPS) u |want_d| + EPS u (T_d + |want_d|)
  sharp  |got - want| <= 6 sigma_d + 2 u |want_d|, sigma_d = 2^-7 / sqrt 12 (sqrt Q_d + |want_d| sqrt P2): the weights' rounding
         errors taken as independent and uniform over a bf16 spacing (at most 2^-7 relative); sqrt Q_d is the numerator's share,
         |want_d| sqrt P2 the share of a denominator summed from the rounded p (triangle inequality; flash_fwd_kernel does not have
         it); 6 sigma for ~1e8 compared elements; 2 u |want_d| = the output rounding plus a fully correlated share (rows whose
         weights sit at one place of a binade).  Only for families that carry noise (all but flat).
None of the three is taken from a run of the kernels.

Emulation (emulate): 64-key tiles; `generic` = online softmax in the log2 domain with the running RAW maximum, p = exp2(fma(s, c,
-(m c))), l from the unrounded p; `fwd64` = integer reference ceil(max s c) of the segment's first tile, raised only when a row of the
64-row wave outgrows it by more than RESCALE_THR, l from the rounded p; bf16 P, fp32 accumulation; the KV tiles cut into segments
at arbitrary tile boundaries, each leaving (m in log2 units, l, O), merged as flash_combine_kernel does.  Raw scores are the fp64
dot product rounded once to fp32.  FAULTS are planted in it (see emulate).
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

U = 2.0 ** -8
EPS = 0.10
LMAX = 300.0
SIGMA_UNIT = 2.0 ** -7 / math.sqrt(12.0)
LOG2E = 1.4426950408889634
KV_TILE = 64
RESCALE_THR = 64.0
NEG = -1e30
EXACT_DELTA = 200.0

NAN_BITS = 0x7FA5                      # bf16 quiet NaN with a payload no kernel writes
GLOBAL_REL = 6e-3
# per head dim: (e_max, e_row) row bounds of tests/test_attention_gpu.py - see its docstring for the rule and the measured maxima
BOUND = {16: (2.43e-2, 8.72e-3), 64: (2.87e-2, 5.44e-3), 80: (2.87e-2, 5.33e-3), 96: (2.72e-2, 5.11e-3), 128: (3.36e-2, 5.90e-3)}
SWEEP_DS = [16, 64, 80, 96, 128]
Q0, K0 = 5, 7                                 # the window starts inside the buffers: rows before it are NaN


# ------------------------------------------------------------------------------------------------ shared with test_attention_gpu.py
class attn_form:
    """g2v_debug_attn_form for the duration of a block (0 = flash_fwd_kernel<128,8> for 256-row items), restored to 1."""

    def __init__(self, hip, f):
        self.hip, self.f = hip, f

    def __enter__(self):
        self.hip.lib().g2v_debug_attn_form(self.f)

    def __exit__(self, *exc):
        self.hip.lib().g2v_debug_attn_form(1)


def nan_bf16(rows, cols):
    return torch.full((rows, cols), float("nan"), dtype=torch.bfloat16, device="cuda")


def ref_fp64(q, k, v, windows, Hq, Hkv, D, scale=None, sums=False):
    """Attention of the bf16 views q [*, >= Hq*D], k / v [*, >= Hkv*D] in float64: per window softmax(Q K^T scale) V,
    GQA by head repeat, bottom-right causal mask.  Windows with the same query rows are ONE softmax over the union of
    their key ranges (the phases of a view-sharded plan).  Returns {(q0, q_len): float64 [q_len, Hq, D]}; with sums,
    {(q0, q_len): (want, T, Q, P2)}: T_d = sum p_j |v_jd|, Q_d = sum p_j^2 v_jd^2 [q_len, Hq, D] and P2 = sum p_j^2 [q_len, Hq, 1]
    with p the normalised weights."""
    scale = D ** -0.5 if scale is None else scale
    rep = Hq // Hkv
    groups = {}
    for w in windows:
        groups.setdefault((w[0], w[1]), []).append(w)
    out = {}
    for (q0, ql), ws in groups.items():
        causal = bool(ws[0][4])
        assert len(ws) == 1 or not causal
        rows = torch.cat([torch.arange(w[2], w[2] + w[3], device=q.device) for w in ws])
        K = k[rows, :Hkv * D].view(-1, Hkv, D).double()
        V = v[rows, :Hkv * D].view(-1, Hkv, D).double()
        Lk = K.shape[0]
        o = torch.empty((ql, Hq, D), dtype=torch.float64, device=q.device)
        if sums:
            T, Qs, P2 = torch.empty_like(o), torch.empty_like(o), torch.empty((ql, Hq, 1), dtype=torch.float64, device=q.device)
        blk = max(1, min(ql, (1 << 25) // (rep * Lk)))
        for h in range(Hkv):
            Kt, Vh = K[:, h].t(), V[:, h]
            for r0 in range(0, ql, blk):
                r1 = min(ql, r0 + blk)
                Q = q[q0 + r0:q0 + r1, h * rep * D:(h + 1) * rep * D].double().view(r1 - r0, rep, D).transpose(0, 1)
                s = torch.matmul(Q, Kt) * scale
                if causal:
                    i = torch.arange(r0, r1, device=q.device).view(-1, 1)
                    j = torch.arange(Lk, device=q.device).view(1, -1)
                    s.masked_fill_(j > i + (Lk - ql), float("-inf"))
                p = torch.softmax(s, dim=-1)
                o[r0:r1, h * rep:(h + 1) * rep] = torch.matmul(p, Vh).transpose(0, 1)
                if sums:
                    T[r0:r1, h * rep:(h + 1) * rep] = torch.matmul(p, Vh.abs()).transpose(0, 1)
                    Qs[r0:r1, h * rep:(h + 1) * rep] = torch.matmul(p * p, Vh * Vh).transpose(0, 1)
                    P2[r0:r1, h * rep:(h + 1) * rep, 0] = (p * p).sum(-1).transpose(0, 1)
        out[(q0, ql)] = (o, T, Qs, P2) if sums else o
    return out


def covered_rows(windows, n_rows):
    m = torch.zeros(n_rows, dtype=torch.bool, device="cuda")
    for w in windows:
        m[w[0]:w[0] + w[1]] = True
    return m


def launch(hip, q, k, v, plan, Hq, Hkv, D, windows, n_rows, ldo, phase_by_phase=False):
    """One attention into a NaN-payload output [n_rows, ldo]; checks that the kernel wrote exactly the window rows x [0, Hq*D)
    and left every other bit alone.  Returns the output view [n_rows, Hq*D]."""
    buf = torch.full((n_rows, ldo), NAN_BITS, dtype=torch.int16, device="cuda")
    out = buf.view(torch.bfloat16)[:, :Hq * D]
    if phase_by_phase:
        for ph in range(len(plan.phases)):
            hip.flash_attn(q, k, v, out, plan, Hq, Hkv, D, phase=ph)
    else:
        hip.flash_attn(q, k, v, out, plan, Hq, Hkv, D)
    cov = covered_rows(windows, n_rows)
    assert bool((buf[~cov] == NAN_BITS).all()), "a row outside every window was written"
    assert bool((buf[:, Hq * D:] == NAN_BITS).all()), "a column past Hq*D was written"
    assert bool(torch.isfinite(out[cov].float()).all()), "non-finite output inside a window (read outside the window?)"
    return out


def padded_inputs(Lq, Lk, Hq, Hkv, D, q_val, k_val, v_val):
    """Window [Q0, Q0+Lq) of q and [K0, K0+Lk) of k / v in NaN-filled buffers with strides wider than H*D."""
    ldq, ldk = Hq * D + 24, Hkv * D + 40
    q, k, v = nan_bf16(Q0 + Lq + 3, ldq), nan_bf16(K0 + Lk + 4, ldk), nan_bf16(K0 + Lk + 4, ldk)
    q[Q0:Q0 + Lq, :Hq * D] = q_val.reshape(Lq, Hq * D).bfloat16()
    k[K0:K0 + Lk, :Hkv * D] = k_val.reshape(Lk, Hkv * D).bfloat16()
    v[K0:K0 + Lk, :Hkv * D] = v_val.reshape(Lk, Hkv * D).bfloat16()
    return q[:, :Hq * D], k[:, :Hkv * D], v[:, :Hkv * D]


def forms(D):
    """(name, tile_rows, g2v_debug_attn_form): the 4-wave form first (the yardstick), then the 8-wave ones."""
    if D == 128:
        return [("4w", 128, 1), ("8w", 256, 0), ("fwd64", 256, 1)]
    return [("4w", 128, 1), ("8w", 256, 1)]


def heads(D):
    return (12, 2) if D == 128 else (4, 4)


# ------------------------------------------------------------------------------------------------ bounds
def hard_bound(want, T):
    return (1 + EPS) * (U * (T + want.abs()) + U * want.abs())


def exact_bound(want, T):
    return (1 + EPS) * U * want.abs() + EPS * U * (T + want.abs())


def sharp_bound(want, Q, P2):
    return 6.0 * SIGMA_UNIT * (Q.sqrt() + want.abs() * P2.sqrt()) + 2.0 * U * want.abs()


NOISY = ("peak", "ramp", "rise", "fall", "offset", "wide", "gauss")          # the sharp bound applies


class Ratios:
    """Worst |err| / bound per name and the count of elements over a bound; works on the tensors' own device."""

    def __init__(self):
        self.worst = {}

    def add(self, name, got, want, hard, sharp=None):
        got = got.double()
        err = (got - want).abs()
        finite = bool(torch.isfinite(got).all())

        def ratio(b):
            if not finite:
                return float("inf"), int(err.numel())
            r = torch.where(err == 0, torch.zeros_like(err), err / b)
            return float(r.max()), int((~(err <= b)).sum())
        rh, nh = ratio(hard)
        rs, ns = ratio(sharp) if sharp is not None else (0.0, 0)
        w = self.worst.setdefault(name, dict(hard=0.0, sharp=0.0, over_hard=0, over_sharp=0, n=0))
        w["hard"], w["sharp"] = max(w["hard"], rh), max(w["sharp"], rs)
        w["over_hard"] += nh; w["over_sharp"] += ns; w["n"] += err.numel()
        return rh, rs, nh, ns

    def report(self, tag):
        for k, w in sorted(self.worst.items()):
            print(f"[{tag}] {k}: |err| / hard {w['hard']:.3f}  |err| / sharp {w['sharp']:.3f}  over {w['over_hard']} + {w['over_sharp']} of {w['n']}")


def check(ratios, name, family, got, sums):
    """got [ql, Hq, D] against (want, T, Q, P2) of ref_fp64(sums=True) under the family's bounds; returns the elements over one."""
    want, T, Q, P2 = sums
    hard = exact_bound(want, T) if family == "flat" else hard_bound(want, T)
    sharp = sharp_bound(want, Q, P2) if family in NOISY else None
    _, _, nh, ns = ratios.add(name, got, want, hard, sharp)
    return nh + ns


def row_errors(got, want, D):
    """(e_max, e_row) [ql, Hq] of test_attention_gpu.Errors: max_d |got - ref| / RMS_d(ref), ||got - ref|| / ||ref||."""
    d = got.double() - want
    rn = want.norm(dim=-1)
    return d.abs().amax(dim=-1) / (rn / math.sqrt(D)), d.norm(dim=-1) / rn


# ------------------------------------------------------------------------------------------------ builders
def c_of(D):
    return D ** -0.5 * LOG2E


def ndir(D):
    return 8 if D == 16 else 16


def ceil5(x):
    """x > 0 rounded up to 5 significant bits (at most 1 / 16 above x)."""
    m, e = math.frexp(x)
    return math.ceil(m * 32) / 32 * 2.0 ** e


def scores_log2(q, k, D):
    """fp64 [Hq, Lq, Lk]: the scores of q [Lq, Hq, D] over k [Lk, Hkv, D] in log2 units."""
    rep = q.shape[1] // k.shape[1]
    kk = k.double().repeat_interleave(rep, dim=1)
    return torch.einsum("ihd,jhd->hij", q.double(), kk) * c_of(D)


def visible(Lq, Lk, causal):
    j = torch.arange(Lk).view(1, -1)
    i = torch.arange(Lq).view(-1, 1)
    return (j <= i + (Lk - Lq)) if causal else torch.ones((Lq, Lk), dtype=torch.bool)


def peak_variants(D):
    """(Lq, Lk, causal, peak keys of the R row classes) of every peak variant of head dim D."""
    R = ndir(D)
    need = [0] + list(range(128, 192)) + list(range(320, 357))           # window 200 x 357: key 0, a full tile, the partial tile
    need += list(range(192, 192 + (-len(need)) % R))
    out = [(200, 357, False, need[i:i + R]) for i in range(0, len(need), R)]
    Lq, Lk = 300, 420                                                    # causal, Lk > Lq: class r's peak is the last allowed key of row i_r
    rows = [r + R * ((5 * r + 1) % (Lq // R)) for r in range(R)]
    out.append((Lq, Lk, True, [i + (Lk - Lq) for i in rows]))
    edge = [0, 419, 63, 64, 383, 384, 418, 200, 1, 31, 32, 65, 127, 128, 385, 400][:R]
    out.append((77, 420, False, edge))
    return out


def peak_coverage(D):
    """What the peaks of peak_variants(D) visit: (slots of a full tile, keys of window 200 x 357's partial tile, key 0, key
    k_len - 1, a causal row's last allowed key)."""
    full, part, first, last, diag = set(), set(), False, False, False
    R = ndir(D)
    for Lq, Lk, causal, keys in peak_variants(D):
        assert len(keys) == R == len(set(keys)) and all(0 <= j < Lk for j in keys)
        for r, j in enumerate(keys):
            if j < KV_TILE * (Lk // KV_TILE):
                full.add(j % KV_TILE)
            elif Lk == 357:
                part.add(j)
            first |= j == 0
            last |= j == Lk - 1
            i = j - (Lk - Lq)
            diag |= causal and 0 <= i < Lq and i % R == r
    return full, part, first, last, diag


def cases(D):
    """Every case of head dim D: dicts (family, param, alt, variant, Lq, Lk, causal)."""
    out = []

    def add(family, param, Lq, Lk, causal, alt=False, variant=0):
        out.append(dict(family=family, param=float(param), alt=alt, variant=variant, Lq=Lq, Lk=Lk, causal=causal))
    for vi, (Lq, Lk, causal, _) in enumerate(peak_variants(D)):
        add("peak", (8.0, 30.0, 200.0)[vi % 3], Lq, Lk, causal, variant=vi)
    for Lq, Lk, causal in ((300, 256, False), (200, 256, True), (200, 200, True)):
        add("ramp", 1.0, Lq, Lk, causal)
    for Lq, Lk, causal in ((200, 357, False), (300, 420, True), (200, 200, True)):
        add("flat", 0.0, Lq, Lk, causal)
    for fam in ("rise", "fall"):
        for si, step in enumerate((0.5, 3.0, 20.0, 70.0, 200.0)):
            for alt in (False, True):
                causal = (fam == "fall" or step <= 20.0) and (alt != (si % 2 == 0))
                Lq, Lk = ((300, 420) if causal else (200, 357)) if si % 2 == 0 else ((200, 420) if causal else (300, 357))
                add(fam, step, Lq, Lk, causal, alt=alt)
    add("offset", 250.0, 200, 357, False)
    add("offset", 250.0, 300, 420, True, variant=1)
    for R_, Lq, Lk, causal in ((40.0, 77, 357, False), (40.0, 200, 420, True), (120.0, 300, 357, False), (120.0, 200, 420, True)):
        add("wide", R_, Lq, Lk, causal)
    add("gauss", 0.0, 77, 420, False)
    add("gauss", 0.0, 300, 357, True)
    return out


def case_id(cs):
    return (f"{cs['family']}-{cs['param']:g}" + ("-alt" if cs["alt"] else "") + (f"-v{cs['variant']}" if cs["variant"] else "")
            + f"-{cs['Lq']}x{cs['Lk']}" + ("-causal" if cs["causal"] else ""))


FAMILIES = ("peak", "ramp", "flat", "rise", "fall", "offset", "wide", "gauss")


def build(cs, Hq, Hkv, D, seed):
    """q [Lq, Hq, D], k, v [Lk, Hkv, D] exactly bf16 (CPU) of one case, and info: `exact` = (bool [Lq], int64 [Lq]): the rows whose
    output must equal a V row bit for bit, and that row's key.  Asserts the profile on the fp64 scores of the rounded tensors."""
    family, param, alt, variant = cs["family"], cs["param"], cs["alt"], cs["variant"]
    Lq, Lk, causal = cs["Lq"], cs["Lk"], cs["causal"]
    assert Lk >= Lq or not causal
    g = torch.Generator()
    g.manual_seed(seed)
    R, c = ndir(D), c_of(D)
    a = 16.0 / R
    vis = visible(Lq, Lk, causal)
    info = dict(exact=None)
    x = torch.randn((Lq, Hq, D), generator=g) * 0.5
    y = torch.randn((Lk, Hkv, D), generator=g) * (0.1 if family == "ramp" else 1.0)
    v = torch.randn((Lk, Hkv, D), generator=g)
    if family == "gauss":
        x = x * 2.0
        q, k = x.bfloat16(), y.bfloat16()
        s = scores_log2(q, k, D)
        assert 0.5 <= float(s.std()) <= 3.0
        return q, k, v.bfloat16(), info
    x[..., D - R:] = 0.0
    y[..., D - R:] = 0.0
    carry = torch.ones(Lq, dtype=torch.bool)
    if alt:
        carry = (torch.arange(Lq) // 32) % 2 == 0
    tile = torch.arange(Lk) // KV_TILE
    if family == "flat":
        y = y[:1].expand(Lk, Hkv, D).clone()
        x[..., D - R:] = a
        v[:, :, 0] = 0.0
        v[0, :, 0] = 1.0
        v[:, :, 1] = (torch.arange(Lk) % 2).float().view(-1, 1)
        q, k = x.bfloat16(), y.bfloat16()
        s = scores_log2(q, k, D)
        assert bool((s == s[..., :1]).all()), "flat: the scores of a row differ"
        return q, k, v.bfloat16(), info
    if family == "peak":
        keys = peak_variants(D)[variant][3]
        cls = torch.arange(Lq) % R
        ap = 4.0
        x[torch.arange(Lq), :, D - R + cls] = ap
        q = x.bfloat16()
        s0 = scores_log2(q, y.bfloat16(), D).masked_fill(~vis, float("-inf"))          # noise alone
        jr = torch.tensor(keys)[cls]                                                    # [Lq]
        sees = vis[torch.arange(Lq), jr]
        at = s0.gather(2, jr.view(1, -1, 1).expand(Hq, Lq, 1))[..., 0]                  # [Hq, Lq]
        need = (s0.amax(-1) - at)[:, sees].max()
        bp = float(torch.tensor((param + float(need) + 0.5) / (ap * c)).bfloat16().float()) * (1 + 2.0 ** -7)
        bp = float(torch.tensor(bp).bfloat16())
        for r, j in enumerate(keys):
            y[j, :, D - R + r] = bp
        k = y.bfloat16()
        s = scores_log2(q, k, D).masked_fill(~vis, float("-inf"))
        pk = s.gather(2, jr.view(1, -1, 1).expand(Hq, Lq, 1))[..., 0]
        rest = s.scatter(2, jr.view(1, -1, 1).expand(Hq, Lq, 1), float("-inf")).amax(-1)
        gap = (pk - rest)[:, sees]
        assert bool((gap >= param).all()) and float(gap.min()) <= param + 16.0, ("peak", float(gap.min()), float(gap.max()))
        if param >= EXACT_DELTA:
            info["exact"] = (sees, jr)
        info["keys"] = keys
        return q, k, v.bfloat16(), info
    # the level families: q carries a on the direction block (the carrying rows), K row j carries b_j
    x[..., D - R:] = (carry.float() * a).view(-1, 1, 1)
    sign = torch.ones(Hkv)
    if family == "ramp":
        kk = round(math.log2(1.0 / (16.0 * c)))
        b = ((torch.arange(Lk) - (Lk - 1)).double() * 2.0 ** kk).view(-1, 1).expand(Lk, Hkv)
    elif family in ("rise", "fall"):
        sb = ceil5(param / (16.0 * c))
        t = (tile - int(tile.max())) if family == "rise" else -tile
        b = (t.double() * sb).view(-1, 1).expand(Lk, Hkv)
    elif family == "offset":
        sign = torch.tensor([1.0 if (h + variant) % 2 == 0 else -1.0 for h in range(Hkv)])
        b = (param / (16.0 * c) * sign).double().view(1, -1).expand(Lk, Hkv)
    elif family == "wide":
        b = ((2 * torch.rand((Lk, 1), generator=g, dtype=torch.float64) - 1) * param / (16.0 * c)).expand(Lk, Hkv)
    else:
        raise ValueError(family)
    b = b.float().bfloat16().float() if family in ("offset", "wide") else b.float()
    assert bool((b.bfloat16().float() == b).all()), "a level is not exact in bf16"
    y[..., D - R:] = b.unsqueeze(-1)
    q, k = x.bfloat16(), y.bfloat16()
    s = scores_log2(q, k, D)                                                            # [Hq, Lq, Lk]
    lvl = (16.0 * c * b.double()).t().repeat_interleave(Hq // Hkv, dim=0)               # [Hq, Lk]: what a carrying row sees
    res = s - lvl.unsqueeze(1) * carry.view(1, -1, 1)
    assert float(res.abs().max()) <= 8.0 and 0.03 <= float(res.std()) <= 3.0, (family, float(res.abs().max()), float(res.std()))
    sm = s.masked_fill(~vis, float("-inf"))
    assert float(sm.amax(-1).abs().max()) <= LMAX, "a row maximum beyond LMAX"
    if family == "ramp":
        last = (torch.arange(Lq) + (Lk - Lq)).clamp(max=Lk - 1) if causal else torch.full((Lq,), Lk - 1)
        assert bool((sm.argmax(-1) == last.view(1, -1)).all()), "ramp: a row does not select its last allowed key"
        step = 16.0 * c * 2.0 ** kk
        assert 0.7 <= step <= 1.42
    elif family in ("rise", "fall"):
        nt = int(tile.max()) + 1
        # (the residue check above holds every single score to its level; here the step itself, on the row-averaged tile means)
        mean = torch.stack([s[:, :, tile == t].mean(-1) for t in range(nt)], -1)        # [Hq, Lq, nt]
        d = (mean[..., 1:] - mean[..., :-1]) * (1.0 if family == "rise" else -1.0)
        dc = d[:, carry].mean(1)
        assert bool((dc >= param - 0.15).all()) and bool((dc <= 1.0625 * param + 0.15).all()), (family, param, dc.min(), dc.max())
        if alt:
            assert float(d[:, ~carry].mean(1).abs().max()) <= 0.15
    elif family == "offset":
        m = s.mean((1, 2)) * sign.repeat_interleave(Hq // Hkv)
        assert bool((m >= 0.99 * param).all()) and bool((m <= 1.01 * param).all()), m.tolist()
    elif family == "wide":
        spread = s.amax(-1) - s.amin(-1)
        assert bool((spread >= 1.6 * param).all()) and bool((spread <= 2.0 * param + 16.0).all())
    return q, k, v.bfloat16(), info


# ------------------------------------------------------------------------------------------------ the kernels, emulated
FAULTS = ("skip_rescale", "l_only", "swap_weights", "v_neighbour", "drop_last_key", "past_diagonal", "stale_p", "ref_never_raised",
          "raw_m", "drop_slot")
FROWS = (32, 64)              # the 32-row block the row-wise faults are planted in
FTILE = 2                     # the KV tile the tile-wise faults are planted in


def segments(nkt, cuts):
    """cuts segments [kt0, kt1) of nkt tiles, at most one per tile."""
    n = min(cuts, nkt)
    b = sorted({(i * nkt) // n for i in range(n + 1)})
    return list(zip(b[:-1], b[1:]))


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def emulate(q, k, v, causal, form, cuts=1, fault=None):
    """out bf16 [Lq, Hq, D] of one window on q [Lq, Hq, D], k / v [Lk, Hkv, D] bf16: form 'generic' (flash_fwd_kernel) or 'fwd64'
    (flash_fwd64_kernel), the KV tiles in `cuts` segments merged as flash_combine_kernel does (cuts = 1: the direct epilogue).
    fault, one of FAULTS:
      skip_rescale      rows FROWS: alpha = 1 whenever their maximum (fwd64: reference) grew
      l_only            rows FROWS: l is rescaled, O is not
      swap_weights      tile FTILE: the weights of keys 17 and 22 change places in the P.V operand
      v_neighbour       tile FTILE: key slot 20 reads the V row of slot 21
      drop_last_key     rows FROWS: key k_len - 1 is masked
      past_diagonal     rows FROWS: the key after the last allowed one is admitted
      stale_p           every tile but a segment's first: d-block 1 (d 32-63; D = 16: d-block 0) of keys 16-31 uses the previous tile's P
      ref_never_raised  fwd64: the reference stays at the first tile's
      raw_m             the second slot's m enters the merge in raw units (m / c)
      drop_slot         the last slot of the merge is dropped"""
    f32 = torch.float32
    Lq, Hq, D = q.shape
    Lk, Hkv = k.shape[0], k.shape[1]
    rep = Hq // Hkv
    c = (torch.tensor(D ** -0.5, dtype=f32) * torch.tensor(LOG2E, dtype=f32))
    nkt = (Lk + KV_TILE - 1) // KV_TILE
    pad = nkt * KV_TILE - Lk
    kmax = torch.arange(Lq) + (Lk - Lq) if causal else torch.full((Lq,), 1 << 30)
    keyi = torch.arange(nkt * KV_TILE)
    vis = (keyi.view(1, -1) < Lk) & (keyi.view(1, -1) <= kmax.view(-1, 1))
    frows = torch.zeros(Lq, dtype=torch.bool)
    frows[FROWS[0]:FROWS[1]] = True
    if fault == "drop_last_key":
        vis[frows, Lk - 1] = False
    if fault == "past_diagonal":
        nxt = kmax + 1
        ok = frows & (nxt < Lk)
        vis[torch.nonzero(ok).flatten(), nxt[ok]] = True
    wave = torch.arange(Lq) // 64
    dblk = slice(0, 16) if D == 16 else slice(32, 64)
    out = torch.empty((Lq, Hq, D), dtype=torch.bfloat16)
    segs = segments(nkt, cuts)
    for h in range(Hq):
        S_all = (q[:, h].double() @ k[:, h // rep].double().t()).float()
        S_all = torch.nn.functional.pad(S_all, (0, pad)).masked_fill(~vis, NEG)
        Vh = torch.nn.functional.pad(v[:, h // rep].float(), (0, 0, 0, pad))
        slots = []
        for kt0, kt1 in segs:
            m = torch.full((Lq,), NEG, dtype=f32)
            l = torch.zeros(Lq, dtype=f32)
            O = torch.zeros((Lq, D), dtype=f32)
            pb_prev = None
            for kt in range(kt0, kt1):
                S = S_all[:, kt * KV_TILE:(kt + 1) * KV_TILE]
                ok = vis[:, kt * KV_TILE:(kt + 1) * KV_TILE]
                Vt = Vh[kt * KV_TILE:(kt + 1) * KV_TILE]
                rmax = S.amax(1)
                if form == "generic":
                    m_new = torch.maximum(m, rmax)
                    alpha = torch.exp2((m - m_new) * c)
                    m = m_new
                    mc = m * c
                else:
                    x = rmax * c
                    if kt == kt0:
                        m = torch.ceil(x)
                    trig = torch.zeros(int(wave.max()) + 1).index_add_(0, wave, (x > m + RESCALE_THR).float())[wave] > 0
                    if fault == "ref_never_raised":
                        trig = torch.zeros_like(trig)
                    m_new = torch.where(trig, torch.maximum(m, torch.ceil(x)), m)
                    alpha = torch.exp2(m - m_new)
                    m = m_new
                    mc = m
                al_l, al_o = alpha, alpha
                if fault == "skip_rescale":
                    al_l = al_o = torch.where(frows, torch.ones_like(alpha), alpha)
                if fault == "l_only":
                    al_o = torch.where(frows, torch.ones_like(alpha), alpha)
                l = l * al_l
                O = O * al_o.unsqueeze(1)
                p = torch.exp2(_fma(S, c, -mc.unsqueeze(1)))
                p = torch.where(ok, p, torch.zeros((), dtype=f32))
                pb = p.bfloat16().float()
                l = l + (p if form == "generic" else pb).sum(1)
                pv, Vu = pb, Vt
                if kt == FTILE and fault == "swap_weights":
                    pv = pb.clone()
                    pv[:, 17], pv[:, 22] = pb[:, 22], pb[:, 17]
                if kt == FTILE and fault == "v_neighbour":
                    Vu = Vt.clone()
                    Vu[20] = Vt[21]
                O = O + pv @ Vu
                if fault == "stale_p" and pb_prev is not None:
                    O[:, dblk] += (pb_prev[:, 16:32] - pb[:, 16:32]) @ Vt[16:32, dblk]
                pb_prev = pb
            slots.append((mc, l, O))
        if len(slots) == 1:
            _, l, O = slots[0]
            out[:, h] = (O * (1.0 / l).unsqueeze(1)).bfloat16()
            continue
        if fault == "raw_m":
            slots[1] = (slots[1][0] / c, slots[1][1], slots[1][2])
        if fault == "drop_slot":
            slots = slots[:-1]
        M = torch.stack([s_[0] for s_ in slots]).amax(0)
        L = torch.zeros(Lq, dtype=f32)
        acc = torch.zeros((Lq, D), dtype=f32)
        for ms, ls, Os in slots:
            wgt = torch.exp2(ms - M)
            L = _fma(ls, wgt, L)
            acc = _fma(Os, wgt.unsqueeze(1), acc)
        out[:, h] = (acc * (1.0 / L).unsqueeze(1)).bfloat16()
    return out


def reference(q, k, v, causal, D):
    """(want, T, Q, P2) of one window on q [Lq, Hq, D], k / v [Lk, Hkv, D]: ref_fp64 on the flattened rows."""
    Lq, Hq = q.shape[0], q.shape[1]
    Lk, Hkv = k.shape[0], k.shape[1]
    return ref_fp64(q.reshape(Lq, Hq * D), k.reshape(Lk, Hkv * D), v.reshape(Lk, Hkv * D), [(0, Lq, 0, Lk, causal)], Hq, Hkv, D, sums=True)[(0, Lq)]
