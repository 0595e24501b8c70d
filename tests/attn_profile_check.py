"""Structured score profiles for the decode attentions: builders, the kernels' launch plans mirrored, an fp64 reference with two
error bounds, and a torch emulation of the split-KV core (csrc/decode_attn_pg.h) on the CPU.

A helper module (pytest does not collect it), importable without a GPU.  tests/test_attn_profile_cpu.py proves the bounds on
the emulation and shows which planted errors each family exposes; tests/test_decode_fp64_gpu.py, test_kv8_gpu.py and
test_shared_prefix_gpu.py apply the builders and the bounds to the kernels.

Profiles.  A profile is the level L_j of key j's score in log2 units after the softmax scale (s . scale . log2 e).  The K row
of key j is noise_j + t_j d, with d the unit vector along the mean normalised q of the kv head's group (or a given one: the
shared prefix), t_j = L_j / (pmin c2), pmin the smallest projection q_h . d of the heads the profile is promised to; head h then
sees rho_h L_j + noise with rho_h = (q_h . d) / pmin >= 1.  Rows are built in fp32 and rounded to bf16 (and sent through the
e4m3 row quantiser where the cache is e4m3); every builder then asserts its profile on the fp64 scores of the rounded rows.
  saw      L rises by `step` per 32-key batch inside every wave's range and restarts with the next wave; where no wave of the
           slot has a second batch (B = 1: 9 keys per wave) it rises per wave inside every block and restarts with the next
           block, so that the four-wave merge takes the steps
  saw_even the same along a direction orthogonal to the odd heads of the group: only the even heads see it
  rise / fall   L rises / falls by `step` per batch over the whole cache
  peak     one key `delta` above the largest other score of every head; the position rotates over the slots (POSITIONS)
  wide     L drawn uniformly from +-R per wave plus per key
  offset   L = +-R for every key of a head
  flat     every key of the slot has the same K row: equal weights
  gauss    L = 0: the inputs of the existing tests, the control of the planted-error table

Bounds.  The persistent-grid kernels round each weight p_j = 2^((s_j - m) c2) to bf16 (relative error <= u = 2^-8) before the
P.V MFMA; V is bf16 and exact, the products and sums are fp32, l sums the unrounded p, the output is rounded to bf16 once.  With
p the normalised fp64 weights, T_d = sum_j p_j |v_jd| and Q_d = sum_j p_j^2 v_jd^2:
  hard    |got - want| <= 1.05 u (T_d + |want_d|): every weight off by u in the worst direction, plus the output rounding.  The
          5 % covers fp32.  The chain of one output element: 3 batches x 32 keys in a wave's MFMAs, 4 fmaf in merge_waves, 16 fmaf
          and 8 adds in the combine: ~130 chained terms at the shapes here, at most ~600 on a 17000-row cache at B = 8 (600 x
          2^-24 = 1 % of u); the rounding of mc = m c2 and of the merge exponents m scale (2^-24 |m c2| each: 2 % of u at |level|
          = 2600, the largest any family reaches); the exp2 / __expf approximations (2^-22).
  sharp   |got - want| <= 6 sigma_d + 2 u |want_d|, sigma_d = 2^-7 / sqrt(12) sqrt(Q_d): the weights' rounding errors taken as
          uniform over a bf16 spacing (at most 2^-7 relative) and independent, 6 sigma for ~1e6 compared elements, 2 u |want_d|
          for the output rounding plus a fully correlated share.  Only for families that carry noise.
First generation (csrc/decode.hip): the weights stay fp32.  A lane's score is four chained mfma_f32_16x16x32_bf16; S * scale,
S - mx and expf round once each; 16 fmaf per lane, two shuffle adds, then the combine: at most ceil(nchunks / 8) fmaf and 16
adds, one division, expf(m - M).  With A = max_j scale sum_i |q_i k_ji| (natural-log units) the relative error of a weight is
at most e_p = 2^-24 (16 A + 2 A + 4) (score accumulation taken as <= 16 roundings of the absolute dot product, the two roundings
at the score's magnitude, two expf of 2 ulp), the chains add 2^-24 (16 + 2 + 9 + 16 + 1 + 2 A + 4):
  hard1   |got - want| <= u |want_d| + (1 + u) 2^-24 (20 A + 52) (T_d + |want_d|)
  sharp1  |got - want| <= u |want_d| + 6 . 2^-24 (20 A + 52) / sqrt(3) . sqrt(Q_d) + 2^-24 . 64 |want_d|: the output rounding is
          deterministic and stays whole; the weights' fp32 errors are taken as independent with a third of their bound as
          standard deviation.
"""
import math

import torch

U = 2.0 ** -8
SCALE = 128 ** -0.5
LOG2E = 1.4426950408889634
C2 = SCALE * LOG2E
KB = 32
DCH = 64
HARD_FACTOR = 1.05
SIGMA_UNIT = 2.0 ** -7 / math.sqrt(12.0)
NOISE_MIN = 0.25

# (family, parameter): the cases of every kernel
CASES = [("saw", 0.5), ("saw", 3.0), ("saw", 20.0), ("saw", 70.0), ("saw_even", 20.0), ("rise", 0.5), ("rise", 20.0), ("fall", 0.5),
         ("fall", 20.0), ("peak", 8.0), ("peak", 30.0), ("peak", 200.0), ("wide", 40.0), ("wide", 120.0), ("offset", 250.0), ("flat", 0.0)]
NOISY = ("saw", "saw_even", "rise", "fall", "peak", "wide", "offset", "gauss")       # the sharp bound applies
EXACT_DELTA = 200.0                                          # from here every other weight underflows in fp32
POSITIONS = ("row0", "last", "new", "batch_end", "batch_start", "wave3")


# The shapes of the GPU tests of g2v_decode_attn_pg and _kv8: (Hq, Hkv, max_len, slot lengths including the new token).
#   b32  nbh 8, 272 keys per block, 68 per wave: batches of 32, 32 and 4.  Slots 0 - 4: full, one short of full, the new row first
#        in a batch (372 = 340 + 32), last in a batch (371 = 340 + 31), alone in a batch (404 = 340 + 64); every peak position
#        (slot z has POSITIONS[z % 6]) meets a slot long enough for it; the rest cycle through the short lengths of LENS
#   b1   nbh 128, 9 keys per wave, one batch: the merge and the combine over 128 partials carry the whole range
#   g8   G = 8 = GMAX at B = 3: nbh 128, 133 keys per block, 34 per wave: batches of 32 and 2
LENS6 = [1, 2, 32, 33, 65, 357]
PG_SHAPES = {
    "b32": (12, 2, 2176, [2176, 2175, 373, 372, 405, 2176, 357, 2, 2175, 357, 65, 357] + [LENS6[z % 6] for z in range(20)]),
    "b1": (12, 2, 4160, [4160]),
    "g8": (8, 1, 17000, [17000, 4103, 357]),
}
GEN1_SHAPE = (12, 2, 4160, [4160, 4103, 357, 65, 33, 32, 2, 1])                      # B = 8: the shape of the existing test
GEN1_CASES = [("saw", 0.5), ("saw", 3.0), ("saw", 20.0), ("saw", 70.0), ("peak", 30.0), ("peak", 200.0), ("wide", 40.0), ("wide", 120.0)]
SHARED_SHAPE = dict(Hq=12, Hkv=2, B=16, plen=17000, smax=320)


def pg_cases(shape):
    """(case, variant) of a shape: every family; the peak's position rotates over the slots, so a one-slot shape takes one
    variant per position; the group-size edge runs the sawtooth and the peak only."""
    cases = [c for c in CASES if shape != "g8" or c[0] in ("saw", "saw_even", "peak")]
    one = len(PG_SHAPES[shape][3]) == 1
    return [(c, v) for c in cases for v in (range(len(POSITIONS)) if one and c[0] == "peak" else (0,))]


def pg_case_id(cv):
    return f"{case_id(cv[0])}" + (f"-{POSITIONS[cv[1]]}" if cv[1] or cv[0][0] == "peak" else "")


def case_id(c):
    return f"{c[0]}-{c[1]:g}"


# ------------------------------------------------------------------------------------------------ the launch plans, mirrored
def pg_nbh(Hkv, B):
    """decode_attn_pg_nbh (csrc/decode_attn_pg.h): blocks per (scene, kv head)."""
    nbh1 = min(256 // Hkv, 128)
    nbhb = max(512 // (Hkv * B), 8)
    return min(nbhb, nbh1)


def pg_split(cap, nbh):
    """S, SW of g2v_decode_attn_pg / _kv8 (csrc/decode_layer.hip, decode_kv8.hip): keys per block and per wave by capacity."""
    S = (cap + nbh - 1) // nbh
    return S, (S + 3) // 4


def pg_waves(cap, nbh):
    """int64 [nbh, 4, 2]: the (lo, hi) key range of every wave if the cache were full: decode_attn_pg_body's wlo and wcap."""
    S, SW = pg_split(cap, nbh)
    bx = torch.arange(nbh).view(-1, 1)
    lo = bx * S + torch.arange(4).view(1, -1) * SW
    hi = torch.minimum(torch.minimum(lo + SW, (bx + 1) * S), torch.tensor(cap))
    return torch.stack([lo, torch.maximum(hi, lo)], -1)


def shared_plan(Hq, Hkv, B, plen, smax):
    """shared_plan (csrc/decode_shared.hip)."""
    G = Hq // Hkv
    spg = min(32 // G, B)
    ngrp = (B + spg - 1) // spg
    nbs = min((smax + 255) // 256, 16)
    target = min(max(512 // (Hkv * ngrp), 8), 128 - nbs)
    per_block = (plen + target - 1) // target
    swp = 32 * ((per_block + 127) // 128)
    nbp = (plen + 4 * swp - 1) // (4 * swp)
    return dict(G=G, spg=spg, ngrp=ngrp, nbs=nbs, nbp=nbp, swp=swp)


def prefix_waves(plen, swp, nbp):
    """int64 [nbp, 4, 2]: prefix_block's wlo and whi (csrc/decode_shared.hip)."""
    lo = (torch.arange(nbp).view(-1, 1) * 4 + torch.arange(4).view(1, -1)) * swp
    hi = torch.minimum(lo + swp, torch.tensor(plen))
    return torch.stack([lo, torch.maximum(hi, lo)], -1)


def shared_waves(Hq, Hkv, B, plen, smax):
    """The waves of one slot of g2v_decode_attn_shared over the keys [prefix | suffix capacity]: the prefix blocks, then the
    suffix blocks (decode_attn_pg_body on suffix_max_len with nbs blocks: g2v_decode_attn_shared's S and (S + 3) / 4)."""
    p = shared_plan(Hq, Hkv, B, plen, smax)
    return torch.cat([prefix_waves(plen, p["swp"], p["nbp"]), pg_waves(smax, p["nbs"]) + plen])


def gen1_waves(cap):
    """decode_attn_kernel (csrc/decode.hip): one wave per 64-key chunk, four chunks per block."""
    nch = (cap + DCH - 1) // DCH
    nblk = (nch + 3) // 4
    lo = torch.arange(nblk * 4).view(nblk, 4) * DCH
    hi = torch.minimum(lo + DCH, torch.tensor(cap))
    return torch.stack([lo, torch.maximum(hi, lo)], -1)


def key_map(waves, n, kb=KB):
    """(wave index, batch index inside the wave, batch ordinal over the cache) of keys [0, n)."""
    wave = torch.zeros(n, dtype=torch.int64)
    batch = torch.zeros(n, dtype=torch.int64)
    for i, (lo, hi) in enumerate(waves.reshape(-1, 2).tolist()):
        hi = min(hi, n)
        if lo < hi:
            wave[lo:hi] = i
            batch[lo:hi] = (torch.arange(lo, hi) - lo) // kb
    nbmax = int(batch.max()) + 1 if n else 1
    order = wave * nbmax + batch
    gb = torch.unique(order, return_inverse=True)[1] if n else order
    return wave, batch, gb


def batch_counts(waves, n, kb=KB):
    """Sorted list of the distinct batch counts of the non-empty waves of a slot of n keys."""
    w = waves.reshape(-1, 2)
    k = (w[:, 1].clamp(max=n) - w[:, 0]).clamp(min=0)
    return sorted(set(((k[k > 0] + kb - 1) // kb).tolist()))


# ------------------------------------------------------------------------------------------------ reference and bounds
def attention64(q, K, V, Hkv):
    """fp64 softmax attention of one query token with the bounds' sums: q [Hq, 128], K / V [L, Hkv, 128] -> (want, T, Q), each
    [Hq, 128]: T_d = sum_j p_j |v_jd|, Q_d = sum_j p_j^2 v_jd^2 with p the normalised weights."""
    Hq = q.shape[0]
    G = Hq // Hkv
    want, T, Q = (torch.empty((Hq, 128), dtype=torch.float64) for _ in range(3))
    for h in range(Hkv):
        sl = slice(h * G, (h + 1) * G)
        p = torch.softmax((q[sl].double() @ K[:, h].double().T) * SCALE, dim=-1)
        v = V[:, h].double()
        want[sl], T[sl], Q[sl] = p @ v, p @ v.abs(), (p * p) @ (v * v)
    return want, T, Q


def hard_bound(want, T):
    return HARD_FACTOR * U * (T + want.abs())


def sharp_bound(want, Q):
    return 6.0 * SIGMA_UNIT * Q.sqrt() + 2.0 * U * want.abs()


def abs_dot(q, K, Hkv):
    """A of the first-generation bounds: max over heads and keys of scale sum_i |q_i k_ji|."""
    Hq = q.shape[0]
    G = Hq // Hkv
    return max(float((q[h * G:(h + 1) * G].double().abs() @ K[:, h].double().abs().T).max()) for h in range(Hkv)) * SCALE


def hard_bound1(want, T, A):
    return U * want.abs() + (1 + U) * 2.0 ** -24 * (20 * A + 52) * (T + want.abs())


def sharp_bound1(want, Q, A):
    return U * want.abs() + 6.0 * 2.0 ** -24 * (20 * A + 52) / math.sqrt(3.0) * Q.sqrt() + 2.0 ** -24 * 64 * want.abs()


class Ratios:
    """Worst |err| / bound per (kernel, family) and the count of elements over a bound."""

    def __init__(self):
        self.worst = {}

    def add(self, name, got, want, hard, sharp=None):
        got = got.detach().cpu().double()
        err = (got - want).abs()
        finite = bool(torch.isfinite(got).all())

        def ratio(b):
            r = torch.where(err == 0, torch.zeros_like(err), err / b)
            return (float(r.max()), int((~(err <= b)).sum())) if finite else (float("inf"), int(err.numel()))
        rh, nh = ratio(hard)
        rs, ns = ratio(sharp) if sharp is not None else (0.0, 0)
        w = self.worst.setdefault(name, dict(hard=0.0, sharp=0.0, over_hard=0, over_sharp=0, n=0))
        w["hard"], w["sharp"] = max(w["hard"], rh), max(w["sharp"], rs)
        w["over_hard"] += nh; w["over_sharp"] += ns; w["n"] += err.numel()
        return rh, rs, nh, ns

    def report(self, tag):
        for k, w in sorted(self.worst.items()):
            print(f"[{tag}] {k}: |err| / hard {w['hard']:.3f}  |err| / sharp {w['sharp']:.3f}  over {w['over_hard']} + {w['over_sharp']} of {w['n']}")


def check_slot(ratios, name, family, got, q, K, V, Hkv, gen1=False):
    """got [Hq, 128] against fp64 attention of q over K / V [L, Hkv, 128] under both bounds; returns the elements over a bound."""
    want, T, Q = attention64(q, K, V, Hkv)
    if gen1:
        A = abs_dot(q, K, Hkv)
        hard, sharp = hard_bound1(want, T, A), sharp_bound1(want, Q, A)
    else:
        hard, sharp = hard_bound(want, T), sharp_bound(want, Q)
    rh, rs, nh, ns = ratios.add(name, got, want, hard, sharp if family in NOISY else None)
    return nh + ns


# ------------------------------------------------------------------------------------------------ builders
def scores_log2(q, K):
    """fp64 [G, n]: the scores of q [G, 128] over K [n, 128] in log2 units."""
    return (q.double() @ K.double().T) * C2


def direction(q, only=None):
    """Unit fp64 [128] along the mean of q's heads; `only` (bool [G]): along the mean of those heads, orthogonal to the others."""
    qd = q.double()
    if only is None:
        d = qd.mean(0)
    else:
        d = qd[only].mean(0)
        Qo, _ = torch.linalg.qr(qd[~only].T)                 # [128, r]
        d = d - Qo @ (Qo.T @ d)
    return d / d.norm()


def streaming_wave(waves, n):
    """Index (over the flattened waves) of the middle one of the waves that stream more than one batch in a slot of n keys;
    of the non-empty waves if none does."""
    w = waves.reshape(-1, 2)
    cnt = (w[:, 1].clamp(max=n) - w[:, 0]).clamp(min=0)
    cand = torch.nonzero(cnt > KB).flatten()
    if cand.numel() == 0:
        cand = torch.nonzero(cnt > 0).flatten()
    return int(cand[cand.numel() // 2])


def peak_position(pos, n_cached, waves, n):
    """Cached-row index of a named position in a slot of n keys (n - 1 cached), or None if the slot is too short for it."""
    w = waves.reshape(-1, 2)
    if n_cached < 1:
        return None
    if pos == "row0":
        return 0
    if pos == "last":
        return n_cached - 1
    if pos in ("batch_end", "batch_start"):
        lo, hi = w[streaming_wave(w, n)].tolist()
        j = lo + KB - 1 if pos == "batch_end" else lo + KB
        return j if j < min(hi, n_cached) else None
    if pos == "wave3":                                       # wave 3 of the last block that has one within the cached rows
        for i in range(w.shape[0] // 4 - 1, -1, -1):
            lo, hi = w[4 * i + 3].tolist()
            if lo < min(hi, n_cached):
                return (lo + min(hi, n_cached) - 1) // 2
        return None
    return None


class Slot:
    """The cached rows of one (slot, kv head) and what the builder asserted about them."""

    def __init__(self, K, V, info):
        self.K, self.V, self.info = K, V, info


def _round(x, quant):
    x = x.float().bfloat16()
    return quant(x) if quant is not None else x


def build_slot(family, param, q, n, waves, gen, pos="row0", knew=None, quant=None, d=None, sign=1.0, pmin=None, kb=KB, offset=0, extra_top=None):
    """K, V bf16 [n - 1, 128] of the cached rows of one (slot, kv head) for normalised, rotated q bf16 [G, 128] and n keys
    including the new token's (its K row, as the kernel will append it: knew [128], needed by peak at 'new').  waves: the plan's
    wave ranges over the capacity; keys [offset, offset + n - 1) of them are built (the suffix of a shared-prefix slot).  quant:
    rows -> rows as the cache stores them (the e4m3 round trip).  d / sign / pmin: a given direction, the sign of this slot's q
    along it and the smallest |projection| (the shared prefix); by default the group's own mean q.  Asserts the profile."""
    G, nc = q.shape[0], n - 1
    info = dict(family=family, param=param, pos=None, exact=False)
    noise = torch.randn((max(nc, 1), 128), generator=gen)[:nc]
    V = _round(torch.randn((max(nc, 1), 128), generator=gen)[:nc], quant)
    if nc == 0:
        return Slot(torch.empty((0, 128), dtype=torch.bfloat16), V, info)
    if family == "flat":
        K = _round(noise[:1].expand(nc, 128).contiguous(), quant)
        s = scores_log2(q, K)
        assert bool((s == s[:, :1]).all()), "flat: the scores of a head differ"
        return Slot(K, V, info)
    only = None
    if family == "saw_even":
        only = torch.arange(G) % 2 == 0
        assert G >= 2
    if d is None:
        d = direction(q, only)
    proj = q.double() @ d                                    # [G]
    seen = only if only is not None else torch.ones(G, dtype=torch.bool)
    assert bool((sign * proj[seen] > 0).all()), "a head's q points against the profile direction"
    if pmin is None:
        pmin = float(proj[seen].abs().min())
    rho = proj / pmin                                        # signed: the level head h sees is rho_h L
    assert float(rho[seen].abs().min()) >= 1 - 1e-9
    wave, batch, gb = (t[offset:offset + nc] for t in key_map(waves, offset + nc, kb))
    gb = gb - gb.min()

    def rows(L, nz=noise):
        return _round(nz + (L / (pmin * C2)).float().unsqueeze(1) * d.float().unsqueeze(0), quant)

    if family == "peak":
        j = peak_position(pos, nc, (waves - offset).clamp(min=0), n)
        if pos == "new":
            # the new token's row holds >= 0.99 of every head's weight and lies param above every other score
            assert knew is not None
            nz = noise * 0.25
            s_new = scores_log2(q, knew.view(1, 128))[:, 0]
            s_nz = scores_log2(q, _round(nz, quant)).amax(1)
            assert sign > 0
            L0 = min(float(((s_new - param - math.log2(max(nc, 1)) - 8.0 - s_nz)[seen] / rho[seen]).min()), 0.0)
            K = rows(torch.full((nc,), L0, dtype=torch.float64), nz)
            s = scores_log2(q, K)
            gap = s_new - s.amax(1)
            assert bool((gap >= param).all()), ("peak at the new row", gap.tolist())
            share = 1.0 / (1.0 + torch.exp2(s - s_new.unsqueeze(1)).sum(1))
            assert bool((share >= 0.99).all()), share.tolist()
            noise_ok(s - s.mean(1, keepdim=True), "peak new")
            info.update(pos="new", exact=param >= EXACT_DELTA, peak=nc)
            return Slot(K, V, info)
        if j is None:
            j = 0
        L = torch.zeros(nc, dtype=torch.float64)
        K = rows(L)
        rest = torch.ones(nc, dtype=torch.bool); rest[j] = False
        s = scores_log2(q, K)
        s_new = scores_log2(q, knew.view(1, 128))[:, 0] if knew is not None else torch.full((G,), -1e30, dtype=torch.float64)
        top = torch.maximum(s[:, rest].amax(1) if nc > 1 else s_new, s_new)
        if extra_top is not None:
            top = torch.maximum(top, extra_top)
        Lp = float(((param + top)[seen] / rho[seen].abs()).max()) + 0.25
        for _ in range(6):                                   # the rounding (e4m3: 2^-4 per element) moves the peak's score
            K[j] = rows(torch.tensor([Lp * float(sign)], dtype=torch.float64), torch.zeros(1, 128))[0]
            gap = scores_log2(q, K[j:j + 1])[:, 0] - top
            if bool((gap >= param).all()):
                break
            Lp += float((param - gap).max()) + 0.5
        assert bool((gap >= param).all()), ("peak", pos, gap.tolist())
        assert float(gap.min()) <= param + 0.08 * Lp + 2.0, ("peak higher than promised", float(gap.min()))
        if nc > 17:
            noise_ok(s[:, rest] - s[:, rest].mean(1, keepdim=True), "peak")
        info.update(pos=pos, exact=param >= EXACT_DELTA, peak=j)
        return Slot(K, V, info)

    L = levels(family, param, wave, batch, gb, gen) * float(sign)     # a slot whose q points against d gets its profile through -L
    K = rows(L)
    if family == "offset":                                   # the rounding of the rows (e4m3: 2^-4 per element) may cost a head a few units
        low = float((scores_log2(q, K).mean(1).abs() / rho.abs()).min())
        if low < abs(param) * 0.99:
            K = rows(L * (abs(param) / low * 1.01))
    assert_profile(family, param, scores_log2(q, K), L * float(sign), rho.abs(), seen)
    info.update(levels=L * float(sign))
    return Slot(K, V, info)


def levels(family, param, wave, batch, gb, gen):
    """fp64 [n]: the nominal level of every key in log2 units, from its wave, its batch inside the wave and its batch ordinal."""
    n = wave.numel()
    if family in ("saw", "saw_even"):                        # a plan of one batch per wave: the teeth are the blocks, a step per wave
        return param * (batch if int(batch.max()) > 0 else wave % 4).double()
    if family == "rise":
        return param * gb.double()
    if family == "fall":
        return -param * gb.double()
    if family == "wide":
        nw = int(wave.max()) + 1
        return param * 0.5 * ((2 * torch.rand(nw, generator=gen, dtype=torch.float64) - 1)[wave]
                              + 2 * torch.rand(n, generator=gen, dtype=torch.float64) - 1)
    if family == "offset":
        return torch.full((n,), param, dtype=torch.float64)
    if family in ("gauss", "peak"):
        return torch.zeros(n, dtype=torch.float64)
    raise ValueError(family)


def noise_ok(res, what, level=0.0):
    """The score noise of a head is at least NOISE_MIN log2 units and stays noise: Gaussian rows give 1.44, the rounding of a
    row at level L adds up to 2^-4 L per element in e4m3 (2^-9 L in bf16), some 3 % of L over a row."""
    sd = float(res.std()) if res.numel() > 16 else 1.0
    assert NOISE_MIN <= sd <= 6.0 + 0.03 * level, f"{what}: score noise {sd:.3f} log2 units"


def assert_profile(family, param, s, Ls, rho, seen):
    """s fp64 [G, n]: the scores every head actually sees; Ls [n]: the level promised at rho = 1; rho [G] >= 1 for the heads
    in `seen`, which see rho_h Ls + noise (slope by least squares, up to its own standard error), the others noise alone."""
    G, n = s.shape
    for h in range(G):
        r = float(rho[h]) if bool(seen[h]) else 0.0
        res = s[h] - r * Ls
        noise_ok(res - res.mean(), f"{family} head {h}", float(Ls.abs().max()) * max(r, 1.0))
        if family == "offset":
            m = float(s[h].mean())
            assert m * math.copysign(1.0, float(Ls[0])) >= abs(param) * 0.98, (family, h, m)
        elif family not in ("gauss", "peak") and n >= 64 and float(Ls.std()) > 0:
            Lc = Ls - Ls.mean()
            slope = float((Lc * (s[h] - s[h].mean())).sum() / (Lc * Lc).sum())
            tol = 0.02 + 5.0 * float(res.std()) / (math.sqrt(n) * float(Ls.std()))
            if bool(seen[h]):
                assert slope >= 1 - tol, (family, param, h, slope)
            else:
                assert abs(slope) <= tol, (family, param, h, slope)


def distinct_scales(K, quantiser):
    """Number of distinct e4m3 row scales of K bf16 [n, 128]."""
    return int(torch.unique(quantiser(K.reshape(-1, 128))[1]).numel())


# ------------------------------------------------------------------------------------------------ the core, emulated
FAULTS = ("skip_rescale", "l_only", "no_fold", "drop_key", "merge_one", "no_guard")
# two more, right in exact arithmetic and wrong only where fp32 overflows: no input with scores of order 1 can show them
UNSAFE = ("stale_max", "merge_max3")


def emulate(q, K, V, waves, fault=None):
    """out bf16 [G, 128] of decode_attn_pg_body + decode_combine_pg_kernel on q bf16 [G, 128], K / V bf16 [n, 128] (n includes
    the new row), waves [NBLK, 4, 2] by capacity: per wave and 32-key batch the running maximum per half-wave folded by the
    swap, alpha, l from the unrounded p, O from the bf16-rounded p in fp32 (attn_batch_step), the four-wave merge (merge_waves)
    and the combine over the blocks' partials.  fault: one of FAULTS, planted in ONE wave, streaming_wave(waves, n):
      skip_rescale  neither l nor O is rescaled at its second batch        l_only     l is rescaled at every batch, O never
      no_fold       the other half-wave's maximum is not folded in         drop_key   the last key of its first batch is masked
      merge_one     its neighbour's weight in the four-wave merge is 1       no_guard   merge_waves without the -inf guard (every block)
    and of UNSAFE, in every wave / block:
      stale_max     the running maximum keeps the first batch's value (p = 2^(s - m) is still consistent, but may overflow)
      merge_max3    merge_waves takes its reference M from waves 0 - 2 only (e^(wm - M) of wave 3 may overflow)"""
    f32 = torch.float32
    G, n = q.shape[0], K.shape[0]
    qf, Kf, Vf = q.float(), K.float(), V.float()
    nblk = waves.shape[0]
    lo = waves[..., 0].reshape(-1)
    hi = torch.maximum(waves[..., 1].reshape(-1).clamp(max=n), lo)
    W = lo.numel()
    scale = torch.tensor(SCALE, dtype=f32)
    c2 = scale * torch.tensor(LOG2E, dtype=f32)
    nb = int(((hi - lo + KB - 1) // KB).max())
    NEG = float("-inf")
    m = torch.full((W, G, 2), NEG, dtype=f32)
    l = torch.zeros((W, G, 2), dtype=f32)
    O = torch.zeros((W, G, 128), dtype=f32)
    half_d = (torch.arange(128) >> 2) & 1                    # the half-wave that holds row d of O^T (wave_result_to_lds)
    half_k = (torch.arange(KB) >> 2) & 1                     # ... and key k of a batch (attn_batch_step)
    at = torch.zeros(W, dtype=torch.bool)
    if fault is not None:
        at[streaming_wave(waves, n)] = True
    at3 = at.view(-1, 1, 1)
    for b in range(nb):
        idx = lo.view(-1, 1) + KB * b + torch.arange(KB).view(1, -1)
        valid = idx < hi.view(-1, 1)
        if fault == "drop_key" and b == 0:                   # nk one short where a second batch follows
            valid[at & ((hi - lo) > KB), KB - 1] = False
        live = valid.any(1)
        ii = idx.clamp(max=n - 1)
        S = torch.einsum("wkd,gd->wgk", Kf[ii], qf)
        S = torch.where(valid.unsqueeze(1), S, torch.tensor(NEG))
        rm = S.view(W, G, KB // 8, 2, 4).amax((2, 4))        # [W, G, 2]: the maximum over each half's keys
        fold = rm.amax(-1, keepdim=True).expand(W, G, 2)
        rm = torch.where(at3, rm, fold) if fault == "no_fold" else fold
        m_new = torch.maximum(m, rm)
        if fault == "stale_max" and b > 0:
            m_new = torch.where(torch.isfinite(m), m, m_new)
        if b > 0:
            alpha = torch.exp2((m - m_new) * c2)
            alpha = torch.where(live.view(-1, 1, 1), alpha, torch.ones_like(alpha))
            if fault == "skip_rescale" and b == 1:
                alpha = torch.where(at3, torch.ones_like(alpha), alpha)
            l = l * alpha
            O = O * (torch.where(at3, torch.ones_like(alpha), alpha) if fault == "l_only" else alpha)[..., half_d]
        mc = m_new * c2
        arg = (S.double() * c2.double() - mc[..., half_k].double()).float()          # fmaf: one rounding
        p = torch.where(valid.unsqueeze(1), torch.exp2(arg), torch.zeros((), dtype=f32))
        l = l + p.view(W, G, KB // 8, 2, 4).sum((2, 4))
        Vb = torch.where(valid.unsqueeze(-1), Vf[ii], torch.zeros((), dtype=f32))
        O = O + torch.einsum("wgk,wkd->wgd", p.bfloat16().float(), Vb)
        m = torch.where(live.view(-1, 1, 1), m_new, m)
    wm = (m[..., 0] * scale).view(nblk, 4, G)                # natural-log units, lanes hh == 0
    wl = l.sum(-1).view(nblk, 4, G)
    wo = O.view(nblk, 4, G, 128)
    M = wm.amax(1)
    if fault == "merge_max3":
        M3 = wm[:, :3].amax(1)
        f = torch.exp(wm - M3.unsqueeze(1))
        f = torch.where(wm == NEG, torch.zeros_like(f), f)
        Lp, Op = (wl * f).sum(1), (wo * f.unsqueeze(-1)).sum(1)
        M = M3
    f = torch.exp(wm - M.unsqueeze(1))
    if fault != "no_guard":
        f = torch.where(wm == NEG, torch.zeros_like(f), f)
    if fault == "merge_one":
        f = torch.where(at.view(nblk, 2, 2).flip(-1).reshape(nblk, 4, 1) & (wm != NEG), torch.ones_like(f), f)
    if fault != "merge_max3":
        Lp, Op = (wl * f).sum(1), (wo * f.unsqueeze(-1)).sum(1)  # [NBLK, G], [NBLK, G, 128]
    Mg = M.amax(0)
    fc = torch.where(M == NEG, torch.zeros_like(M), torch.exp(M - Mg))
    Lt, Ot = (Lp * fc).sum(0), (Op * fc.unsqueeze(-1)).sum(0)
    return (Ot / Lt.unsqueeze(-1)).bfloat16()


def emulate_gen1(q, K, V):
    """out bf16 [G, 128] of decode_attn_kernel + decode_combine_kernel (csrc/decode.hip): fp32 weights per 64-key chunk."""
    f32 = torch.float32
    n = K.shape[0]
    nch = (n + DCH - 1) // DCH
    S = (q.float() @ K.float().T) * torch.tensor(SCALE, dtype=f32)
    S = torch.nn.functional.pad(S, (0, nch * DCH - n), value=float("-inf")).view(-1, nch, DCH)
    Vp = torch.nn.functional.pad(V.float(), (0, 0, 0, nch * DCH - n)).view(nch, DCH, 128)
    mx = S.amax(-1)
    p = torch.exp(S - mx.unsqueeze(-1))
    o = torch.einsum("gck,ckd->gcd", p, Vp)
    f = torch.exp(mx - mx.amax(-1, keepdim=True))
    return ((o * f.unsqueeze(-1)).sum(1) / (p.sum(-1) * f).sum(1, keepdim=True)).bfloat16()


# ------------------------------------------------------------------------------------------------ a whole step
def slot_position(z, variant=0):
    return POSITIONS[(z + variant) % len(POSITIONS)]


def new_row_slots(case, lens, variant=0):
    """The slots whose peak sits in the new token's own row: their raw k is set to the group's mean raw q before the step."""
    if case[0] != "peak":
        return []
    return [z for z, n in enumerate(lens) if slot_position(z, variant) == "new" and n > 1]


def align_new_k(qkv, Hq, Hkv, slots):
    """qkv [B, (Hq + 2 Hkv) 128] (raw, in place): raw k of kv head h := mean raw q of its group, for the given slots."""
    G = Hq // Hkv
    v = qkv.view(qkv.shape[0], Hq + 2 * Hkv, 128)
    for z in slots:
        for h in range(Hkv):
            v[z, Hq + h] = v[z, h * G:(h + 1) * G].float().mean(0).to(v.dtype)
    return qkv


def build_step(case, qn, knew, lens, Hq, Hkv, waves, seed, variant=0, quant=None, kb=KB):
    """Cached rows of every slot of a per-scene cache step: lists K[z], V[z] bf16 [n_z - 1, Hkv, 128] and the Slot infos
    info[z][h].  qn bf16 [B, Hq 128] (cpu), knew bf16 [B, Hkv, 128]: the appended K rows as the cache will hold them."""
    family, param = case
    G = Hq // Hkv
    gen = torch.Generator(); gen.manual_seed(seed)
    Ks, Vs, infos = [], [], []
    for z, n in enumerate(lens):
        q = qn[z].view(Hq, 128)
        pos = slot_position(z, variant)
        if pos == "new" and n == 1:
            pos = "row0"
        kk, vv, ii = [], [], []
        for h in range(Hkv):
            par = -param if family == "offset" and (z + h) % 2 else param
            s = build_slot(family, par, q[h * G:(h + 1) * G], n, waves, gen, pos=pos, knew=knew[z, h], quant=quant, kb=kb)
            kk.append(s.K); vv.append(s.V); ii.append(s.info)
        Ks.append(torch.stack(kk, 1)); Vs.append(torch.stack(vv, 1)); infos.append(ii)
    return Ks, Vs, infos


# ------------------------------------------------------------------------------------------------ the shared prefix
SHARED_CASES = [("saw", 0.5), ("saw", 3.0), ("saw", 20.0), ("saw", 70.0), ("rise", 0.5), ("rise", 20.0), ("fall", 0.5), ("fall", 20.0),
                ("peak_prefix", 8.0), ("peak_prefix", 30.0), ("peak_prefix", 200.0), ("peak_suffix", 8.0), ("peak_suffix", 30.0),
                ("peak_suffix", 200.0), ("wide", 40.0), ("wide", 120.0), ("offset", 250.0), ("flat", 0.0)]


def slot_signs(B, spg):
    """+1 / -1 per slot, alternating inside every column group: neighbours in the MFMA's columns see mirrored profiles."""
    return [1.0 if (z % spg) % 2 == 0 else -1.0 for z in range(B)]


def shared_directions(Hkv, seed):
    """One unit direction per kv head, fixed before q exists: the prefix rows are shared, so the profile comes from q."""
    g = torch.Generator(); g.manual_seed(seed)
    d = torch.randn((Hkv, 128), generator=g, dtype=torch.float64)
    return d / d.norm(dim=1, keepdim=True)


def shared_targets(B, Hq, Hkv, d, signs, seed, along=4.6):
    """fp32 [B, Hq, 128]: what the normalised, rotated q of every slot should be: Gaussian rows whose component along d[kv head]
    is sign_z . along (the size the mean q of six Gaussian heads has along itself)."""
    g = torch.Generator(); g.manual_seed(seed)
    G = Hq // Hkv
    t = torch.randn((B, Hq, 128), generator=g, dtype=torch.float64)
    for h in range(Hq):
        dh = d[h // G]
        t[:, h] += (torch.tensor(signs, dtype=torch.float64) * along - t[:, h] @ dh).unsqueeze(1) * dh
    return t.float()


def build_shared(case, qn, knew, slen, Hq, Hkv, plen, smax, d, signs, seed):
    """Rows of a shared-prefix step: Kp, Vp bf16 [plen, Hkv, 128], lists Ks[z], Vs[z] [n_z - 1, Hkv, 128], and exact[z]: the
    output row of slot z must equal that V row (None otherwise).  The + slots see the family's profile, the - slots its mirror
    image; a suffix peak is every slot's own."""
    family, param = case
    B, G = len(slen), Hq // Hkv
    gen = torch.Generator(); gen.manual_seed(seed)
    waves = shared_waves(Hq, Hkv, B, plen, smax)
    q = qn.view(B, Hq, 128)
    sg = torch.tensor(signs, dtype=torch.float64)
    Kp = torch.empty((plen, Hkv, 128), dtype=torch.bfloat16)
    Vp = torch.randn((plen, Hkv, 128), generator=gen).bfloat16()
    Ks = [torch.empty((n - 1, Hkv, 128), dtype=torch.bfloat16) for n in slen]
    Vs = [torch.randn((max(n - 1, 1), Hkv, 128), generator=gen)[:n - 1].bfloat16() for n in slen]
    exact = [None] * B
    seen = torch.ones(G, dtype=torch.bool)
    fam = "peak" if family.startswith("peak") else family
    for h in range(Hkv):
        qh = q[:, h * G:(h + 1) * G].double()               # [B, G, 128]
        proj = qh @ d[h]                                     # [B, G]
        assert bool((proj * sg.view(-1, 1) > 0).all()), "a slot's q does not point along its sign"
        pmin = float(proj.abs().min())
        rho = proj.abs() / pmin
        wave, batch, gb = key_map(waves, plen)
        noise = torch.randn((plen, 128), generator=gen)
        if fam == "flat":
            row = noise[:1].bfloat16()
            Kp[:, h] = row
            for z, n in enumerate(slen):
                Ks[z][:, h] = row
            continue
        L = levels(fam, param, wave, batch, gb, gen)
        Kh = (noise + (L / (pmin * C2)).float().unsqueeze(1) * d[h].float()).bfloat16()
        if family == "peak_prefix":                          # wave 3 of a middle block, the first key of its second batch
            j = int(waves[waves.shape[0] // 4 // 2, 3, 0]) + KB
            rest = torch.ones(plen, dtype=torch.bool); rest[j] = False
            plus = [z for z in range(B) if signs[z] > 0]
            top = torch.stack([scores_log2(q[z, h * G:(h + 1) * G], Kh[rest]).amax(1) for z in plus])            # [+slots, G]
            top = torch.maximum(top, torch.tensor(4.0 * 1.5))  # the suffix rows and the new row are Gaussian: 4 sigma and more below
            Lp = float(((param + 6.0 + top) / rho[plus]).max())
            Kh[j] = ((Lp / (pmin * C2)) * d[h].float()).bfloat16()
        Kp[:, h] = Kh
        for z, n in enumerate(slen):
            qz = q[z, h * G:(h + 1) * G]
            sp = scores_log2(qz, Kh)
            nc = n - 1
            if family == "peak_suffix":
                top = torch.maximum(sp.amax(1), scores_log2(qz, knew[z, h].view(1, 128))[:, 0])
                if nc == 0:
                    continue
                s = build_slot("peak", param, qz, n, waves, gen, pos="last" if z % 2 else "row0", knew=knew[z, h], d=d[h],
                               sign=signs[z], pmin=pmin, offset=plen, extra_top=top)
                Ks[z][:, h] = s.K
                exact[z] = ("suffix", s.info["peak"]) if s.info["exact"] else None
                continue
            if nc:
                w2, b2, g2 = (t[plen:] for t in key_map(waves, plen + nc))
                g2 = g2 - g2.min() + int(gb.max()) + 1
                Lz = levels(fam, param, w2, b2, g2, gen)
                nz = torch.randn((nc, 128), generator=gen)
                Ks[z][:, h] = (nz + (Lz / (pmin * C2)).float().unsqueeze(1) * d[h].float()).bfloat16()
                sp = torch.cat([sp, scores_log2(qz, Ks[z][:, h])], 1)
                Lall = torch.cat([L, Lz])
            else:
                Lall = L
            if family == "peak_prefix":
                if signs[z] > 0:
                    s_new = scores_log2(qz, knew[z, h].view(1, 128))[:, 0]
                    keep = torch.ones(sp.shape[1], dtype=torch.bool); keep[j] = False
                    gap = sp[:, j] - torch.maximum(sp[:, keep].amax(1), s_new)
                    assert bool((gap >= param).all()), ("peak_prefix", z, gap.tolist())
                    if param >= EXACT_DELTA:
                        exact[z] = ("prefix", j)
                continue
            assert_profile(fam, param, sp, Lall * signs[z], rho[z], seen)
    return Kp, Vp, Ks, Vs, exact
