"""CPU: the launch table and the checks of tests/decode_check.py, before they are applied to the bf16 decode kernels on the GPU
(tests/test_decode_fp64_gpu.py).

1. Coverage.  Every persistent-grid row of decode_check.TABLE is routed with g2v_gemv_pg_route (no device) and the routes
   reached must be exactly: every batch depth of rbs() in csrc/decode_dispatch.h for bf16, each in one trip of the batch loop
   and, where the plan can produce it, in two or more trips ending in a ragged batch; every block size from 192 to 512; NB in
   {2, 4, 8} from B in {1, 2, 3, 4, 5, 7, 8}; the long-K batched form with 1, 2, 6 and 8 rows per block.  What the plan can
   not produce is listed in UNREACHABLE with the reason, and a scan of N confirms that it is not produced.
2. Honest fp32 emulations of the four summation orders (first generation, gemv_pg, gemv_pgb, gemv_pgk) and of the two fused
   norms pass every check with margin: zero flags, implied error below TAU / 4, norm error below a quarter of its bound.
   Measured here: largest implied error 1.0e-10 T (TAU / 4 = 3.8e-6; an output's bf16 rounding interval nearly always holds
   the fp64 value, which reads as 0), largest norm ratio 0.005, largest multi-valued share of a read-back norm 0.39 %.
3. Planted errors - each one a mistake these kernels could make at the depth and trip where it is possible - are flagged
   exactly where they were planted, and nowhere else.  OLD_ACCEPTS records, and the tests assert, whether the older
   comparisons of tests/test_kernels_gpu.py (assert_bf16_close with rl = 4e-3 and 2 ulps on 99.8 % of the elements; rel < 2e-3
   on a whole residual vector; per activation vector) accept the same output as planted, and whether they accept the same
   wrong elements among the 151 936 rows of the lm_head, the one shape at which the second trip ran before:
     dead chunk counted (one wave, K = 520)             rejected, rejected (the chunk is counted 127 times over)
     ragged batch shifted by one row (4 rows)           rejected at N = 6401, rejected
     bias of the next batch (5 rows)                    rejected at N = 6401, ACCEPTED among 151 936
     residual of the next scene (3 rows, 2 scenes)      rejected at N = 8193, rejected
     padding row stored                                 ACCEPTED: they never look behind the B rows
     gate and up swapped in one group of 16             rejected, rejected
     wave 7's K share dropped in 2 rows                 rejected at N = 300, ACCEPTED among 151 936
     rstd of row 0 for every row                        rejected (every element of a row moves)
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_check as D  # noqa: E402
import gemm_check as G  # noqa: E402
import rowop_check as R  # noqa: E402
from g2vlm_amd import hip  # noqa: E402
from g2vlm_amd.weights import interleave_gate_up  # noqa: E402

MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def measured():
    yield
    for k, v in sorted(MEASURED.items()):
        print(f"[decode check] {k}: {v}")


@pytest.fixture(scope="module")
def built():
    from g2vlm_amd import build
    build.build()
    return hip


# ------------------------------------------------------------------------------------------------ 1. coverage of the plan
# rbs() of csrc/decode_dispatch.h for bf16, by (scenes per pass NB - 0: the batch-1 entry, act, long K)
RBS = {(0, False, False): (1, 2, 3, 4, 5, 6, 8), (0, True, False): (1, 2, 3, 4, 5), (0, False, True): (1,),
       (2, False, False): (1, 2, 3, 5), (2, True, False): (1, 2, 3, 5), (4, False, False): (1, 2, 3), (4, True, False): (1, 2, 3),
       (8, False, False): (1, 2), (8, True, False): (1, 2)}
THREADS = (192, 256, 320, 384, 448, 512)
# (class, depth, 'ragged') the plan never produces: equal_batches() cuts a wave's units into ceil(per / cap) batches of
# ceil(per / batches), so a wave that needs a second trip runs at more than half of the cap (the last entry of the list)
_WHY = "two trips mean more than cap units per wave, and equal_batches() then picks a depth above cap / 2"
UNREACHABLE = {((0, False, False), d): _WHY for d in (1, 2, 3, 4)}
UNREACHABLE.update({((0, True, False), d): _WHY for d in (1, 2)})
UNREACHABLE.update({((nb, act, False), d): _WHY for nb in (2,) for act in (False, True) for d in (1, 2)})
UNREACHABLE.update({((nb, act, False), 1): _WHY for nb in (4, 8) for act in (False, True)})


def plan_py(B, N, K, act, norm):
    """pg::plan of csrc/decode_dispatch.h for bf16, transcribed: dict(form, threads, rb, kch, nb, uq, ur, per)."""
    def fit(l, x):
        return next((v for v in l if x <= v), l[-1])

    def equal_batches(per, cap):
        if per <= cap:
            return per
        nbat = -(-per // cap)
        return -(-per // nbat)

    if B == 0:
        longk = K > 1536
        l = RBS[(0, act, longk)]
        U = N // 2 if act else N
        small = N * K * 2.0 / 256.0 < 48.0 * 1024.0
        best, best_imb = 4, 1e30
        for t in range(6):
            nwb = 3 + t if small else 8 - t
            nw = 256 * nwb
            per = U / nw
            imb = (-(-U // nw)) / per if per >= 1.0 else 1.0 / per
            if small and -(-U // nw) > l[-1] and best_imb < 1e29:
                continue
            if imb < best_imb - 1e-9:
                best_imb, best = imb, nwb
        waves = 256 * best
        return dict(form=1, threads=64 * best, rb=fit(l, equal_batches(-(-U // waves), l[-1])), kch=18 if longk else 3, nb=0,
                    uq=U // waves, ur=U % waves, per=0)
    nb = fit((2, 4, 8), B)
    if K > 1536:
        return dict(form=3, threads=512, rb=6, kch=(K // 8 + 7) // 8, nb=nb, uq=0, ur=0, per=(N + 255) // 256)
    l = RBS[(nb, act, False)]
    U = N // 2 if act else N
    uq, ur = divmod(U, 2048)
    return dict(form=2, threads=512, rb=fit(l, equal_batches(uq + (1 if ur else 0), l[-1])), kch=3, nb=nb, uq=uq, ur=ur, per=0)


def wave_units(p, gw):
    lo = gw * p["uq"] + min(gw, p["ur"])
    return lo, lo + p["uq"] + (1 if gw < p["ur"] else 0)


def trips(p):
    """The kinds of wave a launch has: 'one' (all its units in one batch), 'ragged' (two or more trips, the last one short),
    'even' (two or more full trips)."""
    waves = 256 * p["threads"] // 64
    sizes = set()
    if p["ur"]:
        sizes.add(p["uq"] + 1)
    if p["uq"] and p["ur"] < waves:
        sizes.add(p["uq"])
    return {"one" if s <= p["rb"] else ("ragged" if s % p["rb"] else "even") for s in sizes}


def reached(rows, h):
    out = dict(depth=set(), threads=set(), nb_b=set(), per=set())
    for row in rows:
        B, N, K, act, norm, fp8 = D.route_args(row)
        p = plan_py(B, N, K, act, norm)
        assert h.gemv_pg_route(B, N, K, act, norm, False) == (p["form"], p["threads"], p["rb"], p["kch"]), row
        if p["form"] == 3:
            out["per"].add(p["per"])
            assert p["kch"] <= 192 and 8 * p["kch"] >= K // 8, row          # a wave holds 3 x 64 chunks; 8 waves cover K
        else:
            cls = (p["nb"], bool(act), K > 1536)
            assert p["rb"] in RBS[cls], row
            for kind in trips(p):
                out["depth"].add((cls, p["rb"], kind))
            if p["form"] == 1:
                out["threads"].add(p["threads"])
        if B:
            out["nb_b"].add((p["nb"], B))
    return out


def test_the_table_reaches_every_depth_block_size_nb_and_pass_count(built):
    rows = [r for r in D.TABLE if r[0] in ("pg", "pgb")]
    got = reached(rows, built)
    want = set()
    for cls, depths in RBS.items():
        for d in depths:
            want.add((cls, d, "one"))
            if cls[2]:
                want.add((cls, d, "even"))                          # long K: one row per batch, trips are never ragged
            elif (cls, d) not in UNREACHABLE:
                want.add((cls, d, "ragged"))
    have = {k for k in got["depth"] if k[2] != "even" or k[0][2]}
    assert have == want, (sorted(want - have), sorted(have - want))
    assert got["threads"] == set(THREADS)
    assert {nb for nb, B in got["nb_b"]} == {2, 4, 8} and {B for nb, B in got["nb_b"]} == {1, 2, 3, 4, 5, 7, 8}
    assert got["per"] >= {1, 2, 6, 8}
    for K in (8, 256, 512, 520, 1528, 1536, 1544, 2064, 8960, 9216, 12288):
        assert any(r[4] == K for r in rows), K
    for entry in ("pg", "pgb", "g1"):
        assert {(f, N, K) for e, f, B, N, K in D.TABLE if e == entry} >= set(D.PRODUCTION), entry
    big = [r for r in D.TABLE if r[3] * r[4] * 2 > 64e6 and (r[1], r[3], r[4]) not in D.PRODUCTION]
    assert not big, big


def test_what_is_listed_as_unreachable_is_never_planned(built):
    """Every N up to 70 000 (act: every multiple of 32) at a short and a streaming K, through the route call."""
    seen = set()
    for (nb, act, longk) in RBS:
        if longk:
            continue
        B = {0: 0, 2: 2, 4: 3, 8: 8}[nb]
        for K in (256, 1536):
            for N in range(32 if act else 1, 70000, 32 if act else 1):
                form, threads, rb, kch = built.gemv_pg_route(B, N, K, act, act, False)
                U = N // 2 if act else N
                waves = 256 * threads // 64
                p = dict(threads=threads, rb=rb, uq=U // waves, ur=U % waves)
                seen |= {((nb, act, False), rb, k) for k in trips(p)}
    for (cls, d), why in UNREACHABLE.items():
        assert (cls, d, "ragged") not in seen, (cls, d)
        assert (cls, d, "one") in seen
    for cls, depths in RBS.items():
        if not cls[2]:
            assert {d for d in depths if (cls, d, "ragged") in seen} == {d for d in depths if (cls, d) not in UNREACHABLE}, cls


# ------------------------------------------------------------------------------------------------ 2. honest emulations
def rnd(*shape, seed=0, scale=1.0):
    return D.rnd(*shape, seed=seed, scale=scale)


def lane_tables(kind, K):
    """idx [S, 64, J] of 16-byte chunk numbers (-1: none) in the order a lane accumulates them, S = the shares added after the
    lane sums: 'g1' 4 waves of a 256-thread block, thread t takes chunks t, t + 256, ..; 'pg' / 'pgb' one wave, lane l takes
    l, l + 64, ..; 'pgk' 8 waves, wave w the chunks [w CW, (w + 1) CW), lane l takes w CW + l + 64 j, j < 3."""
    nch = K // 8
    if kind == "g1":
        J = -(-nch // 256)
        c = torch.arange(256).view(4, 64, 1) + 256 * torch.arange(J).view(1, 1, J)
        return torch.where(c < nch, c, -1)
    if kind in ("pg", "pgb"):
        J = 18 if K > 1536 else 3
        c = torch.arange(64).view(1, 64, 1) + 64 * torch.arange(J).view(1, 1, J)
        return torch.where(c < nch, c, -1)
    CW = (nch + 7) // 8
    w = torch.arange(8).view(8, 1, 1)
    c = w * CW + torch.arange(64).view(1, 64, 1) + 64 * torch.arange(3).view(1, 1, 3)
    return torch.where((c < (w + 1) * CW) & (c < nch), c, -1)


def butterfly(v, masks):
    """Sum over dim 1 (64 lanes) by xor exchanges in the given order; lane 0's total."""
    lanes = torch.arange(64)
    for m in masks:
        v = v + v[:, lanes ^ m]
    return v[:, 0]


def lane_sum(v, kind):
    if kind == "pg":                                            # wave_sum_dpp: rows of 16 by xor 8, 4, 2, 1, then (r0 + r1) + (r2 + r3)
        lanes = torch.arange(64)
        for m in (8, 4, 2, 1):
            v = v + v[:, lanes ^ m]
        return (v[:, 0] + v[:, 16]) + (v[:, 32] + v[:, 48])
    return butterfly(v, (32, 16, 8, 4, 2, 1))                  # wave_sum / reduce_transpose


def emulate(kind, X, W, mask_dead=True, drop_share=None, exact=True):
    """fp32 [B, N] accumulation of X bf16 [B, K] . W bf16 [N, K]^T in the summation order of `kind`.  exact: every product is
    added in the kernel's order (pairs for v_dot2, singly for the fmaf chain); else a lane's terms are summed by one matmul."""
    B, K = X.shape
    N = W.shape[0]
    nch = K // 8
    idx = lane_tables(kind, K)
    S, _, J = idx.shape
    live = (idx >= 0)
    ci = torch.where(live, idx, nch - 1)                        # the kernels clamp the address and mask the value
    xc, wc = X.float().view(B, nch, 8), W.float().view(N, nch, 8)
    acc = torch.zeros((S, 64, B, N))
    for j in range(J):
        x = xc[:, ci[:, :, j]].permute(1, 2, 0, 3)              # [S, 64, B, 8]
        w = wc[:, ci[:, :, j]].permute(1, 2, 0, 3)              # [S, 64, N, 8]
        if mask_dead:
            x = x * live[:, :, j, None, None]
        if exact:
            prod = x[:, :, :, None, :] * w[:, :, None, :, :]
            if kind == "g1":
                for e in range(8):
                    acc = acc + prod[..., e]
            else:
                for e in range(4):
                    acc = acc + (prod[..., 2 * e] + prod[..., 2 * e + 1])
        else:
            acc = acc + torch.matmul(x, w.transpose(2, 3))
    s = lane_sum(acc.view(S, 64, B * N), kind).view(S, B, N)
    if kind == "g1":
        return (s[0] + s[1]) + (s[2] + s[3])
    if kind == "pgk":
        t = torch.zeros((B, N))
        for k in range(8):
            if k != drop_share:
                t = t + s[k]
        return t
    return s[0]


def emulate_norm(kind, x, nw, rstd_row=None):
    """bf16 [B, K]: the fused RMSNorm in fp32.  'g1': thread t of 256 sums the float4s at 4 t + 1024 i as (v0^2 + v1^2) + (v2^2 +
    v3^2), wave sums, four waves through LDS; 'pg': lane l sums its chunks l + 64 j, x[e]^2 + x[4 + e]^2 per step, wave_sum_dpp."""
    B, K = x.shape
    x = x.float()
    if kind == "g1":
        n4 = K // 4
        J = -(-n4 // 256)
        c = torch.arange(256).view(256, 1) + 256 * torch.arange(J).view(1, J)
        v = torch.cat([x.view(B, n4, 4), torch.zeros(B, 1, 4)], 1)[:, torch.where(c < n4, c, n4)]       # [B, 256, J, 4]
        ss = torch.zeros(B, 256)
        for j in range(J):
            q = v[:, :, j] * v[:, :, j]
            ss = ss + ((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3]))
        s = butterfly(ss.view(B, 4, 64).permute(1, 2, 0), (32, 16, 8, 4, 2, 1))                         # [4, B]
        tot = (s[0] + s[1]) + (s[2] + s[3])
    else:
        nch = K // 8
        c = torch.arange(64).view(64, 1) + 64 * torch.arange(3).view(1, 3)
        v = torch.cat([x.view(B, nch, 8), torch.zeros(B, 1, 8)], 1)[:, torch.where(c < nch, c, nch)]    # [B, 64, 3, 8]
        ss = torch.zeros(B, 64)
        for j in range(3):
            q = v[:, :, j] * v[:, :, j]
            for e in range(4):
                ss = ss + (q[..., e] + q[..., 4 + e])
        tot = lane_sum(ss.t().reshape(1, 64, B), "pg")[0]
    rstd = 1.0 / torch.sqrt(tot / float(K) + torch.tensor(D.EPS, dtype=torch.float32))
    if rstd_row is not None:
        rstd = rstd[rstd_row].expand(B)
    return (nw.float()[None] * (x * rstd[:, None])).bfloat16()


def epilogue(form, acc, bias, res0):
    """The kernels' rounding points on fp32 accumulations acc [B, N]."""
    if form == "gu":
        a = acc.view(acc.shape[0], -1, 2, 16)
        g, u = a[:, :, 0].reshape(acc.shape[0], -1).bfloat16().float(), a[:, :, 1].reshape(acc.shape[0], -1).bfloat16().float()
        return (torch.nn.functional.silu(g).bfloat16().float() * u).bfloat16()
    v = (acc + (bias.float()[None] if bias is not None else 0.0)).bfloat16()
    return res0 + v.float() if res0 is not None else v


class CpuCase:
    """decode_check.Case's operands on the CPU (the weight drawn here)."""

    def __init__(self, form, B, N, K, seed):
        self.form, self.B, self.N, self.K = form, B, N, K
        self.norm, self.act = form in D.NORM_FORMS, form == "gu"
        w = rnd(N, K, seed=seed, scale=K ** -0.5)
        if self.act:
            w = interleave_gate_up(w[:N // 2].contiguous(), w[N // 2:].contiguous())
        self.wd = w.bfloat16()
        self.bias = rnd(N, seed=seed + 1, scale=0.1).bfloat16() if form in ("qkv", "bias") else None
        self.nw = 1 + 0.1 * rnd(K, seed=seed + 2) if self.norm else None
        self.x = rnd(B, K, seed=seed + 3) if self.norm else rnd(B, K, seed=seed + 3).bfloat16()
        self.res0 = rnd(B, N, seed=seed + 4) if form in D.RES_FORMS else None

    def check(self, got, A):
        epi = G.EPI_SWIGLU if self.act else (G.EPI_RES_F32 if self.res0 is not None else G.EPI_BF16)
        return G.check_gemm(got, A, self.wd, self.bias, epi, res=self.res0)


TABLE_K = sorted({r[4] for r in D.TABLE})
KINDS = {"g1": lambda K: True, "pg": lambda K: K <= 9216, "pgb": lambda K: K <= 1536, "pgk": lambda K: 1536 < K <= 12288}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_honest_emulations_pass_with_margin(kind):
    worst_d, worst_norm, worst_multi = 0.0, 0.0, 0.0
    for K in TABLE_K:
        if not KINDS[kind](K):
            continue
        for form in ("bias", "o", "qkv", "gu"):
            if form in D.NORM_FORMS and (K > 1536 or kind == "pgk"):
                continue
            B, N = 8, 64
            c = CpuCase(form, B, N, K, seed=K + len(form))
            A = c.x
            if c.norm:
                A = emulate_norm("g1" if kind == "g1" else "pg", c.x, c.nw)
                r = D.check_norm(A, c.x, c.nw)
                assert r.count == 0, r.report(what=f"norm {kind} K={K}")
                worst_norm = max(worst_norm, r.max_ratio)
                worst_multi = max(worst_multi, r.multi_share)
                assert r.multi_share <= R.MULTI_CAP
            got = epilogue(form, emulate(kind, A, c.wd), c.bias, c.res0)
            chk = c.check(got, A)
            assert chk.count == 0, chk.report(what=f"{kind} {form} K={K}")
            worst_d = max(worst_d, chk.max_d)
            if c.act:
                assert chk.max_ulps <= G.ULP_BOUND[G.EPI_SWIGLU]
    MEASURED[f"honest {kind}"] = f"implied error {worst_d:.2e} T (TAU {G.TAU:.2e}), norm ratio {worst_norm:.3f}, multi {worst_multi:.2%}"
    assert worst_d < G.TAU / 4 and worst_norm < 0.25


def test_the_norm_operands_of_the_table_stay_under_the_multi_cap():
    """The share of multi-valued elements is a property of the reference and the operands alone, so every fused-norm row of
    the table is checked here, with the operands the GPU test will draw: the emulated readback has zero flags and the share is
    under MULTI_CAP (the smallest case has 64 elements: one multi-valued element is 1.6 %, two would fail)."""
    worst = 0.0
    for row in D.TABLE:
        entry, form, B, N, K = row
        if form not in D.NORM_FORMS:
            continue
        seed = D.case_seed(row)
        nw, x = 1 + 0.1 * rnd(K, seed=seed + 2), rnd(B, K, seed=seed + 3)
        r = D.check_norm(emulate_norm("g1" if entry == "g1" else "pg", x, nw), x, nw)
        assert r.count == 0, row
        worst = max(worst, r.multi_share)
        assert r.multi_share <= R.MULTI_CAP, (row, r.multi_share)
    MEASURED["table norms"] = f"largest multi-valued share {worst:.2%}"


# ------------------------------------------------------------------------------------------------ 3. planted errors
LM_ROWS = 151936


def old_accepts(got, ref, res0=None, at_rows=None):
    """Would tests/test_kernels_gpu.py have accepted `got`?  Per activation vector, as those tests run: assert_bf16_close(rl =
    4e-3, ulps = 2.0) on a bf16 output, rel < 2e-3 on a whole residual vector; ref = the fp32 Linear on the bf16 operands.
    at_rows: the same wrong elements among that many rows of the same rms instead (rel scales with sqrt(N / at_rows), the
    share of elements off by more than 2 ulps with N / at_rows)."""
    N = got.shape[1]
    sc = 1.0 if at_rows is None else N / at_rows
    for b in range(got.shape[0]):
        g, r = got[b].float(), ref[b].float()
        rel = float((g - r).double().norm() / (r.double().norm() + 1e-30)) * sc ** 0.5
        if res0 is not None:
            if not rel < 2e-3:
                return False
        else:
            tol = 2.0 * 2.0 ** -8 * r.abs().clamp_min(r.abs().max() * 2 ** -7)
            if not (torch.isfinite(g).all() and rel < 4e-3 and float(((g - r).abs() > tol).float().mean()) * sc < 2e-3):
                return False
    return True


# name -> (the older comparison accepts the planted output, it accepts the same wrong elements in an lm_head-sized output)
OLD_ACCEPTS = {"dead chunk": (False, False), "ragged shifted": (False, False), "next bias": (False, True),
               "next scene residual": (False, False), "padding row": (True, True), "gate/up swapped": (False, False),
               "wave 7 dropped": (False, True), "rstd of row 0": (False, False)}
SEEN = {}


def cols(chk):
    return sorted(set(chk.bad.any(0).nonzero().flatten().tolist()))


def finish(name, c, got, A, want_cols, want_rows=None):
    chk = c.check(got, A)
    assert cols(chk) == list(want_cols), (name, cols(chk)[:20], list(want_cols)[:20])
    if want_rows is not None:
        assert chk.flagged_rows() == list(want_rows), (name, chk.flagged_rows())
    ref = torch.nn.functional.linear(A.float(), c.wd.float(), c.bias.float() if c.bias is not None else None)
    if c.act:
        r = ref.view(c.B, -1, 2, 16)
        ref = (torch.nn.functional.silu(r[:, :, 0]) * r[:, :, 1]).reshape(c.B, -1)
    if c.res0 is not None:
        ref = c.res0 + ref
    SEEN[name] = (old_accepts(got, ref, c.res0), old_accepts(got, ref, c.res0, at_rows=LM_ROWS))
    MEASURED["planted " + name] = (f"flagged {chk.count} elements in columns {cols(chk)[:3]}..; older comparison accepts: {SEEN[name][0]}, "
                                   f"among {LM_ROWS} rows: {SEEN[name][1]}")
    assert SEEN[name] == OLD_ACCEPTS[name], (name, SEEN[name])


def test_planted_dead_chunk_counted():
    """K = 520 is 65 chunks: in the second chunk step only lane 0 has one, the others clamp to chunk 64 and must zero it."""
    c = CpuCase("bias", 8, 300, 520, seed=11)
    p = plan_py(0, 300, 520, False, False)
    lo, hi = wave_units(p, 5)
    got = epilogue("bias", emulate("pg", c.x, c.wd, exact=False), c.bias, None)
    bad = epilogue("bias", emulate("pg", c.x, c.wd, mask_dead=False, exact=False), c.bias, None)
    assert hi > lo
    got[:, lo:hi] = bad[:, lo:hi]
    finish("dead chunk", c, got, c.x, range(lo, hi))


def test_planted_ragged_batch_shifted_and_next_bias():
    """N = 6401 at K = 256: depth 5, a wave with 9 rows runs 5 + 4.  (a) the short batch stores row n + 1's value at n; (b) the
    first batch adds the bias the look-ahead loaded for the second."""
    N, K = 6401, 256
    p = plan_py(0, N, K, False, False)
    assert (p["rb"], p["uq"], p["ur"]) == (5, 8, 257)
    lo, hi = wave_units(p, 3)
    assert hi - lo == 9
    c = CpuCase("bias", 8, N, K, seed=12)
    acc = emulate("pg", c.x, c.wd, exact=False)
    a = acc.clone()
    a[:, lo + 5:hi] = acc[:, lo + 6:hi + 1]
    finish("ragged shifted", c, epilogue("bias", a, c.bias, None), c.x, range(lo + 5, hi))
    b = c.bias.clone()
    b[lo:lo + 5] = c.bias[[min(lo + 5 + r, hi - 1) for r in range(5)]]
    finish("next bias", c, epilogue("bias", acc, b, None), c.x, range(lo, lo + 5))


def test_planted_residual_of_the_next_scene_and_a_stored_padding_row():
    """B = 3 runs as NB = 4.  (a) a wave's rows take the residual of scene lb + 1 (the last scene's own: min(lb + 1, B - 1));
    (b) the padding scene b = 3 is stored: the guard rows behind the B outputs must keep their sentinel."""
    B, N, K = 3, 8193, 256
    p = plan_py(B, N, K, False, False)
    assert (p["nb"], p["rb"]) == (4, 3) and "ragged" in trips(p)
    lo, hi = wave_units(p, 7)
    c = CpuCase("o", B, N, K, seed=13)
    acc = emulate("pgb", c.x, c.wd, exact=False)
    got = epilogue("o", acc, None, c.res0)
    shifted = epilogue("o", acc, None, c.res0[[1, 2, 2]])
    got[:, lo:hi] = shifted[:, lo:hi]
    finish("next scene residual", c, got, c.x, range(lo, hi), want_rows=[0, 1])
    full = R.sentinel((B + 2, N), torch.float32)
    full[:B] = epilogue("o", acc, None, c.res0)
    assert D.guard_flags(full, B).sum() == 0
    full[B, lo:hi] = full[B - 1, lo:hi]
    flags = D.guard_flags(full, B)
    assert flags.nonzero().tolist() == [[0, n] for n in range(lo, hi)]
    chk = c.check(full[:B], c.x)
    assert chk.count == 0                                        # nothing else notices: only the guard does
    SEEN["padding row"] = (True, True)
    MEASURED["planted padding row"] = f"guard flags {int(flags.sum())}; the older comparisons never look past row B: accepted"
    assert SEEN["padding row"] == OLD_ACCEPTS["padding row"]


def test_planted_gate_and_up_swapped_in_one_group():
    N, K = 2592, 256
    c = CpuCase("gu", 8, N, K, seed=14)
    A = emulate_norm("pg", c.x, c.nw)
    acc = emulate("pg", A, c.wd, exact=False)
    sw = acc.clone().view(8, -1, 2, 16)
    sw[:, 10] = sw[:, 10].flip(1)
    got = epilogue("gu", sw.view(8, N), None, None)
    finish("gate/up swapped", c, got, A, range(160, 176))


def test_planted_wave_7_share_dropped_in_the_long_k_form():
    B, N, K = 4, 300, 8960
    p = plan_py(B, N, K, False, False)
    assert (p["form"], p["per"], p["kch"]) == (3, 2, 140)
    c = CpuCase("o", B, N, K, seed=15)
    got = epilogue("o", emulate("pgk", c.x, c.wd, exact=False), None, c.res0)
    bad = epilogue("o", emulate("pgk", c.x, c.wd, drop_share=7, exact=False), None, c.res0)
    got[:, 34:36] = bad[:, 34:36]                                # block 17 owns rows 34 and 35
    finish("wave 7 dropped", c, got, c.x, range(34, 36), want_rows=[0, 1, 2, 3])


def test_planted_rstd_of_row_0_for_every_row():
    B, K = 5, 1536
    nw, x = 1 + 0.1 * rnd(K, seed=16), rnd(B, K, seed=17)
    r = D.check_norm(emulate_norm("pg", x, nw), x, nw)
    assert r.count == 0
    r = D.check_norm(emulate_norm("pg", x, nw, rstd_row=0), x, nw)
    assert r.flagged_rows() == [1, 2, 3, 4], r.flagged_rows()
    y = (nw[None] * x * x.pow(2).mean(-1, keepdim=True).add(D.EPS).rsqrt()).bfloat16()
    SEEN["rstd of row 0"] = (old_accepts(emulate_norm("pg", x, nw, rstd_row=0), y),) * 2      # every element moves: N does not matter
    MEASURED["planted rstd of row 0"] = f"flagged {r.count} of {r.n}; older comparison accepts: {SEEN['rstd of row 0']}"
    assert SEEN["rstd of row 0"] == OLD_ACCEPTS["rstd of row 0"]


def test_swiglu_check_flags_one_wrong_element():
    gu = rnd(2, 64, seed=18).bfloat16()
    v = gu.float().view(2, -1, 2, 16)
    got = (torch.nn.functional.silu(v[:, :, 0]).bfloat16().float() * v[:, :, 1]).reshape(2, -1).bfloat16()
    assert D.check_swiglu(got, gu).count == 0
    got[1, 7] = G.from_key(G.key(got[1, 7:8]) + 3)[0]
    assert D.check_swiglu(got, gu).bad.nonzero().tolist() == [[1, 7]]


def test_attention_metrics_flag_a_dropped_key():
    g = torch.Generator(); g.manual_seed(19)
    q, K, V = (torch.randn(s, generator=g).bfloat16() for s in ((12, 128), (33, 2, 128), (33, 2, 128)))
    want = D.attention64(q, K, V, 2)
    r, e = D.row_metrics(want.bfloat16(), want)
    assert r < D.REL_BOUND / 2 and e < D.ELEM_BOUND / 2
    r, e = D.row_metrics(D.attention64(q, K[:32], V[:32], 2).bfloat16(), want)
    assert r > D.REL_BOUND and e > D.ELEM_BOUND
