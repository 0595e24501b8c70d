"""CPU: the e4m3 launch table of tests/decode_check.py (TABLE8, ROUTES8) and the checks, before they are applied to the e4m3
decode GEMVs on the GPU (tests/test_fp8_decode_gpu.py).  The shape of tests/test_decode_check_cpu.py, whose helpers it uses.

1. Plan.  plan8_py transcribes pg::plan and rbs() of csrc/decode_dispatch.h for e4m3; it is compared with g2v_gemv_pg_route
   (no device) on every row of the table and over a scan of N, and every row's route is the one pinned in ROUTES8.
2. Coverage.  The routes reached must hold every class of want(): every batch depth of rbs(fp8 = true) for nb = 0, 2, 4, 8 with
   and without SwiGLU and at long K for nb = 0, each in one trip and, where the plan can produce it, in ragged and in even
   trips; every block size 192 - 512; B = 1 .. 8; an odd N whose pair without a second row is the last unit of a wave that has one
   unit, of a full batch and of a ragged last batch; the long-K batched form at S = 2, 3, 6, 9, 9, 12 with per = 1, R and > R
   for R = 8 and 4 and both epilogues; the batch-1 K and boundaries.  What the plan never produces is in UNREACHABLE8, confirmed by
   the scan.  A missing class is named in the failure.
3. Operands.  Every row of the table is drawn with per-row magnitudes: the scale the quantiser returns for row n is
   2^row_exponents[n] and differs from that of rows n +- 1, 2, 3, 4, 6, 8, 12 and 16.
4. Honest fp32 emulations of the three e4m3 summation orders pass check_gemm with zero flags and an implied error under TAU / 4.
   Measured here: largest implied error 0 T for all three (TAU / 4 = 3.8e-6: the bf16 rounding interval of every output held
   the fp64 value), SwiGLU at most 0.50 ulp.
5. Planted mistakes, each where the kernel could make it, are flagged exactly where planted.  OLD8 records, and the tests
   assert, what tests/test_fp8_decode_gpu.py did with the same mistake before this table, on a shape it runs and the operands it
   draws (rows of N(0, 1 / K), no guard rows):
     scale of row n + 1 (pg8, depth 12, 12 + 5)           never ran (depth 12 ran ragged only in the lm_head); planted in every
                                                          row of bias 1000 x 256 it is rejected, by the 17 % of the rows whose
                                                          next row has another scale; at K = 9216 every row has the same scale
     gate and up scales swapped (pg8, depth 6, 6 + 1)     rejected at gu 96 x 256, by 10 of its 48 units
     slot-1 halves to the wrong row (pair form, K 1536)   rejected at qkv 300 x 1536
     phantom row of an odd N stored                       rejected at qkv 7 x 256, B = 3 (the next scene's row 0); ACCEPTED at B = 1
     phantom row's empty sum stored into row N - 1        rejected
     dead chunk counted (pg8 K 1040; pgk8 K 8960 wave 8)  rejected at o 300 x 2064 and down 300 x 8960
     last wave's share dropped (pgk8, second pass)        rejected at down 300 x 8960 (first pass: the second never ran)
     bias / residual of the next batch (ragged trip)      never ran: no bias or residual form had two trips
     scale of the next batch (pair form, 4 + 1)           rejected at gu 17920 x 1536, B = 2, by 22 of the 512 rows looked at
     padding scene's row stored (B = 3 as NB = 4)         ACCEPTED: nothing looked behind the B rows
     byte pairs of a weight word swapped                  rejected at bias 1000 x 256
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_check as D  # noqa: E402
import gemm_check as G  # noqa: E402
import rowop_check as R  # noqa: E402
import test_decode_check_cpu as T  # noqa: E402  (helpers only: trips, wave_units, butterfly, emulate_norm, epilogue, cols)
from g2vlm_amd import hip  # noqa: E402

MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def measured():
    yield
    for k, v in sorted(MEASURED.items()):
        print(f"[fp8 decode check] {k}: {v}")


@pytest.fixture(scope="module")
def built():
    from g2vlm_amd import build
    build.build()
    return hip


# ------------------------------------------------------------------------------------------------ 1. the plan
# rbs(fp8 = true, ..) of csrc/decode_dispatch.h, by (scenes per pass NB - 0: the batch-1 entry, act, long K)
RBS8 = {(0, False, False): (1, 2, 3, 4, 6, 8, 12), (0, True, False): (1, 2, 3, 4, 6), (0, False, True): (1, 2),
        (2, False, False): (1, 2, 4), (2, True, False): (1, 2, 4), (4, False, False): (1, 2, 4), (4, True, False): (1, 2, 4),
        (8, False, False): (1, 2), (8, True, False): (1, 2)}
THREADS = (192, 256, 320, 384, 448, 512)
LONG_K1 = 2048                                                 # batch 1: K above this takes 9 chunk steps and depth <= 2
# (class, depth) the plan never runs in more than one trip
_WHY = "two trips mean more than cap units per wave, and equal_batches() then picks a depth above cap / 2"
UNREACHABLE8 = {((0, False, False), d): _WHY for d in (1, 2, 3, 4, 6)}
UNREACHABLE8.update({((0, True, False), d): _WHY for d in (1, 2, 3)})
UNREACHABLE8[((0, False, True), 1)] = _WHY
UNREACHABLE8.update({((nb, act, False), d): _WHY for nb in (2, 4) for act in (False, True) for d in (1, 2)})
UNREACHABLE8.update({((8, act, False), 1): _WHY for act in (False, True)})


def plan8_py(B, N, K, act, norm):
    """pg::plan of csrc/decode_dispatch.h for e4m3, transcribed: dict(form, threads, rb, kch, nb, uq, ur, per)."""
    def fit(l, x):
        return next((v for v in l if x <= v), l[-1])

    def equal_batches(per, cap):
        if per <= cap:
            return per
        nbat = -(-per // cap)
        return -(-per // nbat)

    if B == 0:
        longk = K > LONG_K1
        l = RBS8[(0, act, longk)]
        U = N // 2 if act else N
        small = N * K * 1.0 / 256.0 < 48.0 * 1024.0
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
        return dict(form=1, threads=64 * best, rb=fit(l, equal_batches(-(-U // waves), l[-1])), kch=9 if longk else 2, nb=0,
                    uq=U // waves, ur=U % waves, per=0)
    nb = fit((2, 4, 8), B)
    if K > 1536:                                                # one wave per 1024 elements of K
        S = (K // 16 + 63) // 64
        return dict(form=3, threads=64 * S, rb=4 if nb == 8 else 8, kch=S, nb=nb, uq=0, ur=0, per=(N + 255) // 256)
    l = RBS8[(nb, act, False)]
    uq, ur = divmod((N + 1) // 2, 2048)                         # units: pairs of rows (act: a gate and an up row)
    return dict(form=2, threads=512, rb=fit(l, equal_batches(uq + (1 if ur else 0), l[-1])), kch=2, nb=nb, uq=uq, ur=ur, per=0)


def plan_of(row):
    B, N, K, act, norm, fp8 = D.route_args(row)
    assert fp8
    return plan8_py(B, N, K, act, norm)


def last_unit_wave(p):
    """(lo, hi) of the wave that owns the last unit."""
    waves = 256 * p["threads"] // 64
    return T.wave_units(p, p["ur"] - 1 if p["uq"] == 0 else waves - 1)


def reached(rows, h=None):
    """The set of coverage classes the rows reach."""
    have = set()
    for row in rows:
        entry, form, B, N, K = row
        p = plan_of(row)
        if h is not None:
            assert h.gemv_pg_route(*D.route_args(row)) == (p["form"], p["threads"], p["rb"], p["kch"]) == D.ROUTES8[row], row
        act = form == "gu"
        kind = "act" if act else ("norm" if form in D.NORM_FORMS else "plain")
        if p["form"] == 3:
            S, Rr = p["kch"], p["rb"]
            assert p["threads"] == 64 * S and 2 <= S <= 12 and 64 * S >= K // 16 > 64 * (S - 1), row
            per = p["per"]
            have.add(("form 3", K, S, Rr, "per 1" if per == 1 else ("per R" if per == Rr else ("per > R ragged" if per > Rr and per % Rr else per))))
            have.add(("form 3 epilogue", "fp32 residual" if form in D.RES_FORMS else "bias, bf16 out"))
        else:
            cls = (p["nb"], act, p["nb"] == 0 and K > LONG_K1)
            assert p["rb"] in RBS8[cls], row
            for k in T.trips(p):
                have.add(("depth", cls, p["rb"], k))
                if cls[2] and p["rb"] == 2:
                    have.add(("long K depth 2", K, k))
            if p["form"] == 1:
                have.add(("threads", p["threads"]))
                have.add(("batch-1 K", K, kind))
            else:
                have.add(("pair-form K", K))
                if N % 2:
                    lo, hi = last_unit_wave(p)
                    n = hi - lo
                    have.add(("odd N", "only unit" if n == 1 else ("full batch" if n % p["rb"] == 0 else
                                                                   ("ragged last batch" if n > p["rb"] else "short single batch"))))
        if p["nb"]:
            have.add(("B", p["nb"], B))
    return have


def want():
    w = set()
    for cls, depths in RBS8.items():
        for d in depths:
            w.add(("depth", cls, d, "one"))
            if (cls, d) not in UNREACHABLE8:
                w |= {("depth", cls, d, "ragged"), ("depth", cls, d, "even")}
    w |= {("threads", t) for t in THREADS}
    w |= {("B", nb, B) for nb, Bs in ((2, (1, 2)), (4, (3, 4)), (8, (5, 6, 7, 8))) for B in Bs}
    w |= {("odd N", k) for k in ("only unit", "full batch", "ragged last batch")}
    for K, S in ((1552, 2), (2064, 3), (6000, 6), (8960, 9), (9216, 9), (12288, 12)):
        w |= {("form 3", K, S, Rr, per) for Rr in (8, 4) for per in ("per 1", "per R", "per > R ragged")}
    w |= {("form 3 epilogue", e) for e in ("fp32 residual", "bias, bf16 out")}
    w |= {("batch-1 K", K, k) for K in (16, 256, 512, 528, 1024, 1040, 1536) for k in ("plain", "norm", "act")}
    w |= {("batch-1 K", K, "plain") for K in (1552, 2048, 2064, 8960, 9216)}
    # the even trips of depth 2 start at N = 4609: at K >= 8960 that is a weight of more than 32 M elements, so they run at 2064
    w |= {("long K depth 2", K, k) for K in (2064, 8960, 9216) for k in ("one", "ragged")} | {("long K depth 2", 2064, "even")}
    w |= {("pair-form K", K) for K in (16, 256, 512, 528, 1024, 1040, 1536)}
    return w


def test_the_table_reaches_every_class(built):
    have = reached(D.TABLE8, built)
    missing = want() - have
    for c in sorted(have, key=str):
        print("[fp8 decode check] reached", c)
    for (cls, d), why in sorted(UNREACHABLE8.items()):
        print("[fp8 decode check] unreachable: more than one trip at", cls, "depth", d)
    assert not missing, sorted(missing, key=str)
    assert all(r[0] in ("pg8", "pgb8") and D.ENTRIES[r[0]][1] for r in D.TABLE8)
    assert all(r[2] == 8 for r in D.TABLE8 if r[0] == "pg8")               # batch 1: 8 activation vectors
    assert not [r for r in D.TABLE8 if r[3] * r[4] > 32 * 2 ** 20]          # no weight above 32 M elements
    assert not [r for r in D.TABLE8 if (r[1], r[3], r[4]) in D.PRODUCTION]  # the production shapes are test_fp8_decode_gpu.py's REAL


def test_every_row_is_the_only_or_a_redundant_carrier_and_dropping_a_sole_carrier_is_noticed():
    """Deleting a row that alone carries a class makes want() - reached() name that class."""
    w, have = want(), {}
    for row in D.TABLE8:
        for c in reached([row]) & w:
            have.setdefault(c, []).append(row)
    sole = {c: r[0] for c, r in have.items() if len(r) == 1}
    assert len(sole) >= 40
    for c, row in list(sole.items())[::7]:
        assert c in w - reached([r for r in D.TABLE8 if r != row])
    MEASURED["sole carriers"] = f"{len(sole)} of {len(w)} classes rest on a single row"


def test_what_is_listed_as_unreachable_is_never_planned(built):
    """Every N up to 70 000 (act: every multiple of 32; long K: up to 9 000) through the route call, against the transcription."""
    seen = set()
    for cls in RBS8:
        nb, act, longk = cls
        B = {0: 0, 2: 2, 4: 3, 8: 8}[nb]
        for K in ((2064, 9216) if longk else (256, 1536)):
            for N in range(32 if act else 1, 9000 if longk else 70000, 32 if act else 1):
                p = plan8_py(B, N, K, act, act)
                assert built.gemv_pg_route(B, N, K, act, act, True) == (p["form"], p["threads"], p["rb"], p["kch"]), (B, N, K, act)
                seen |= {(cls, p["rb"], k) for k in T.trips(p)}
    for cls, depths in RBS8.items():
        for d in depths:
            assert (cls, d, "one") in seen
            multi = {k for k in ("ragged", "even") if (cls, d, k) in seen}
            assert multi == (set() if (cls, d) in UNREACHABLE8 else {"ragged", "even"}), (cls, d, multi)
    assert set(UNREACHABLE8) <= {(cls, d) for cls, depths in RBS8.items() for d in depths}


# ------------------------------------------------------------------------------------------------ 3. operands
D_CONFUSED = (1, 2, 3, 4, 6, 8, 12, 16)


def assert_rows_tell_apart(s, N):
    assert torch.equal(s, torch.ldexp(torch.ones(N), D.row_exponents(N)))
    for d in D_CONFUSED:
        assert bool((s[d:] != s[:-d]).all()), d


def test_the_quantiser_s_scale_of_every_row_differs_from_its_neighbours():
    """On the scales quantize_rows_e4m3 actually returns, for the operands the GPU test draws (which asserts the same on every
    Case): every distinct (form, N, K) of the table up to 4 M elements and the largest weight."""
    done = set()
    big = max(D.TABLE8, key=lambda r: r[3] * r[4])
    for row in D.TABLE8:
        entry, form, B, N, K = row
        if (N * K > 4 * 2 ** 20 and row != big) or (form == "gu", N, K, D.case_seed(row)) in done:
            continue
        done.add((form == "gu", N, K, D.case_seed(row)))
        q, s, wd = D.fp8_weight(form, N, K, D.case_seed(row), row_scales=True)
        assert_rows_tell_apart(s, N)
        qa = q.view(torch.float8_e4m3fn).float().abs().amax(1)
        assert bool(((qa >= 224) & (qa <= 448)).all())              # the codes still fill the e4m3 range
    MEASURED["row scales"] = f"{len(done)} weights drawn; scales 2^{int(D.row_exponents(64).min())} .. 2^{int(D.row_exponents(64).max())}"
    # the operands the earlier tests draw: most neighbours share their scale
    _, s, _ = D.fp8_weight("bias", 1000, 9216, 208)
    MEASURED["row scales without"] = f"N(0, 1/K) rows at K = 9216: {float((s[1:] == s[:-1]).float().mean()):.0%} of the rows share the next row's scale"


# ------------------------------------------------------------------------------------------------ 4. honest emulations
NONE = 1 << 20


def tables8(kind, K, role=0, flip=False):
    """(ci, live, dead) [S, 64, J]: the 16-element chunks a lane accumulates, in order (ci clamped into the row as the kernels
    clamp the address; live: the lane's activation is not zeroed; dead: it is zeroed because the chunk lies past K).
    'pg8': one wave, lane l takes l, l + 64, .. (2 steps up to K = 2048, else 9).  'pgb8': row A (role 0) / row B (role 1) of a
    pair - first the slot-1 chunk 64 + (l & 31), in the low half-wave for row A and the high one for row B (flip: the other
    way round), then chunk l.  'pgk8': S = ceil(K / 1024) waves, wave w takes chunk 64 w + l."""
    nch = K // 16
    l = torch.arange(64)
    if kind == "pg8":
        J = 2 if K <= LONG_K1 else 9
        c = l.view(1, 64, 1) + 64 * torch.arange(J).view(1, 1, J)
    elif kind == "pgb8":
        mine = (l >= 32) == (bool(role) != flip)
        c = torch.stack([torch.where(mine, 64 + (l & 31), NONE), l], 1).view(1, 64, 2)
    else:
        S = (nch + 63) // 64
        c = 64 * torch.arange(S).view(S, 1, 1) + l.view(1, 64, 1)
    return c.clamp_max(nch - 1), c < nch, (c >= nch) & (c < NONE)


def lane_sums(X, Wa, Wb, tab, mask_dead=True, exact=True):
    """fp32 [S, 64, B, N]: lane accumulations of X bf16 [B, K] with the weight codes (as float) Wa [N, K]; the first step of the
    pair form takes Wb.  exact: two products per v_dot2, low byte pair of a word first, added in order; else one matmul per chunk."""
    ci, live, dead = tab
    B, K = X.shape
    N = Wa.shape[0]
    xc = X.float().view(B, K // 16, 16)
    S, _, J = ci.shape
    acc = torch.zeros((S, 64, B, N))
    for j in range(J):
        on = live[:, :, j] if mask_dead else (live[:, :, j] | dead[:, :, j])
        x = xc[:, ci[:, :, j]].permute(1, 2, 0, 3) * on[:, :, None, None]
        w = (Wb if (Wb is not None and j == 0) else Wa).view(N, K // 16, 16)[:, ci[:, :, j]].permute(1, 2, 0, 3)
        if exact:
            prod = x[:, :, :, None, :] * w[:, :, None, :, :]
            for e in range(8):
                acc = acc + (prod[..., 2 * e] + prod[..., 2 * e + 1])
        else:
            acc = acc + torch.matmul(x, w.transpose(2, 3))
    return acc


def wave_total(acc, drop_share=None):
    """reduce_transpose (partners lane ^ 32, ^ 16, ^ 8, then i <-> 7 - i, ^ 2, ^ 1), then the wave shares added in wave order."""
    S, _, B, N = acc.shape
    s = T.butterfly(acc.reshape(S, 64, B * N), (32, 16, 8, 7, 2, 1)).view(S, B, N)
    if S == 1:
        return s[0]
    t = torch.zeros((B, N))
    for k in range(S):
        if k != drop_share:
            t = t + s[k]
    return t


def pair_roles(N, act):
    n = torch.arange(N)
    return (n // 16) % 2 if act else n % 2


def pair_partner(N, act):
    n = torch.arange(N)
    return n ^ 16 if act else (n ^ 1).clamp_max(N - 1)


def emulate8(kind, X, qf, s, act=False, flip_rows=None, **kw):
    """fp32 [B, N]: the row sums over the codes qf (float [N, K]) in the order of `kind`, times the row's scale.
    flip_rows (pair form): rows whose slot-1 partial comes from the other half-wave, which holds the partner row's chunks."""
    B, K = X.shape
    N = qf.shape[0]
    md, ex = kw.get("mask_dead", True), kw.get("exact", True)
    if kind != "pgb8":
        tot = wave_total(lane_sums(X, qf, None, tables8(kind, K), md, ex), kw.get("drop_share"))
    else:
        tot = torch.zeros((B, N))
        role = pair_roles(N, act)
        for r in (0, 1):
            rows = (role == r).nonzero().flatten()
            if rows.numel():
                tot[:, rows] = wave_total(lane_sums(X, qf[rows], qf[rows], tables8(kind, K, r), md, ex))
        if flip_rows is not None and len(flip_rows):
            fr = torch.as_tensor(list(flip_rows))
            part = pair_partner(N, act)[fr]
            for r in (0, 1):
                sel = role[fr] == r
                if bool(sel.any()):
                    tot[:, fr[sel]] = wave_total(lane_sums(X, qf[fr[sel]], qf[part[sel]], tables8(kind, K, r, flip=True), md, ex))
    return tot * s[None]


class Cpu8(T.CpuCase):
    """decode_check.Case's e4m3 operands on the CPU: the same draws, seed for seed."""

    def __init__(self, form, B, N, K, seed, row_scales=True):
        self.form, self.B, self.N, self.K = form, B, N, K
        self.norm, self.act = form in D.NORM_FORMS, form == "gu"
        self.q, self.s, self.wd = D.fp8_weight(form, N, K, seed, row_scales)
        self.qf = self.q.view(torch.float8_e4m3fn).float()
        self.bias = D.rnd(N, seed=seed + 1, scale=0.1).bfloat16() if form in ("qkv", "bias") else None
        self.nw = 1 + 0.1 * D.rnd(K, seed=seed + 2) if self.norm else None
        self.x = D.rnd(B, K, seed=seed + 3) if self.norm else D.rnd(B, K, seed=seed + 3).bfloat16()
        self.res0 = D.rnd(B, N, seed=seed + 4) if form in D.RES_FORMS else None
        self.A = T.emulate_norm("pg", self.x, self.nw) if self.norm else self.x

    def out(self, acc, bias="own", res0="own"):
        return T.epilogue(self.form, acc, self.bias if isinstance(bias, str) else bias, self.res0 if isinstance(res0, str) else res0)


def of_row(row, **kw):
    entry, form, B, N, K = row
    assert row in D.TABLE8, row
    return Cpu8(form, B, N, K, D.case_seed(row), **kw)


HONEST_K = {"pg8": (16, 256, 512, 528, 1024, 1040, 1536, 1552, 2048, 2064, 8960, 9216), "pgb8": (16, 256, 512, 528, 1024, 1040, 1536),
            "pgk8": (1552, 2064, 6000, 8960, 9216, 12288)}


@pytest.mark.parametrize("kind", sorted(HONEST_K))
def test_honest_emulations_pass_with_margin(kind):
    worst_d, worst_ulps = 0.0, 0.0
    for K in HONEST_K[kind]:
        assert any(r[4] == K for r in D.TABLE8)
        for form in ("bias", "o", "qkv", "gu"):
            if (form in D.NORM_FORMS and K > 1536) or (kind == "pgk8" and form in D.NORM_FORMS):
                continue
            c = Cpu8(form, 8, 65 if form != "gu" else 64, K, seed=K + len(form))
            assert_rows_tell_apart(c.s, c.N)
            got = c.out(emulate8(kind, c.A, c.qf, c.s, c.act))
            chk = c.check(got, c.A)
            assert chk.count == 0, chk.report(what=f"{kind} {form} K={K}")
            worst_d, worst_ulps = max(worst_d, chk.max_d), max(worst_ulps, chk.max_ulps)
            if c.act:
                assert chk.max_ulps <= G.ULP_BOUND[G.EPI_SWIGLU]
    MEASURED[f"honest {kind}"] = f"largest implied error {worst_d:.2e} T (TAU / 4 = {G.TAU / 4:.2e}), SwiGLU {worst_ulps:.2f} ulp"
    assert worst_d < G.TAU / 4


# ------------------------------------------------------------------------------------------------ 5. planted mistakes
# What tests/test_fp8_decode_gpu.py did with each before this table: "rejects" / "accepts" on a shape it ran with the operands
# it drew (Case without row_scales, its seeds), "never ran" where none of its launches could make the mistake.
OLD8 = {"scale of row n + 1": ("never ran", "rejects"), "gate and up scales swapped": ("rejects",), "slot-1 halves swapped": ("rejects",),
        "phantom row stored": ("rejects", "accepts"), "phantom row's sum into row N - 1": ("rejects",),
        "dead chunk counted": ("rejects", "rejects"), "last wave's share dropped": ("rejects",),
        "bias of the next batch": ("never ran",), "residual of the next batch": ("never ran",), "scale of the next batch": ("rejects",),
        "padding scene's row stored": ("accepts",), "byte pairs swapped": ("rejects",)}
SEEN = {}
OLD_REAL = [("qkv", 2048, 1536), ("o", 1536, 1536), ("gu", 17920, 1536), ("down", 1536, 8960), ("lm", 151936, 1536)]
OLD_RAGGED = [("qkv", 7, 256), ("qkv", 300, 1536), ("lm", 1000, 256), ("gu", 96, 256), ("gu", 992, 1536),
              ("o", 7, 256), ("o", 300, 2064), ("o", 1000, 9216), ("down", 7, 9216), ("down", 300, 8960), ("down", 1000, 2064),
              ("bias", 7, 2064), ("bias", 1000, 256), ("bias", 300, 9216)]


def old_case(form, N, K, B=None):
    """The Case test_fp8_decode_gpu.py draws for this shape (B None: the batch-1 test)."""
    assert (form, N, K) in OLD_RAGGED
    return Cpu8(form, 8 if B is None else B, N, K, (100 if B is None else 200 + B) + N % 97 + K % 89, row_scales=False)


def old_shapes_with_more_than_one_trip(pred):
    """The shapes of the older test (both entries, its B) whose plan runs two or more trips and satisfy pred(form, plan)."""
    out = []
    for form, N, K in OLD_REAL + OLD_RAGGED:
        for B in (0, 1, 2, 3, 5, 8):
            p = plan8_py(B, N, K, form == "gu", form in D.NORM_FORMS)
            if p["form"] != 3 and T.trips(p) & {"ragged", "even"} and pred(form, p):
                out.append((form, N, K, B))
    return out


def verdict(name, *v):
    SEEN[name] = tuple(v)
    MEASURED["planted " + name] = "flagged where planted; the older test: " + ", ".join(v)
    assert SEEN[name] == OLD8[name], (name, SEEN[name])


def flagged_exactly(name, c, got, want_cols, want_rows=None):
    chk = c.check(got, c.A)
    assert T.cols(chk) == list(want_cols), (name, T.cols(chk)[:20], list(want_cols)[:20])
    if want_rows is not None:
        assert chk.flagged_rows() == list(want_rows), (name, chk.flagged_rows())
    return chk


def old_verdict(c, got):
    return "rejects" if c.check(got, c.A).count else "accepts"


def last_trip(p, gw):
    """(first unit of the last trip, hi) of wave gw, which must run two or more trips with a ragged last one."""
    lo, hi = T.wave_units(p, gw)
    n = hi - lo
    assert n > p["rb"] and n % p["rb"], (n, p["rb"])
    return lo + n // p["rb"] * p["rb"], hi


def test_planted_scale_of_the_next_row():
    """Depth 12, 12 + 5: the rows of wave 3's short batch take the scale of row n + 1."""
    row = ("pg8", "o", 8, 12801, 256)
    p = plan_of(row)
    assert (p["rb"], p["uq"], p["ur"]) == (12, 16, 513)
    u0, hi = last_trip(p, 3)
    c = of_row(row)
    acc = emulate8("pg8", c.A, c.qf, torch.ones(c.N), exact=False)
    s = c.s.clone()
    s[u0:hi] = c.s[u0 + 1:hi + 1]
    flagged_exactly("scale n + 1", c, c.out(acc * s[None]), range(u0, hi), want_rows=range(8))
    never = not old_shapes_with_more_than_one_trip(lambda f, p: p["form"] == 1 and p["rb"] == 12 and f != "lm")
    o = old_case("bias", 1000, 256)
    s = torch.cat([o.s[1:], o.s[-1:]])
    share = float((s != o.s).float().mean())
    MEASURED["old operands, scale of row n + 1"] = f"{share:.0%} of the rows of bias 1000 x 256 have a next row with another scale"
    verdict("scale of row n + 1", "never ran" if never else "ran", old_verdict(o, o.out(emulate8("pg8", o.A, o.qf, s, exact=False))))


def test_planted_gate_and_up_scales_swapped():
    """Depth 6, 6 + 1: the one unit of wave 0's short batch multiplies the gate sum by the up row's scale and the reverse."""
    row = ("pg8", "gu", 8, 12832, 256)
    p = plan_of(row)
    u0, hi = last_trip(p, 0)
    c = of_row(row)
    acc = emulate8("pg8", c.A, c.qf, torch.ones(c.N), exact=False)
    units = torch.arange(u0, hi)
    g = 32 * (units // 16) + units % 16
    s = c.s.clone()
    s[g], s[g + 16] = c.s[g + 16], c.s[g]
    flagged_exactly("gate/up scales", c, c.out(acc * s[None]), range(u0, hi))
    o = old_case("gu", 96, 256)
    s = o.s.view(-1, 2, 16).flip(1).reshape(-1)
    MEASURED["old operands, gate/up"] = f"{int((s != o.s).sum()) // 2} of 48 units of gu 96 x 256 have gate and up rows with different scales"
    verdict("gate and up scales swapped", old_verdict(o, o.out(emulate8("pg8", o.A, o.qf, s, exact=False))))


def test_planted_slot_1_halves_handed_to_the_wrong_row():
    """K = 1536: unit 77 (rows 154, 155) adds the high half-wave's slot-1 partial - row B's chunks 64 .. 95 - to row A and the low
    one to row B.  At K = 1024 slot 1 is empty and the same mistake changes no bit."""
    row = ("pgb8", "qkv", 6, 301, 1536)
    c = of_row(row)
    got = c.out(emulate8("pgb8", c.A, c.qf, c.s, flip_rows=(154, 155)))
    flagged_exactly("slot 1", c, got, [154, 155], want_rows=range(6))
    row = ("pgb8", "qkv", 4, 301, 1024)
    c4 = of_row(row)
    assert torch.equal(emulate8("pgb8", c4.A, c4.qf, c4.s, flip_rows=(154, 155)), emulate8("pgb8", c4.A, c4.qf, c4.s))
    o = old_case("qkv", 300, 1536, B=3)
    verdict("slot-1 halves swapped", old_verdict(o, o.out(emulate8("pgb8", o.A, o.qf, o.s, flip_rows=range(300), exact=False))))


def test_planted_phantom_row_of_an_odd_n():
    """N = 8191 at NB = 8: the last unit (row 8190 and no second row) closes a full batch of wave 2047.  (a) its second value is
    stored: element N of scene b is element 0 of scene b + 1, and of the first guard row for the last scene; (b) the
    phantom's sum is taken as empty and stored into row N - 1."""
    row = ("pgb8", "qkv", 8, 8191, 256)
    p = plan_of(row)
    lo, hi = last_unit_wave(p)
    assert (p["rb"], hi - lo, hi) == (2, 2, 4096)
    c = of_row(row)
    B, N = c.B, c.N
    acc = emulate8("pgb8", c.A, c.qf, c.s, exact=False)
    full = R.sentinel((B + D.GUARD, N), torch.bfloat16)
    full[:B] = c.out(acc)
    assert not D.guard_flags(full, B).any() and c.check(full[:B], c.A).count == 0
    flat = full.view(-1)
    for b in range(B):
        flat[b * N + N] = full[b, N - 1]                          # the re-read row N - 1 with its own bias
    assert D.guard_flags(full, B).nonzero().tolist() == [[0, 0]]
    flagged_exactly("phantom stored", c, full[:B], [0], want_rows=range(1, B))
    a = acc.clone()
    a[:, N - 1] = 0.0
    flagged_exactly("phantom into N - 1", c, c.out(a), [N - 1], want_rows=range(B))
    res = []
    for Bo in (3, 1):                                            # the older test: N = 7, no guard rows
        o = old_case("qkv", 7, 256, B=Bo)
        good = o.out(emulate8("pgb8", o.A, o.qf, o.s))
        for b in range(Bo - 1):
            good[b + 1, 0] = good[b, 6]
        res.append(old_verdict(o, good))
    verdict("phantom row stored", *res)
    o = old_case("qkv", 7, 256, B=3)
    a = emulate8("pgb8", o.A, o.qf, o.s)
    a[:, 6] = 0.0
    verdict("phantom row's sum into row N - 1", old_verdict(o, o.out(a)))


def test_planted_dead_chunk_counted():
    """(a) pg8 at K = 1040: 65 chunks, in the second step lane 0 alone is live, the others clamp to chunk 64 and must zero it.
    (b) pgk8 at K = 8960: 560 chunks in 9 x 64 slots, lanes 48 .. 63 of wave 8 clamp to chunk 559."""
    row = ("pg8", "bias", 8, 301, 1040)
    p = plan_of(row)
    lo, hi = T.wave_units(p, 5)
    assert hi > lo
    c = of_row(row)
    got = c.out(emulate8("pg8", c.A, c.qf, c.s, exact=False))
    bad = c.out(emulate8("pg8", c.A, c.qf, c.s, exact=False, mask_dead=False))
    got[:, lo:hi] = bad[:, lo:hi]
    flagged_exactly("dead chunk pg8", c, got, range(lo, hi))
    row = next(r for r in D.TABLE8 if r[3:] == (1000, 8960))
    p = plan_of(row)
    assert (p["form"], p["kch"], p["rb"], p["per"]) == (3, 9, 4, 4)
    c = of_row(row)
    got = c.out(emulate8("pgk8", c.A, c.qf, c.s, exact=False))
    bad = c.out(emulate8("pgk8", c.A, c.qf, c.s, exact=False, mask_dead=False))
    got[:, 68:72] = bad[:, 68:72]                                # block 17
    flagged_exactly("dead chunk pgk8", c, got, range(68, 72))
    o1, o2 = old_case("o", 300, 2064), old_case("down", 300, 8960, B=3)
    verdict("dead chunk counted", old_verdict(o1, o1.out(emulate8("pg8", o1.A, o1.qf, o1.s, exact=False, mask_dead=False))),
            old_verdict(o2, o2.out(emulate8("pgk8", o2.A, o2.qf, o2.s, exact=False, mask_dead=False))))


def test_planted_last_wave_s_share_dropped():
    """K = 8960, R = 8, per = 9: block 100's second pass (its one ragged row 908) adds the shares of waves 0 .. 7 only."""
    row = next(r for r in D.TABLE8 if r[3:] == (2100, 8960))
    p = plan_of(row)
    assert (p["form"], p["kch"], p["rb"], p["per"]) == (3, 9, 8, 9)
    c = of_row(row)
    got = c.out(emulate8("pgk8", c.A, c.qf, c.s, exact=False))
    bad = c.out(emulate8("pgk8", c.A, c.qf, c.s, exact=False, drop_share=8))
    n = 100 * 9 + 8
    got[:, n] = bad[:, n]
    flagged_exactly("last share", c, got, [n], want_rows=range(c.B))
    o = old_case("down", 300, 8960, B=3)                         # per = 2: one pass
    assert plan8_py(3, 300, 8960, False, False)["per"] == 2
    verdict("last wave's share dropped", old_verdict(o, o.out(emulate8("pgk8", o.A, o.qf, o.s, exact=False, drop_share=8))))


def test_planted_bias_residual_and_scale_of_the_next_batch():
    """The look-ahead of a ragged launch loads the next batch's bias, residual and scale while this batch is reduced.  (a) pg8
    depth 8, 8 + 5: wave 0's first batch adds the bias loaded for the second (unit min(u0 + 8 + i, hi - 1)); (b) pair form, NB = 4,
    4 + 1: wave 0's first batch adds the residual of the second batch's rows; (c) pair form, NB = 2, 4 + 1: its scale."""
    row = ("pg8", "qkv", 8, 9217, 256)
    p = plan_of(row)
    lo, hi = T.wave_units(p, 0)
    assert (p["rb"], hi - lo) == (8, 13)
    c = of_row(row)
    acc = emulate8("pg8", c.A, c.qf, c.s, exact=False)
    b = c.bias.clone()
    b[lo:lo + 8] = c.bias[[min(lo + 8 + i, hi - 1) for i in range(8)]]
    flagged_exactly("next bias", c, c.out(acc, bias=b), range(lo, lo + 8))

    def pair_rows_of_the_next_batch(p, N):
        lo, hi = T.wave_units(p, 0)
        assert (p["rb"], hi - lo) == (4, 5)
        return [2 * min(lo + 4 + i // 2, hi - 1) + i % 2 for i in range(8)]

    row = ("pgb8", "o", 4, 16385, 256)
    c = of_row(row)
    nxt = pair_rows_of_the_next_batch(plan_of(row), c.N)
    acc = emulate8("pgb8", c.A, c.qf, c.s, exact=False)
    r = c.res0.clone()
    r[:, :8] = c.res0[:, nxt]
    flagged_exactly("next residual", c, c.out(acc, res0=r), range(8), want_rows=range(4))
    row = ("pgb8", "bias", 2, 16385, 256)
    c = of_row(row)
    nxt = pair_rows_of_the_next_batch(plan_of(row), c.N)
    s = c.s.clone()
    s[:8] = c.s[nxt]
    flagged_exactly("next scale", c, c.out(emulate8("pgb8", c.A, c.qf, s, exact=False)), range(8), want_rows=range(2))
    assert not old_shapes_with_more_than_one_trip(lambda f, p: f in ("qkv", "bias") + D.RES_FORMS)
    verdict("bias of the next batch", "never ran")
    verdict("residual of the next batch", "never ran")
    # the scale: the batched gate/up Linear (4 + 1 pairs in waves 0 .. 767) and the lm_head at batch 1 ran two trips.  The first
    # 64 waves of gate/up at B = 2 with the operands that test draws: rows 0 .. 639 are their 320 units
    two = old_shapes_with_more_than_one_trip(lambda f, p: True)
    assert {(f, N) for f, N, K, B in two} == {("gu", 17920), ("lm", 151936)} and ("gu", 17920, 1536, 2) in two
    p = plan8_py(2, 17920, 1536, True, True)
    assert (p["rb"], p["uq"], p["ur"]) == (4, 4, 768)
    o = Cpu8("gu", 2, 17920, 1536, 200 + 17920 % 97 + 1536 % 89 + 2, row_scales=False)
    o.N, o.qf, o.wd, s = 640, o.qf[:640], o.wd[:640], o.s[:640].clone()
    for w in range(64):
        for u in range(5 * w, 5 * w + 4):
            g, g2 = 32 * (u // 16) + u % 16, 32 * ((5 * w + 4) // 16) + (5 * w + 4) % 16
            s[g], s[g + 16] = o.s[g2], o.s[g2 + 16]
    MEASURED["old operands, next batch's scale"] = f"{int((s != o.s[:640]).sum())} of 512 rows of gu 17920 x 1536 get another scale"
    verdict("scale of the next batch", old_verdict(o, o.out(emulate8("pgb8", o.A, o.qf, s, act=True, exact=False))))


def test_planted_padding_scene_s_row_stored():
    """B = 3 runs as NB = 4: the fourth scene's values (the third's again) are stored.  Only the guard rows notice."""
    row = ("pgb8", "bias", 3, 8193, 256)
    p = plan_of(row)
    assert p["nb"] == 4
    lo, hi = T.wave_units(p, 7)
    c = of_row(row)
    full = R.sentinel((c.B + D.GUARD, c.N), torch.bfloat16)
    full[:c.B] = c.out(emulate8("pgb8", c.A, c.qf, c.s, exact=False))
    assert not D.guard_flags(full, c.B).any()
    full[c.B, 2 * lo:2 * hi] = full[c.B - 1, 2 * lo:2 * hi]
    assert D.guard_flags(full, c.B).nonzero().tolist() == [[0, n] for n in range(2 * lo, 2 * hi)]
    assert c.check(full[:c.B], c.A).count == 0
    verdict("padding scene's row stored", "accepts")             # the older test drew no guard rows


def test_planted_byte_pairs_of_a_weight_word_swapped():
    """cvt8_lo and cvt8_hi exchanged: bytes 2, 3 of every word meet the activations of bytes 0, 1.  Wave 2 of a depth-4 launch."""
    row = ("pg8", "bias", 8, 2561, 256)
    p = plan_of(row)
    lo, hi = T.wave_units(p, 2)
    assert p["rb"] == 4 and hi - lo == 4
    c = of_row(row)
    qf = c.qf.clone()
    qf[lo:hi] = c.qf[lo:hi].view(hi - lo, -1, 2, 2).flip(2).reshape(hi - lo, -1)
    flagged_exactly("byte pairs", c, c.out(emulate8("pg8", c.A, qf, c.s, exact=False)), range(lo, hi), want_rows=range(8))
    o = old_case("bias", 1000, 256)
    qf = o.qf.view(1000, -1, 2, 2).flip(2).reshape(1000, -1)
    verdict("byte pairs swapped", old_verdict(o, o.out(emulate8("pg8", o.A, qf, o.s, exact=False))))


def test_every_planted_mistake_has_its_record():
    """Runs last: every entry of OLD8 was produced by a test above."""
    assert set(SEEN) == set(OLD8), set(OLD8) ^ set(SEEN)
