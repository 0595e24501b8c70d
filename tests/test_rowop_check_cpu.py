"""CPU (no GPU): the row-kernel checks of tests/rowop_check.py against honest emulations and planted errors.

Honest emulations - fp32 torch restatements of layernorm_kernel, rmsnorm_kernel and qknorm_mrope_cache_kernel in their own
summation order (per-lane groups of four, the 64-lane or 16-lane xor tree, separate multiplies and adds) - must give zero
flags on every input family (`3 randn + 0.5`, `100 + randn`, `1e-3 randn`, `1e4 randn`, an all-zero row), stay under 0.25 of
the bound, and keep the share of bf16 outputs with more than one admissible value under the 2 % cap.  The one exemption: the
bf16-output LayerNorm of the offset rows (`100 + randn`), whose T carries mean|x| ~ 100 sigma, so TAU T is a sizeable part
of a bf16 ulp there; those rows are checked in the fp32-output form, which has no admissible set.

Each planted error must be flagged where it was planted and nowhere else, while the comparisons the older tests use
(assert_bf16_close and the whole-tensor rel < 1e-6 of tests/test_kernels_gpu.py, copied here) accept the same output.  A
fault that spoils a whole row passes assert_bf16_close only once the row is under 0.2 % of the tensor and under its rel-L2
bound, so those are planted in a 2500-row tensor; a 0.13 % change of one row's rstd flips a third of its bf16 roundings, which
passes in a 400-row tensor; the single-element faults pass at the older tests' own sizes.  A dropped eps is
accepted by any comparison on the older tests' data (mean(x^2) ~ 9: nothing moves), which the test records, and is flagged
on a row with mean(x^2) = 4 eps.  "cos/sin from the wrong axis at a section boundary" is planted at d = 16 (first h dim, given
the t angle) and at d = 15 (last t dim, given the h angle).  An ignored und_rounding is the one planted error that
assert_bf16_close rejects too (it moves a third of all elements by one ulp), and the test records that.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowop_check as R  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
CS = [4, 160, 516, 1280, 1536, 2048]
FAMILIES = ["plain", "offset", "tiny", "huge", "zero"]
STATS = {}


@pytest.fixture(scope="module", autouse=True)
def measured():
    """Prints the maxima the rowop_check.py docstring quotes (visible with -s)."""
    yield
    for k, v in sorted(STATS.items()):
        print("STATS", k, f"{v:.3g}")


def note(k, v):
    STATS[k] = max(STATS.get(k, 0.0), float(v))


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


def old_accepts(got, y):
    """What the older tests assert on this output: assert_bf16_close(ulps=1.01) for bf16, rel < 1e-6 for fp32."""
    if got.dtype == F32:
        return rel(got, y.float()) < 1e-6
    try:
        assert_bf16_close(got, R.rn(y), ulps=1.01)
        return True
    except AssertionError:
        return False


def rnd(*shape, seed=0):
    g = torch.Generator(); g.manual_seed(seed)
    return torch.randn(shape, generator=g)


def family(name, M, C, seed):
    z = rnd(M, C, seed=seed)
    return {"plain": 3 * z + 0.5, "offset": 100 + z, "tiny": 1e-3 * z, "huge": 1e4 * z, "zero": torch.zeros(M, C)}[name]


def weights(C, seed):
    return 1 + 0.1 * rnd(C, seed=seed), 0.1 * rnd(C, seed=seed + 1), 1 + 0.1 * rnd(C, seed=seed + 2)


# --------------------------------------------------------------------------------------------- the emulations
def lanes(x, mv):
    """fp32 [M, C] -> [M, mv, 64, 4], zero beyond C: group i of lane l holds columns (i 64 + l) 4 .. + 3."""
    M, C = x.shape
    p = torch.zeros((M, 256 * mv), dtype=F32)
    p[:, :C] = x
    return p.view(M, mv, 64, 4)


def tree(v, width=64):
    """The xor-shuffle reduction over the last dim (every lane ends with the same sum); returns lane 0, keepdim."""
    idx = torch.arange(width)
    o = width // 2
    while o:
        v = v + v[..., idx ^ o]
        o //= 2
    return v[..., :1]


def emul_rmsnorm(x, w_lo, w_hi, split, eps, out_dtype, fault=None, row=0):
    M, C = x.shape
    mv = R.maxv(C)
    v = lanes(x.float(), mv)
    q = torch.zeros((M, 64), dtype=F32)
    for i in range(mv):
        sq = v[:, i] * v[:, i]
        part = (sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3])
        if fault == "lane" and i == (C // 4 - 1) // 64:
            part[row, (C // 4 - 1) % 64] = 0.0                  # the lane that holds the row's last four columns
        q = q + part
    div = torch.full((M, 1), float(C), dtype=F32)
    e = torch.full((M, 1), eps, dtype=F32)
    lo = torch.arange(M) < split
    if fault == "padded":
        div[row] = 256.0 * mv
    if fault == "eps":
        e[row] = 0.0
    if fault == "w_hi":
        lo[row] = False
    rstd = 1.0 / torch.sqrt(tree(q) / div + e)
    w = torch.where(lo[:, None], w_lo[None], w_hi[None])
    return (w * (x.float() * rstd)).to(out_dtype)


def emul_layernorm(x, w, b, eps, out_dtype, fault=None, row=0):
    M, C = x.shape
    mv = R.maxv(C)
    xf = x.float()
    v = lanes(xf, mv)
    live = lanes(torch.ones((M, C)), mv) > 0
    div = torch.full((M, 1), float(C), dtype=F32)
    if fault == "padded":
        div[row] = 256.0 * mv
    s = torch.zeros((M, 64), dtype=F32)
    for i in range(mv):
        s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
    mean = tree(s) / div
    q = torch.zeros((M, 64), dtype=F32)
    for i in range(mv):
        for e in range(4):
            d = v[:, i, :, e] - mean
            q = q + torch.where(live[:, i, :, e], d * d, torch.zeros_like(d))
    rstd = 1.0 / torch.sqrt(tree(q) / div + torch.tensor(eps, dtype=F32))
    return (((xf - mean) * rstd) * w + b).to(out_dtype)


def emul_qk(qkv, Hq, Hkv, ws, split, eps, und, cos, sin, kv_rows, k_cache, v_cache, flip=None, k_shift_row=None):
    """Returns q_out and writes the caches in place.  flip = (row, head, d): the sign of rotate_half flipped there;
    k_shift_row: that row's K goes to kv_rows[row] + 1."""
    L = qkv.shape[0]
    H = Hq + Hkv
    x = qkv.view(L, Hq + 2 * Hkv, 128)
    xh = x[:, :H].float()
    x0, x1 = xh[..., :64].reshape(L, H, 16, 4), xh[..., 64:].reshape(L, H, 16, 4)
    ss = torch.zeros((L, H, 16), dtype=F32)
    for e in range(4):
        ss = ss + (x0[..., e] * x0[..., e] + x1[..., e] * x1[..., e])
    rstd = 1.0 / torch.sqrt(tree(ss, 16) / 128.0 + torch.tensor(eps, dtype=F32))
    n = xh * rstd
    if und:
        n = n.bfloat16().float()
    lo = (torch.arange(L) < split)[:, None, None]
    w = torch.cat([torch.where(lo, ws[0][None, None], ws[1][None, None]).expand(L, Hq, 128),
                   torch.where(lo, ws[2][None, None], ws[3][None, None]).expand(L, Hkv, 128)], 1)
    m = w * n
    rot = torch.cat([-m[..., 64:], m[..., :64]], -1)
    if flip is not None:
        rot[flip] = -rot[flip]
    a = m * cos[:, None, :]
    b = rot * sin[:, None, :]
    o = (a + b).bfloat16()
    rows = kv_rows.long().clone()
    v_cache[rows] = x[:, H:]
    if k_shift_row is not None:
        rows[k_shift_row] += 1
    k_cache[rows] = o[:, Hq:]
    return o[:, :Hq].contiguous()


# ---------------------------------------------------------------------------------------- honest emulations pass
@pytest.mark.parametrize("C", CS)
def test_honest_norm_emulations_pass(C):
    w, b, w2 = weights(C, 100 + C)
    for fi, fam in enumerate(FAMILIES):
        M = 1 if fam == "zero" else 12
        x = family(fam, M, C, seed=7 * C + fi)
        for eps in (1e-6, 1e-5):
            for xin in (x, x.bfloat16()):
                y, T = R.layernorm64(xin, w, b, eps)
                for od in (F32, BF):
                    got = emul_layernorm(xin, w, b, eps, od)
                    res = R.check_out(got, y, T)
                    assert res.count == 0, res.report(f"layernorm C={C} {fam} {xin.dtype}->{od} eps={eps}")
                    assert res.max_ratio < 0.25
                    note(("layernorm ratio", str(od)), res.max_ratio)
                    if od == BF and res.n >= 1000:                # C = 4: 48 elements, one of them is 2 %
                        note(("layernorm multi share", fam), res.multi_share)
                        if fam != "offset":                       # the offset rows' bf16 form is exempt (module docstring)
                            assert res.multi_share <= R.MULTI_CAP, (C, fam, res.multi_share)
                    if fam == "zero":
                        assert torch.equal(got.double(), b.double()[None].to(od).double()) and torch.equal(y, b.double()[None])
            for split in (0, M // 2, M):
                y, T = R.rmsnorm64(x, w, w2, split, eps)
                for od in (F32, BF):
                    got = emul_rmsnorm(x, w, w2, split, eps, od)
                    res = R.check_out(got, y, T)
                    assert res.count == 0, res.report(f"rmsnorm C={C} {fam} ->{od} split={split}")
                    assert res.max_ratio < 0.25
                    note(("rmsnorm ratio", str(od)), res.max_ratio)
                    if od == BF and res.n >= 1000:
                        note(("rmsnorm multi share", fam), res.multi_share)
                        assert res.multi_share <= R.MULTI_CAP, (C, fam, res.multi_share)
                    if fam == "zero":
                        assert float(got.abs().max()) == 0 and float(y.abs().max()) == 0


def qk_case(L=45, Hq=12, Hkv=2, seed=31, perm=True):
    qkv = rnd(L, (Hq + 2 * Hkv) * 128, seed=seed).bfloat16()
    ws = [1 + 0.1 * rnd(128, seed=seed + 1 + i) for i in range(4)]
    g = torch.Generator(); g.manual_seed(seed + 9)
    pos = torch.stack([torch.randint(0, 2000, (L,), generator=g), torch.randint(2000, 4000, (L,), generator=g),
                       torch.randint(4000, 6000, (L,), generator=g)])
    inv = 1.0 / (1e6 ** (torch.arange(0, 128, 2, dtype=torch.int64).float() / 128))
    c64, s64 = R.mrope_table64(pos, inv)
    Rr = 2 * L + 8
    rows = (torch.randperm(L, generator=g) * 2 + 3).to(torch.int32) if perm else torch.arange(L, dtype=torch.int32) + 8
    return dict(qkv=qkv, Hq=Hq, Hkv=Hkv, ws=ws, cos=c64.float(), sin=s64.float(), rows=rows, R=Rr, L=L, pos=pos, inv=inv)


def run_qk(c, split, und, emul_und=None, cos=None, sin=None, **fault):
    kb, vb = R.sentinel((c["R"], c["Hkv"], 128), BF), R.sentinel((c["R"], c["Hkv"], 128), BF)
    ka, va = kb.clone(), vb.clone()
    cs, sn = (c["cos"] if cos is None else cos), (c["sin"] if sin is None else sin)
    q = emul_qk(c["qkv"], c["Hq"], c["Hkv"], c["ws"], split, 1e-6, und if emul_und is None else emul_und, cs, sn, c["rows"],
                ka, va, **fault)
    res = R.check_qknorm_mrope_cache(c["qkv"], c["Hq"], c["Hkv"], *c["ws"], split, 1e-6, und, c["cos"], c["sin"], c["rows"], q,
                                     kb, ka, vb, va)
    return res, q, ka


@pytest.mark.parametrize("und", [0, 1])
@pytest.mark.parametrize("Hq,Hkv", [(12, 2), (2, 1)])
def test_honest_qk_emulation_passes(und, Hq, Hkv):
    for L in (1, 3, 45):
        c = qk_case(L=L, Hq=Hq, Hkv=Hkv)
        for split in (0, L // 2, L):
            res, _, _ = run_qk(c, split, und)
            assert res.count == 0, res.report(f"L={L} und={und} split={split}")
            assert res.max_ratio < 0.25
            note(("qknorm ratio", und), res.max_ratio)
            if L == 45:
                note(("qknorm multi share", und), res.multi_share)
                assert res.multi_share <= R.MULTI_CAP


# ------------------------------------------------------------------------------------------------ planted errors
BIG_M = 2500          # one spoiled row is 0.04 % of the tensor and moves its rel-L2 by 0.14 / 50: under both allowances of assert_bf16_close
MID_M = 400           # a row in which a third of the elements move by one ulp (some ulps exceed 1.01 x 2^-8 |ref|) is under it too


def test_planted_eps_dropped():
    C, row = 516, 700
    w, b, w2 = weights(C, 1)
    x = family("plain", BIG_M, C, seed=2)
    # on the older tests' data nothing moves: every comparison, this one included, accepts a missing eps
    y, T = R.rmsnorm64(x, w, w2, 41, 1e-6)
    for od in (F32, BF):
        got = emul_rmsnorm(x, w, w2, 41, 1e-6, od, fault="eps", row=row)
        assert old_accepts(got, y) and R.check_out(got, y, T).count == 0
    x[row] = 2e-3 * rnd(C, seed=3)                              # mean(x^2) = 4 eps
    y, T = R.rmsnorm64(x, w, w2, 41, 1e-6)
    for od in (F32, BF):
        got = emul_rmsnorm(x, w, w2, 41, 1e-6, od, fault="eps", row=row)
        res = R.check_out(got, y, T)
        assert res.flagged_rows() == [row] and res.count > C // 2, res.report()
    assert old_accepts(got, y)                                  # bf16: one row of 2500, rel-L2 2e-3


@pytest.mark.parametrize("kernel", ["rmsnorm", "layernorm"])
def test_planted_padded_width(kernel):
    C, row = 1532, 17                                           # MAXV = 6: 1536 padded columns
    w, b, w2 = weights(C, 4)
    x = family("plain", MID_M, C, seed=5)
    for od in (F32, BF):
        if kernel == "rmsnorm":
            y, T = R.rmsnorm64(x, w, w2, 20, 1e-6)
            got = emul_rmsnorm(x, w, w2, 20, 1e-6, od, fault="padded", row=row)
        else:
            y, T = R.layernorm64(x, w, b, 1e-6)
            got = emul_layernorm(x, w, b, 1e-6, od, fault="padded", row=row)
        res = R.check_out(got, y, T)
        assert res.flagged_rows() == [row], res.report()
        assert res.count > (C // 2 if od == F32 else 20)
    assert old_accepts(got, y)                                  # bf16: a 0.13 % change of rstd stays within an ulp


def test_planted_w_hi_on_row_split_minus_1():
    C, split = 516, 641
    w, b, w2 = weights(C, 6)
    x = family("plain", BIG_M, C, seed=7)
    y, T = R.rmsnorm64(x, w, w2, split, 1e-6)
    for od in (F32, BF):
        got = emul_rmsnorm(x, w, w2, split, 1e-6, od, fault="w_hi", row=split - 1)
        res = R.check_out(got, y, T)
        assert res.flagged_rows() == [split - 1] and res.count > C // 2, res.report()
    assert old_accepts(got, y)


def test_planted_lane_missing_from_sum_of_squares():
    C, row = 1536, 9
    w, b, w2 = weights(C, 8)
    x = family("plain", MID_M, C, seed=9)
    y, T = R.rmsnorm64(x, w, w2, 20, 1e-6)
    for od in (F32, BF):
        got = emul_rmsnorm(x, w, w2, 20, 1e-6, od, fault="lane", row=row)
        res = R.check_out(got, y, T)
        assert res.flagged_rows() == [row], res.report()
        assert res.count > (C // 2 if od == F32 else 20)
    assert old_accepts(got, y)


def test_planted_one_ulp():
    C = 160
    w, b, w2 = weights(C, 10)
    x = family("plain", 37, C, seed=11)
    y, T = R.layernorm64(x, w, b, 1e-6)
    got = emul_layernorm(x, w, b, 1e-6, BF)
    # an element whose y* sits in the middle half of its rounding interval: away from a tie
    off = (y - got.double()).abs() / R.ulp_bf16(y)
    cand = ((off < 0.25) & (y.abs() > 0.1)).nonzero()
    r, c = (int(v) for v in cand[len(cand) // 2])
    for step in (1, -1):
        bad = got.clone()
        bad[r, c] = R.from_key(R.key(got[r, c].reshape(1)) + step)[0]
        res = R.check_out(bad, y, T)
        assert res.where() == [(r, c)], res.report()
        assert old_accepts(bad, y)


def test_planted_rotate_half_sign():
    c = qk_case()
    for und in (0, 1):
        for h, d in ((3, 70), (12, 5)):                          # a q head, second half; a k head, first half
            res, q, ka = run_qk(c, 40, und, flip=(20, h, d))
            if h < c["Hq"]:
                assert res.q.where() == [(20, h, d)] and res.k.count == 0 and res.v.count == 0, res.report()
            else:
                assert res.k.where() == [(int(c["rows"][20]), h - c["Hq"], d)] and res.q.count == 0 and res.v.count == 0
        honest, q0, _ = run_qk(c, 40, und)
        assert_bf16_close(q, q0, ulps=1.01)                      # the older comparison accepts one wrong element
    assert honest.count == 0


@pytest.mark.parametrize("d,src", [(16, 0), (15, 1)])
def test_planted_wrong_axis_at_a_section_boundary(d, src):
    """d = 16 is the first h dim, d = 15 the last t dim: each is given the neighbouring section's axis, on one row."""
    c = qk_case()
    row = 11
    c["pos"][:, row] = torch.tensor([1000, 1001, 1003])          # neighbouring positions, as the tokens of an image have
    c64, s64 = R.mrope_table64(c["pos"], c["inv"])
    c["cos"], c["sin"] = c64.float(), s64.float()
    f = (c["pos"][src, row].float() * c["inv"][d]).double()
    cos, sin = c["cos"].clone(), c["sin"].clone()
    for dd in (d, d + 64):
        cos[row, dd], sin[row, dd] = f.cos().float(), f.sin().float()
    # the table check sees it at (row, d) and (row, d + 64) only
    bad, _ = R.check_mrope_table(cos, sin, c["pos"], c["inv"], 2e-6)
    assert [tuple(i) for i in bad.nonzero().tolist()] == [(row, d), (row, d + 64)]
    assert R.check_mrope_table(c["cos"], c["sin"], c["pos"], c["inv"], 2e-6)[0].sum() == 0
    # and the kernel check sees outputs computed from such a table, at that row and those two dims of every head
    res, q, ka = run_qk(c, 40, 1, cos=cos, sin=sin)
    assert res.count > 0 and res.v.count == 0
    assert all(w[0] == row and w[2] in (d, d + 64) for w in res.q.where())
    assert all(w[0] == int(c["rows"][row]) and w[2] in (d, d + 64) for w in res.k.where())
    assert res.q.count >= c["Hq"]                                # a 0.03 rad error of the angle is 2^14 TAU
    _, q0, _ = run_qk(c, 40, 1)
    assert_bf16_close(q, q0, ulps=1.01)                          # 24 elements of 69120 wrong by ~3 %: accepted


def test_planted_k_row_written_one_row_late():
    c = qk_case()
    r = 30
    res, q, ka = run_qk(c, 40, 1, k_shift_row=r)
    tgt = int(c["rows"][r])
    assert res.q.count == 0 and res.v.count == 0
    assert res.k.flagged_rows() == [tgt, tgt + 1], res.report()  # the sentinel left behind, and the unnamed row written
    assert res.k.count == 2 * c["Hkv"] * 128
    # the older test's cache rows are arange + T0 and it compares kc[T0:] only after zero-filling: with a gapped scatter it
    # has no statement about the rows in between at all


def test_planted_und_rounding_ignored():
    c = qk_case()
    res, q, ka = run_qk(c, 40, 1, emul_und=0)
    assert res.count > 100 and res.v.count == 0, res.report()
    _, q0, _ = run_qk(c, 40, 1)
    with pytest.raises(AssertionError):                          # the one planted error the older comparison catches as well:
        assert_bf16_close(q, q0, ulps=1.01)                      # a third of the elements move by an ulp of more than 1.01 x 2^-8 |ref|
    res, q, ka = run_qk(c, 40, 0, emul_und=1)                    # and the converse
    assert res.count > 100


# ------------------------------------------------------------------------------------------- the exact-op helpers
def test_cast_table_covers_what_it_names():
    t = R.cast_table()
    b = R.bits(t.bfloat16()).to(torch.int32) & 0xFFFF
    x = R.bits(t).to(torch.int64) & 0xFFFFFFFF
    want = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x7F7F7FFF: 0x7F7F, 0x7F7F8000: 0x7F80,
            0xFF7F8000: 0xFF80, 0x80000000: 0x8000, 0x007FFFFF: 0x0080, 0x00000001: 0x0000, 0x00008000: 0x0000, 0x00018000: 0x0002}
    got = {int(k): int(v) for k, v in zip(x, b)}
    for k, v in want.items():
        assert got[k] == v, (hex(k), hex(got[k]), hex(v))
    assert torch.isnan(R.cast_nan_table()).all() and torch.isnan(R.cast_nan_table().bfloat16()).all()


def test_sentinels_and_rope_vision_emulation():
    s = R.sentinel((3, 5), BF)
    assert R.is_sentinel(s).all() and torch.isnan(s.float()).all()
    s[1, 2] = 1.0
    assert int((~R.is_sentinel(s)).sum()) == 1
    assert R.is_sentinel(R.sentinel((2, 2), F32)).all()
    L, Hh, D = 5, 3, 8
    x = rnd(L, Hh * D + 4, seed=50).bfloat16()
    ang = rnd(L, D // 2, seed=51) * 3
    emb = torch.cat([ang, ang], -1)
    out = R.rope_vision_emul(x, Hh, D, emb.cos(), emb.sin())
    assert torch.equal(out[:, Hh * D:], x[:, Hh * D:])
    t = x[:, :Hh * D].view(L, Hh, D).double()
    ref = t * emb.cos().double()[:, None] + torch.cat([-t[..., D // 2:], t[..., :D // 2]], -1) * emb.sin().double()[:, None]
    assert ((out[:, :Hh * D].view(L, Hh, D).double() - ref).abs() <= R.ulp_bf16(ref)).all()
