"""GPU: every launch form of csrc/norm_rope.hip and the fp32 row movers and casts of csrc/misc.hip, element by element
against the fp64 references and exact emulations of tests/rowop_check.py (the rule behind each bound is in its docstring).

A case passes with zero flagged elements.  Outputs are prefilled with NaN sentinels (bf16 0x7FA5, fp32 0x7FA5A5A5): padding
columns (ldo > C), rows past M, cache rows not named in kv_rows must keep them; unread input padding is NaN as well.  Every
call runs twice and the two results must be bit-identical.  Every pointer keeps the alignment its entry point documents; the
one deliberately misaligned pointer is rope2d's x, where the host tests the alignment and selects the 2-byte scalar form.

Launch forms reached.  Norms, by row width: MAXV 2 at C = 4, 160, 384, 512; MAXV 4 at 516, 1024; MAXV 6 at 1028, 1280, 1536;
MAXV 8 at 1540, 2048 - each at both ends of its range, for all four LayerNorm dtype pairs and both RMSNorm output types, at
M = 1, 3, 4, 37 (a lone row, a partial block of four, one full block, full blocks and a tail), ldx = C + 8, ldo = C + 4.
rope2d: the layouts `packed`, `ld+8` and `col0=D` reach the vec4 form at D = 16 and 96; `col0=2`, `ld+2` and `x+2B` (x one
bf16 off 8-byte alignment) reach the scalar form, each through one dispatch condition alone; every layout is scalar at
D = 40.  The test states the form from the dispatch conditions of g2v_rope2d and requires all layouts to agree bit for bit.
qk-norm: 16 (row, head) items per block; the (12, 2) cases fill whole blocks, every (2, 1) case ends in a dead tail.

Measured figures.  This module has not run on an MI355X yet (no GPU could be had when it was written), so no measured figure
is claimed here: the mRoPE bound is the 2e-6 the older test asserts (to become 2 x the measured maximum, never above 2e-6),
and the per-kernel largest error / (TAU T), the cosf / sinf maximum and the multi-valued share per case are printed by the
module's teardown (STATS lines, visible with -s) to be copied here.  The CPU emulations of the same kernels measure 0.10 - 0.11
for the norms' error / (TAU T) and 0.2 - 0.5 % multi-valued shares (rowop_check.py).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowop_check as R  # noqa: E402
from oracle import g2vlm_oracle as O  # noqa: E402  (rope2d reference only)

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
CS = [4, 160, 384, 512, 516, 1024, 1028, 1280, 1536, 1540, 2048]
MS = [1, 3, 4, 37]
FAMILIES = ["plain", "offset", "tiny", "huge", "zero"]
MROPE_BOUND = 2e-6            # |cosf / sinf - fp64| on the device; see the module docstring
STATS = {}


@pytest.fixture(scope="module", autouse=True)
def measured_maxima():
    """Prints the figures the module docstring quotes (visible with -s) once the module's tests have run."""
    yield
    for k, v in sorted(STATS.items(), key=str):
        print("STATS", k, f"{v:.3g}" if isinstance(v, float) else v)


def note(k, v):
    STATS[k] = max(STATS.get(k, 0.0), float(v))


@pytest.fixture(scope="module")
def hip():
    from g2vlm_amd import hip as h
    h.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return h


def rnd(*shape, seed=0):
    g = torch.Generator(); g.manual_seed(seed)
    return torch.randn(shape, generator=g)


def dev(t):
    return t.cuda()


def rows_of(M, C, seed):
    """[M, C] fp32, row i of family FAMILIES[i % 5]: 3 randn + 0.5, 100 + randn, 1e-3 randn, 1e4 randn, all zero."""
    z = rnd(M, C, seed=seed)
    x = torch.empty(M, C)
    fam = torch.arange(M) % 5
    for i, f in enumerate((3 * z + 0.5, 100 + z, 1e-3 * z, 1e4 * z, torch.zeros(M, C))):
        x[fam == i] = f[fam == i]
    return x, fam


def padded(x, extra, extra_rows=0):
    """A device copy of x [M, C] inside a NaN-filled [M + extra_rows, C + extra] buffer; returns (buffer, view)."""
    M, C = x.shape
    buf = R.sentinel((M + extra_rows, C + extra), x.dtype, "cuda")
    buf[:M, :C] = x.cuda()
    return buf, buf[:M, :C]


def out_buf(M, C, dtype, extra=4):
    buf = R.sentinel((M + 2, C + extra), dtype, "cuda")
    return buf, buf[:M, :C]


def assert_untouched(buf, M, C, what):
    keep = R.is_sentinel(buf)
    assert bool(keep[M:].all()) and bool(keep[:, C:].all()), f"{what}: wrote outside the [M, C] block"


def twice(run):
    """run() -> (buffer, view): both launches' whole buffers must be bit-identical."""
    b1, v1 = run()
    b2, _ = run()
    assert torch.equal(R.bits(b1), R.bits(b2)), "two launches differ"
    return b1, v1


class Share:
    """Share of bf16 outputs with more than one admissible value, pooled over the cases of one test."""

    def __init__(self):
        self.multi = self.n = 0

    def add(self, multi, n):
        self.multi += int(multi); self.n += int(n)

    def check(self, what):
        share = self.multi / max(self.n, 1)
        note(what, share)
        if self.n >= 1000:
            assert share <= R.MULTI_CAP, (what, share)


def multi_by_family(y, T, fam):
    _, _, n = R.admissible(y, T, R.TAU)
    return {f: (int((n[fam == f] > 1).sum()), int((fam == f).sum()) * y.shape[1]) for f in range(5)}


# ---------------------------------------------------------------------------------------------------- norms
@pytest.mark.parametrize("C", CS)
def test_layernorm(hip, C):
    w, b = 1 + 0.1 * rnd(C, seed=C + 1), 0.1 * rnd(C, seed=C + 2)
    wd, bd = dev(w), dev(b)
    share = {f: Share() for f in range(5)}
    for M in MS:
        x32, fam = rows_of(M, C, seed=3 * C + M)
        for xin in (x32, x32.bfloat16()):
            _, xv = padded(xin, 8)
            for eps in (1e-6, 1e-5):
                y, T = R.layernorm64(xin, w, b, eps)
                for od in (F32, BF):
                    def run():
                        buf, view = out_buf(M, C, od)
                        hip.layernorm(xv, wd, bd, eps, od, out=view)
                        return buf, view
                    buf, got = twice(run)
                    what = f"layernorm MAXV={R.maxv(C)} C={C} M={M} {xin.dtype}->{od} eps={eps}"
                    assert_untouched(buf, M, C, what)
                    res = R.check_out(got, y, T)
                    assert res.count == 0, res.report(what)
                    note(("layernorm err/(TAU T)", R.maxv(C), str(od)), res.max_ratio)
                    if od == BF:
                        for f, (m, n) in multi_by_family(y, T, fam).items():
                            share[f].add(m, n)
                    zero = fam == 4
                    if bool(zero.any()):                        # an all-zero row gives exactly b
                        assert torch.equal(got.cpu()[zero].double(), bd.cpu().to(od).double()[None].expand(int(zero.sum()), C))
    for f in range(5):
        if FAMILIES[f] != "offset":                             # the offset rows' bf16 form is exempt from the cap (rowop_check.py)
            share[f].check(("layernorm multi share", FAMILIES[f]))
        else:
            note(("layernorm multi share", "offset (exempt)"), share[f].multi / max(share[f].n, 1))


@pytest.mark.parametrize("C", CS)
def test_rmsnorm(hip, C):
    w0, w1 = 1 + 0.1 * rnd(C, seed=C + 3), 1 + 0.1 * rnd(C, seed=C + 4)
    w0d, w1d = dev(w0), dev(w1)
    share = {f: Share() for f in range(5)}
    for M in MS:
        x, fam = rows_of(M, C, seed=5 * C + M)
        _, xv = padded(x, 8)
        for split in sorted({0, 1, max(M - 1, 0), M, min(M, 18)}):          # 18: the middle of the block of rows 16 .. 19
            y, T = R.rmsnorm64(x, w0, w1, split, 1e-6)
            for od in (F32, BF):
                def run():
                    buf, view = out_buf(M, C, od)
                    hip.rmsnorm(xv, w0d, w1d, split, 1e-6, od, out=view)
                    return buf, view
                buf, got = twice(run)
                what = f"rmsnorm MAXV={R.maxv(C)} C={C} M={M} ->{od} split={split}"
                assert_untouched(buf, M, C, what)
                res = R.check_out(got, y, T)
                assert res.count == 0, res.report(what)
                note(("rmsnorm err/(TAU T)", R.maxv(C), str(od)), res.max_ratio)
                if od == BF:
                    for f, (m, n) in multi_by_family(y, T, fam).items():
                        share[f].add(m, n)
                zero = fam == 4
                if bool(zero.any()):
                    assert float(got.cpu()[zero].float().abs().max()) == 0
    for f in range(5):
        share[f].check(("rmsnorm multi share", FAMILIES[f]))


@pytest.mark.parametrize("kernel", ["layernorm", "rmsnorm"])
@pytest.mark.parametrize("C", [516, 1024, 2048])
def test_norm_depends_on_the_last_lane_of_the_last_group(hip, kernel, C):
    """x[r, C - 1] is read by one lane only - lane 63 of the last MAXV group at C = 1024 (MAXV 4) and 2048 (MAXV 8), the one
    live lane of a partial group at C = 516: changing it changes row r - that element and, through the statistics, the first
    one - and no other row."""
    M, r = 7, 5
    x = rnd(M, C, seed=C) * 3 + 0.5
    w, b = dev(1 + 0.1 * rnd(C, seed=1)), dev(0.1 * rnd(C, seed=2))
    x2 = x.clone()
    x2[r, C - 1] += 40.0
    outs = []
    for xx in (x, x2):
        _, xv = padded(xx, 8)
        buf, view = out_buf(M, C, F32)
        if kernel == "layernorm":
            hip.layernorm(xv, w, b, 1e-6, F32, out=view)
            y, T = R.layernorm64(xx, w.cpu(), b.cpu(), 1e-6)
        else:
            hip.rmsnorm(xv, w, b, 3, 1e-6, F32, out=view)
            y, T = R.rmsnorm64(xx, w.cpu(), b.cpu(), 3, 1e-6)
        assert R.check_out(view, y, T).count == 0
        outs.append(R.bits(buf.cpu()))
    changed = outs[0] != outs[1]
    assert changed.any(1).nonzero().flatten().tolist() == [r]
    assert bool(changed[r, C - 1]) and bool(changed[r, 0]) and int(changed[r].sum()) > C // 2


@pytest.mark.parametrize("kernel", ["layernorm", "rmsnorm"])
def test_norm_argument_checks(hip, kernel):
    """C > 2048, C % 4 != 0 and ldx % 4 != 0 are refused by the entry point: the wrapper raises and nothing is written."""
    for C, extra in ((2052, 0), (6, 0), (512, 2)):
        M = 4
        _, xv = padded(rnd(M, C, seed=C), extra)
        w = dev(torch.ones(max(C, 8)))
        buf, view = out_buf(M, C, BF, extra=0 if C == 6 else 4)
        with pytest.raises(hip.HipError):
            if kernel == "layernorm":
                hip.layernorm(xv, w, w, 1e-6, BF, out=view)
            else:
                hip.rmsnorm(xv, w, w, 2, 1e-6, BF, out=view)
        torch.cuda.synchronize()
        assert bool(R.is_sentinel(buf).all())


# ------------------------------------------------------------------------------------------------ mRoPE table
def positions(L, seed, top=45000):
    """[3, L] positions up to `top` on every axis, different on every axis at every row (so a wrong axis shows)."""
    g = torch.Generator(); g.manual_seed(seed)
    t = torch.randint(0, top - 2, (L,), generator=g)
    h = (t + 1 + torch.randint(0, top // 2, (L,), generator=g)) % (top + 1)
    w = (h + 1 + torch.randint(0, top // 3, (L,), generator=g)) % (top + 1)
    w = torch.where(w == t, (w + 1) % (top + 1), w)
    pos = torch.stack([t, h, w])
    pos[:, 0] = torch.tensor([top, top - 1, top - 2])
    assert bool((pos[0] != pos[1]).all() and (pos[1] != pos[2]).all() and (pos[0] != pos[2]).all())
    return pos


INV_FREQ = 1.0 / (1e6 ** (torch.arange(0, 128, 2, dtype=torch.int64).float() / 128))


@pytest.mark.parametrize("L", [1, 3, 300, 301])
def test_mrope_table(hip, L):
    """300 rows are 75 full blocks of 256 threads; 1, 3 and 301 end in a partial block, which must write nothing past row L."""
    pos = positions(L, seed=L)
    pd, inv = dev(pos.to(torch.int32)), dev(INV_FREQ)

    def run():
        buf = R.sentinel((2, L + 1, 128), F32, "cuda")
        hip.mrope_table_into(pd, inv, buf[0, :L], buf[1, :L])
        return buf, buf[:, :L]
    buf, got = twice(run)
    assert bool(R.is_sentinel(buf[:, L:]).all())
    bad, err = R.check_mrope_table(got[0], got[1], pos, INV_FREQ, MROPE_BOUND)
    note(("mrope_table max |got - ref|",), err)
    assert int(bad.sum()) == 0, f"L={L}: {int(bad.sum())} flagged, first at {bad.nonzero()[0].tolist()}, max err {err:.3g}"


# ------------------------------------------------------------------------------ qk-norm + mRoPE + cache write
def qk_inputs(L, Hq, Hkv, seed):
    qkv = rnd(L, (Hq + 2 * Hkv) * 128, seed=seed).bfloat16()
    ws = [1 + 0.1 * rnd(128, seed=seed + 1 + i) for i in range(4)]               # q_lo q_hi k_lo k_hi
    c64, s64 = R.mrope_table64(positions(L, seed + 7, top=2000), INV_FREQ)
    g = torch.Generator(); g.manual_seed(seed + 8)
    rows = (torch.randperm(L + 3, generator=g)[:L] * 2 + 1).to(torch.int32)      # a permutation with gaps into 2 L + 8 rows
    return qkv, ws, c64.float(), s64.float(), rows


def qk_run(hip, qkv, Hq, Hkv, ws, split, und, cos, sin, rows):
    """Launches twice into fresh sentinel buffers (q_out with one row to spare); returns the check and (q_out, k, v)."""
    L = qkv.shape[0]
    dq, dw, dc, ds, dr = dev(qkv), [dev(w) for w in ws], dev(cos), dev(sin), dev(rows)
    kb, vb = R.sentinel((2 * L + 8, Hkv, 128), BF), R.sentinel((2 * L + 8, Hkv, 128), BF)

    def run():
        qo, ka, va = R.sentinel((L + 1, Hq, 128), BF, "cuda"), dev(kb), dev(vb)
        hip.qknorm_mrope_cache(dq, Hq, Hkv, *dw, split, 1e-6, und, dc, ds, qo[:L], ka, va, dr)
        return qo, ka, va
    first, second = run(), run()
    for a, b in zip(first, second):
        assert torch.equal(R.bits(a), R.bits(b)), "two launches differ"
    qo, ka, va = first
    assert bool(R.is_sentinel(qo[L:]).all()), "q_out written past row L"
    return R.check_qknorm_mrope_cache(qkv, Hq, Hkv, *ws, split, 1e-6, und, cos, sin, rows, qo[:L], kb, ka, vb, va), (qo, ka, va)


@pytest.mark.parametrize("und", [0, 1])
@pytest.mark.parametrize("Hq,Hkv", [(12, 2), (2, 1)])
def test_qknorm_mrope_cache(hip, und, Hq, Hkv):
    """16 (row, head) items per block: L (Hq + 2 Hkv) is a multiple of 16 only at (12, 2), L = 1, 3, 7, 45; every other
    case ends in a partial block whose dead lanes re-read item 0 and must write nothing."""
    for L in (1, 3, 7, 45):
        qkv, ws, cos, sin, rows = qk_inputs(L, Hq, Hkv, seed=100 * L + Hq)
        for split in sorted({0, L, L // 2}):
            res, _ = qk_run(hip, qkv, Hq, Hkv, ws, split, und, cos, sin, rows)
            what = f"qknorm und={und} Hq={Hq} Hkv={Hkv} L={L} split={split} items%16={L * (Hq + 2 * Hkv) % 16}"
            assert res.count == 0, res.report(what)
            note(("qknorm err/(TAU T)", und), res.max_ratio)
            note(("qknorm multi share", und, (Hq, Hkv), L), res.multi_share)
            assert res.multi_share <= R.MULTI_CAP, (what, res.multi_share)


@pytest.mark.parametrize("Hq,Hkv", [(12, 2), (2, 1)])
def test_qknorm_mrope_cache_as_the_decode_step_calls_it(hip, Hq, Hkv):
    """decode.py: one row, split = 0, the same weight as lo and hi, und_rounding = 1."""
    qkv, ws, cos, sin, rows = qk_inputs(1, Hq, Hkv, seed=77)
    ws = [ws[0], ws[0], ws[2], ws[2]]
    res, _ = qk_run(hip, qkv, Hq, Hkv, ws, 0, 1, cos, sin, rows)
    assert res.count == 0, res.report("decode call")
    assert res.multi_share <= R.MULTI_CAP


def test_qknorm_depends_on_the_last_live_item_of_a_partial_block(hip):
    """Hq = 2, Hkv = 1, L = 7: 28 items, the second block holds 12 live ones.  The last item is row 6's V head, the one
    before it row 6's K head: changing one input element of each changes exactly that V element, exactly that K head row."""
    Hq, Hkv, L = 2, 1, 7
    qkv, ws, cos, sin, rows = qk_inputs(L, Hq, Hkv, seed=9)
    _, (q0, k0, v0) = qk_run(hip, qkv, Hq, Hkv, ws, 3, 1, cos, sin, rows)
    q2 = qkv.clone()
    q2[L - 1, -1] = -q2[L - 1, -1] + 1.0                                  # V, dim 127
    q2[L - 1, (Hq + Hkv) * 128 - 1] = q2[L - 1, (Hq + Hkv) * 128 - 1] * 3 + 4.0   # K, dim 127
    res, (q1, k1, v1) = qk_run(hip, q2, Hq, Hkv, ws, 3, 1, cos, sin, rows)
    assert res.count == 0, res.report("perturbed")
    assert torch.equal(R.bits(q0), R.bits(q1))
    tgt = int(rows[L - 1])
    dv = (R.bits(v0) != R.bits(v1)).nonzero().tolist()
    assert dv == [[tgt, 0, 127]], dv
    dk = R.bits(k0) != R.bits(k1)
    assert dk.any(-1).nonzero().tolist() == [[tgt, 0]] and bool(dk[tgt, 0, 127]) and bool(dk[tgt, 0, 63]) and int(dk.sum()) > 64


# ---------------------------------------------------------------------------------------------------- rope2d
def rope2d_expected(buf, col0, n_heads, D, pos, N, P):
    """bf16 eager arithmetic of the reference (oracle rope2d) on columns [col0, col0 + n_heads D) of every row."""
    want = buf.clone()
    t = buf[:, col0:col0 + n_heads * D].reshape(N, P, n_heads, D).transpose(1, 2)
    r = O.rope2d(t, pos.view(1, P, 2).expand(N, -1, -1))
    want[:, col0:col0 + n_heads * D] = r.transpose(1, 2).reshape(N * P, n_heads * D)
    return want


ROPE2D_LAYOUTS = {                 # name: (col0, extra ld, element offset of x, heads skipped)
    "packed": (0, 0, 0, 0), "ld+8": (0, 8, 0, 0), "col0=D": (None, 0, 0, 1),
    "col0=2": (2, 4, 0, 0), "ld+2": (0, 2, 0, 0), "x+2B": (0, 0, 1, 0),
}


@pytest.mark.parametrize("D", [16, 96, 40])
def test_rope2d(hip, D):
    """Two views (row % P wraps), q and k heads rotated in place, V columns and padding untouched.  The vec4 form needs
    D % 16 == 0, ld % 4 == 0, col0 % 4 == 0 and an 8-byte aligned x; each layout below breaks at most one of them, and the
    results of all layouts on the same tokens must agree bit for bit (vec4 against scalar)."""
    N, gh, gw, Hh = 2, 3, 5, 2
    P, M, packed = gh * gw, 2 * gh * gw, 3 * Hh * D
    tok = rnd(M, packed, seed=D).bfloat16()
    pos = torch.cartesian_prod(torch.arange(gh), torch.arange(gw))
    cos, sin = O.rope2d_tables(D // 2, max(gh, gw), BF)
    dc, ds, dp = dev(cos), dev(sin), dev(pos.to(torch.int32))
    rotated = {}
    for name, (col0, extra, off, skip) in ROPE2D_LAYOUTS.items():
        col0 = D * skip if col0 is None else col0
        n_heads = 2 * Hh - skip
        ld = packed + extra
        lay = R.sentinel((M, ld), BF)
        c_tok = col0 - D * skip
        lay[:, c_tok:c_tok + packed] = tok
        vec4 = D % 16 == 0 and ld % 4 == 0 and col0 % 4 == 0 and off == 0
        note(("rope2d form", D, name), 4.0 if vec4 else 1.0)

        def run():
            flat = R.sentinel((M * ld + 8,), BF, "cuda")
            x = flat[off:off + M * ld].view(M, ld)
            x.copy_(lay)
            assert (x.data_ptr() % 8 == 0) == (off == 0)
            hip.rope2d(x, col0, n_heads, D, dc, ds, dp, P)
            return flat, x
        flat, x = twice(run)
        want = rope2d_expected(lay, col0, n_heads, D, pos, N, P)
        assert torch.equal(R.bits(x.cpu()), R.bits(want)), f"rope2d D={D} {name} ({'vec4' if vec4 else 'scalar'})"
        keep = R.is_sentinel(flat)
        assert bool(keep[:off].all() and keep[off + M * ld:].all())
        if not skip:
            rotated[name] = R.bits(x.cpu()[:, c_tok:c_tok + packed])
            assert torch.equal(rotated[name], rotated["packed"]), f"{name} differs from the packed layout"
            assert torch.equal(x.cpu()[:, c_tok + 2 * Hh * D:c_tok + packed], tok[:, 2 * Hh * D:])       # V untouched
    if D % 16 == 0:
        assert {STATS[("rope2d form", D, n)] for n in ("packed", "ld+8", "col0=D")} == {4.0}
        assert {STATS[("rope2d form", D, n)] for n in ("col0=2", "ld+2", "x+2B")} == {1.0}


@pytest.mark.parametrize("D", [16, 96])
def test_rope2d_depends_on_the_last_pair(hip, D):
    """The last rotation pair of the last row and head is the last live lane's: changing its second element changes exactly
    that pair."""
    gh, gw, Hh = 3, 5, 2
    P, M, packed = gh * gw, 2 * gh * gw, 3 * Hh * D
    tok = rnd(M, packed, seed=D + 1).bfloat16()
    pos = torch.cartesian_prod(torch.arange(gh), torch.arange(gw))
    cos, sin = O.rope2d_tables(D // 2, max(gh, gw), BF)
    tok2 = tok.clone()
    last = 2 * Hh * D - 1                                                  # second element of the last x-axis pair
    tok2[M - 1, last] = tok2[M - 1, last] * 2 + 1.0
    outs = []
    for t in (tok, tok2):
        x = dev(t).clone()
        hip.rope2d(x, 0, 2 * Hh, D, dev(cos), dev(sin), dev(pos.to(torch.int32)), P)
        outs.append(R.bits(x.cpu()))
    assert (outs[0] != outs[1]).nonzero().tolist() == [[M - 1, last - D // 4], [M - 1, last]]


# ----------------------------------------------------------------------------------------------- rope_vision
@pytest.mark.parametrize("D", [80, 64])
@pytest.mark.parametrize("L", [1, 64])
def test_rope_vision(hip, D, L):
    Hh = 3
    ld = 3 * Hh * D + 8
    lay = R.sentinel((L, ld), BF)
    lay[:, :3 * Hh * D] = rnd(L, 3 * Hh * D, seed=42 + D + L).bfloat16()
    ang = rnd(L, D // 2, seed=43 + D + L) * 3
    emb = torch.cat([ang, ang], -1)
    cos, sin = emb.cos(), emb.sin()
    sin[:, D // 2:] = (ang * 1.0001).sin()                                  # the two halves of the tables are read separately
    dc, ds = dev(cos), dev(sin)

    def run():
        buf = R.sentinel((L + 1, ld), BF, "cuda")
        buf[:L] = dev(lay)
        hip.rope_vision(buf[:L], 2 * Hh, D, dc, ds)
        return buf, buf[:L]
    buf, x = twice(run)
    assert bool(R.is_sentinel(buf[L:]).all())
    want = R.rope_vision_emul(lay, 2 * Hh, D, cos, sin)
    assert torch.equal(R.bits(x.cpu()), R.bits(want)), f"rope_vision D={D} L={L}: {int((R.bits(x.cpu()) != R.bits(want)).sum())} differ"
    lay2 = lay.clone()
    last = 2 * Hh * D - 1                                                   # read by the last live lane only
    lay2[L - 1, last] = lay2[L - 1, last] * 2 + 1.0
    buf2 = R.sentinel((L + 1, ld), BF, "cuda")
    buf2[:L] = dev(lay2)
    hip.rope_vision(buf2[:L], 2 * Hh, D, dc, ds)
    assert (R.bits(buf2.cpu()) != R.bits(buf.cpu())).nonzero().tolist() == [[L - 1, last - D // 2], [L - 1, last]]


# --------------------------------------------------------------------------------------------- casts, movers
def cast_input(n):
    """`1e3 randn` and `1e-3 randn` values followed by cast_table() (n = 4: NaN, -inf, a tie and the overflow threshold)."""
    tab = R.cast_table()
    if n < tab.numel():
        return tab[torch.tensor([0, 2, 13, 21])][:n]
    z = rnd(n - tab.numel(), seed=n)
    z[::2] *= 1e3
    z[1::2] *= 1e-3
    return torch.cat([z, tab])


@pytest.mark.parametrize("n", [4, 1028, 4 * (2 ** 18 + 1)])
def test_cast_f32_bf16(hip, n):
    """Expected: torch's own round-to-nearest-even conversion on the CPU, bit for bit.  A NaN must give a NaN: its payload is
    not compared, because torch's own CPU conversion gives 0x7FC0 or 0xFFFF for the same NaN depending on the code path."""
    src = cast_input(n)
    want = src.bfloat16()
    ds = dev(src)

    def run():
        buf = R.sentinel((n + 8,), BF, "cuda")
        hip._ck(hip.lib().g2v_cast_f32_bf16(hip._p(ds), hip._p(buf), n, hip._stream()), "g2v_cast_f32_bf16")
        return buf, buf[:n]
    buf, got = twice(run)
    assert bool(R.is_sentinel(buf[n:]).all())
    got = got.cpu()
    nan = torch.isnan(src)
    assert torch.equal(torch.isnan(got.float()), nan)
    diff = (R.bits(got) != R.bits(want)) & ~nan
    assert not bool(diff.any()), [hex(int(v) & 0xFFFFFFFF) for v in R.bits(src)[diff][:8]]
    assert torch.equal(R.bits(hip.cast_bf16(ds).cpu()), R.bits(got))          # the wrapper, same bits


def test_cast_f32_bf16_keeps_every_nan_a_nan(hip):
    src = R.cast_nan_table()
    got = hip.cast_bf16(dev(src)).cpu()
    assert bool(torch.isnan(got.float()).all()), [hex(int(v) & 0xFFFF) for v in R.bits(got)]


def test_cast_bf16_f32_every_pattern(hip):
    pat = torch.arange(65536, dtype=torch.int32)
    src = (pat - (pat >= 32768) * 65536).to(torch.int16).view(BF)
    ds = dev(src)

    def run():
        buf = R.sentinel((65536 + 4,), F32, "cuda")
        hip._ck(hip.lib().g2v_cast_bf16_f32(hip._p(ds), hip._p(buf), 65536, hip._stream()), "g2v_cast_bf16_f32")
        return buf, buf[:65536]
    buf, got = twice(run)
    assert bool(R.is_sentinel(buf[65536:]).all())
    got = got.cpu()
    nan = torch.isnan(src.float())
    assert int(nan.sum()) == 2 * 127
    assert torch.equal(torch.isnan(got), nan)                                    # NaN stays NaN
    assert torch.equal(R.bits(got)[~nan], (pat << 16)[~nan])                     # everything else: the same bits, 16 zeros appended
    assert torch.equal(R.bits(hip.cast_f32(ds).cpu())[~nan], R.bits(got)[~nan])  # the wrapper, same bits


@pytest.mark.parametrize("C", [4, 1536])
@pytest.mark.parametrize("rows", [1, 20])
def test_row_movers(hip, C, rows):
    """Padded ld_src and ld_dst; rows x C / 4 float4 moves are 1, 20, 384 and 7680: three partial blocks of 256 and one exact."""
    src = rnd(50, C, seed=C + rows)
    src[0, 0], src[1, 0], src[2, 0] = float("nan"), float("-inf"), -0.0      # moved as bits
    idx = torch.randperm(50, generator=torch.Generator().manual_seed(rows))[:rows].to(torch.int32)
    _, sv = padded(src, 4)
    di = dev(idx)

    def gather():
        buf, view = out_buf(rows, C, F32, extra=8)
        hip.gather_rows(sv, di, view)
        return buf, view
    buf, got = twice(gather)
    assert_untouched(buf, rows, C, "gather")
    assert torch.equal(R.bits(got.cpu()), R.bits(src[idx.long()]))

    _, sv2 = padded(src[:rows], 4)

    def scatter():
        buf = R.sentinel((50, C + 8), F32, "cuda")
        hip.scatter_rows(sv2, di, buf[:, :C])
        return buf, buf[:, :C]
    buf, got = twice(scatter)
    want = R.sentinel((50, C + 8), F32)
    want[idx.long(), :C] = src[:rows]
    assert torch.equal(R.bits(buf.cpu()), R.bits(want))                          # unaddressed rows and padding keep the sentinel
