"""GPU: flash attention (csrc/attn.hip) checked ROW BY ROW against an fp64 reference.

The attention tests of test_kernels_gpu.py bound one global rel-L2 over a whole output.  A kernel that gets a few rows
wrong (one 256-row tile loses the last key of its window, a wrong causal diagonal in one tile, a rescale slip in the rows
of one 32-row block whose maximum grew) moves that number by a few 1e-3 and passes.  Here every (query row, head) inside a
window is held to a bound of its own:

    r     = RMS over d of the fp64 reference row
    e_max = max_d |got - ref| / r
    e_row = ||got - ref|| / ||ref||

and the global rel-L2 bound of the older tests (6e-3) is kept on top.  test_row_metric_flags_one_narrowed_tile shows why:
a plan with one tile narrowed by one key is flagged row-exactly while its global rel-L2 stays under 6e-3.

The reference (ref_fp64) is plain torch float64 matmul / softmax on the device - no project kernel - over the exact bf16
tensors the kernel reads, chunked by kv head and query block; test_fp64_reference_matches_oracle ties it to the oracle's
varlen_attention(precise=True) on a small case.

Every case also guards what the kernel must NOT touch: the window sits at q0 > 0 / k0 > 0 (edge sweeps), every Q / K / V
element it must not read (rows outside the windows, stride padding) is NaN - a read of a V row outside the window
surfaces as NaN since 0 x NaN = NaN - and the output is pre-filled with a NaN bit pattern carrying a payload (0x7FA5) in a
buffer with ldo > Hq*D: rows outside every window and columns [Hq*D, ldo) must keep those bits.  The production cases
(section 5) keep their call sites' strides, with NaN wherever the layout holds memory the kernel must not read (the DINO
tail rows, the KV cache rows past the attended length).

Forms (launch_flash picks the kernel from D, tile_rows = 32 x waves and ldk == ldv; engine.attn_tile_rows picks tile_rows):

    kernel                  D    waves  layout pinned                                          test
    flash_fwd_kernel<D,4>   16   4      padded strides, 4:4 heads                              test_edge_sweep[16-*]
    flash_fwd_kernel<D,8>   16   8      padded strides, 4:4 heads                              test_edge_sweep[16-*]
    flash_fwd_kernel<64,4>  64   4      DINO C2: packed qkv ld 3072, 2 x 777 over 2 x 782      test_dino[C2], test_edge_sweep[64-*]
    flash_fwd_kernel<64,8>  64   8      DINO C3: packed qkv ld 3072, 8 x 1369 over 8 x 1374    test_dino[C3], test_edge_sweep[64-*]
    flash_fwd_kernel<80,4>  80   4      padded strides, 4:4 heads                              test_edge_sweep[80-*]
    flash_fwd_kernel<80,8>  80   8      ViT: packed qkv ld 3840, 1 and 8 x 2916               test_vit, test_edge_sweep[80-*]
    flash_fwd_kernel<96,4>  96   4      decoder C2: self ld 4608 / cross q 1536, K/V 3072      test_decoder[*C2], test_edge_sweep[96-*]
    flash_fwd_kernel<96,8>  96   8      decoder C3: self ld 4608 / cross q 1536, K/V 3072      test_decoder[*C3], test_edge_sweep[96-*]
    flash_fwd_kernel<128,4> 128  4      MoT C2, causal text prompt, ViT staircase; q 1536 / cache 256   test_mot, test_edge_sweep[128-*]
    flash_fwd_kernel<128,8> 128  8      form 0 (g2v_debug_attn_form), padded strides, 12:2    test_edge_sweep[128-*]
    flash_fwd64_kernel      128  4x64   MoT C3, view-sharded C4 phases; q 1536 / cache 256     test_mot, test_c4_rank_phases, test_edge_sweep[128-*], test_fwd64_rescale_threshold
    flash_combine_kernel    all  -      every edge case again at max_blocks 3 and 7; C4 phases test_edge_sweep, test_c4_rank_phases
Every row of this table runs again in tests/test_flash_profile_gpu.py on structured score profiles (one key or one tile carries
the row, equal weights, +-250 offsets, steps of up to 200 per KV tile; max_blocks None / 3 / 7), every ELEMENT against fp64 under
bounds derived from the kernels' arithmetic instead of measured on them (tests/flash_profile_check.py).

Bounds.  Rule: every case is measured under its production form and under the 4-wave 128-row form on the same inputs;
the bound of a head dim is 1.5 x the largest e_max / e_row measured for that D over all cases and forms on an MI355X.
A form may not be materially less accurate than the 4-wave form on the same inputs: global error <= 1.5 x the 4-wave
form's + 1e-4 (as in the 4 x 64 form test).  Measured maxima over all cases and forms (first MI355X run of this module,
1232 launches) and the bounds derived from them:

    D     max e_max  (case)                          max e_row  (case)                    bound e_max  bound e_row
    16    1.617e-2   growth, alternating sub-blocks  5.81e-3    causal 257 x 257           2.43e-2      8.72e-3
    64    1.909e-2   DINO C3                         3.624e-3   DINO C3                    2.87e-2      5.44e-3
    80    1.912e-2   ViT 8 images                    3.553e-3   ViT 8 images               2.87e-2      5.33e-3
    96    1.808e-2   decoder self C2                 3.406e-3   decoder cross C3           2.72e-2      5.11e-3
    128   2.236e-2   Lq 549 x Lk 150, fwd64          3.927e-3   causal 65 x 65, fwd64      3.36e-2      5.90e-3

No case stood apart from the others of its D.  flash_fwd64_kernel is the least accurate form at D = 128 (its softmax
reference is a power of two, so a row's largest p is rounded to bf16 like every other p; e_max 2.24e-2 against 1.74e-2 of
the 4-wave form on the same inputs), within the 1.5 x + 1e-4 rule.  The 8-wave generic forms match the 4-wave form to the
printed digits.  The narrowed tile of the sensitivity test measures e_row >= 1.6e-2 and e_max >= 3.5e-2 on every
affected row (3x and 1.2x the D = 64 bounds), every other row stays under them, and its global rel-L2 is 3.6e-3 - 4.5e-3.
The whole module runs in about 7 s on one MI355X.
"""
import copy
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
# shared with tests/test_flash_profile_gpu.py and kept in its helper module: the fp64 reference, the guarded launch, the padded
# inputs, the form table and the row bounds BOUND[D] (per head dim (e_max, e_row): the rule and the measured maxima are above)
from flash_profile_check import (BOUND, GLOBAL_REL, K0, NAN_BITS, Q0, SWEEP_DS, attn_form, covered_rows, forms, heads,  # noqa: E402,F401
                                 launch, nan_bf16, padded_inputs, ref_fp64)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from g2vlm_amd import hip as h
    h.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return h


def gen(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def randn(g, *shape, scale=1.0):
    return torch.randn(shape, generator=g, device="cuda") * scale


# ------------------------------------------------------------------------------------------------ reference and metric
class Errors:
    """Row metric of one launch: e_max / e_row per (row, head) of every window, and the global rel-L2."""

    def __init__(self, got, ref, Hq, D):
        num = den = 0.0
        self.e_max, self.e_row = {}, {}
        for (q0, ql), r in ref.items():
            g = got[q0:q0 + ql, :Hq * D].double().view(ql, Hq, D)
            d = g - r
            rn = r.norm(dim=-1)
            self.e_max[q0] = d.abs().amax(dim=-1) / (rn / math.sqrt(D))
            self.e_row[q0] = d.norm(dim=-1) / rn
            num += float((d * d).sum())
            den += float((r * r).sum())
        self.rel = math.sqrt(num / den)
        self.max_e_max = max(float(x.max()) for x in self.e_max.values())
        self.max_e_row = max(float(x.max()) for x in self.e_row.values())

    def flagged(self, D):
        bm, br = BOUND[D]
        return {q0: (self.e_max[q0] > bm) | (self.e_row[q0] > br) for q0 in self.e_max}


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def check_bounds(err, D, what):
    bm, br = BOUND[D]
    print(f"ATTN-ROW D={D} {what}: e_max {err.max_e_max:.3e} e_row {err.max_e_row:.3e} rel {err.rel:.3e}")
    assert err.rel < GLOBAL_REL, (what, err.rel)
    assert err.max_e_max <= bm and err.max_e_row <= br, (what, err.max_e_max, err.max_e_row, BOUND[D])


def check_vs_4wave(e_prod, e_4w, what):
    assert e_prod.rel <= 1.5 * e_4w.rel + 1e-4, (what, e_prod.rel, e_4w.rel)


def test_fp64_reference_matches_oracle():
    """ref_fp64 (chunked, device) against the oracle's varlen_attention(precise=True) (CPU, whole score matrix): two windows,
    one causal with Lk > Lq, GQA 6:2, and blocks small enough that the chunking is exercised."""
    from oracle import g2vlm_oracle as O
    Hq, Hkv, D = 6, 2, 32
    g = gen(1)
    q, k, v = randn(g, 300, Hq * D).bfloat16(), randn(g, 420, Hkv * D).bfloat16(), randn(g, 420, Hkv * D).bfloat16()
    wins = [(0, 100, 0, 180, True), (100, 200, 180, 240, False)]
    ref = ref_fp64(q, k, v, wins, Hq, Hkv, D)
    for (qs, ql, ks, kl, causal) in wins:
        want = O.varlen_attention(q.cpu().double().view(-1, Hq, D), k.cpu().double().view(-1, Hkv, D), v.cpu().double().view(-1, Hkv, D),
                                  [0, qs, qs + ql], [0, ks, ks + kl], causal, precise=True)[qs:qs + ql]
        assert float((ref[(qs, ql)].cpu() - want).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ edge sweeps (section 3)
def run_forms(hip, q, k, v, wins, Hq, Hkv, D, what, max_blocks_list=(None, 3, 7)):
    """Every form of D x every max_blocks on one input; row bounds on each, and each 8-wave form against the 4-wave form."""
    ref = ref_fp64(q, k, v, wins, Hq, Hkv, D)
    n_rows, ldo = q.shape[0], Hq * D + 36
    for mb in max_blocks_list:
        errs = {}
        for name, tile_rows, f in forms(D):
            plan = hip.make_attn_plan(wins, Hq, "cuda", max_blocks=mb, tile_rows=tile_rows)
            with attn_form(hip, f):
                out = launch(hip, q, k, v, plan, Hq, Hkv, D, wins, n_rows, ldo)
            errs[name] = e = Errors(out, ref, Hq, D)
            check_bounds(e, D, f"{what} {name} mb={mb}")
        for name in errs:
            check_vs_4wave(errs[name], errs["4w"], f"{what} {name} mb={mb}")


LK_SWEEP = [1, 2, 63, 64, 65, 127, 128, 129, 357]
LQ_SWEEP = [1, 31, 32, 33, 63, 65, 127, 128, 129, 255, 256, 257, 2 * 128 + 37, 2 * 256 + 37]
CAUSAL_SWEEP = [(1, 1), (33, 33), (65, 65), (129, 129), (257, 257), (100, 164), (257, 300), (37, 1000)]


@pytest.mark.parametrize("sweep", ["lk", "lq", "causal"])
@pytest.mark.parametrize("D", SWEEP_DS)
def test_edge_sweep(hip, D, sweep):
    """Every kernel instantiation of D at the window edges where tiles go wrong: key counts around the 64-key tile, query
    counts around the 32-row wave block and the 128 / 256-row item, causal diagonals crossing 32-, 64- and item-row
    boundaries; each at the plan's own schedule and again cut into stream-K pieces (max_blocks 3 and 7: the combine pass)."""
    Hq, Hkv = heads(D)
    cases = {"lk": [(77, lk, False) for lk in LK_SWEEP], "lq": [(lq, 150, False) for lq in LQ_SWEEP],
             "causal": [(lq, lk, True) for lq, lk in CAUSAL_SWEEP]}[sweep]
    for i, (Lq, Lk, causal) in enumerate(cases):
        g = gen(1000 * D + 10 * i + len(sweep))
        q, k, v = padded_inputs(Lq, Lk, Hq, Hkv, D, randn(g, Lq, Hq * D), randn(g, Lk, Hkv * D), randn(g, Lk, Hkv * D))
        run_forms(hip, q, k, v, [(Q0, Lq, K0, Lk, causal)], Hq, Hkv, D, f"{sweep} Lq={Lq} Lk={Lk}")


def growth_inputs(g, Lq, Lk, Hq, Hkv, D, step_log2, alt=False, jump_at=None):
    """Scores s(i, j) = noise + a_i * b_j with a common direction u: b_j grows by `step_log2` (log2 domain, after the softmax
    scale) at every 64-key tile - or, with jump_at, once, at that tile - so a row's maximum grows at every (that) KV tile.
    alt: only the rows of even 32-row sub-blocks carry the growth (a_i = 0 on the others)."""
    c = D ** -0.5 * math.log2(math.e)
    u = torch.nn.functional.normalize(randn(g, D), dim=0)
    a = 8.0
    x, y = randn(g, Lq, Hq, D, scale=0.5), randn(g, Lk, Hkv, D)
    x, y = x - (x @ u)[..., None] * u, y - (y @ u)[..., None] * u
    t = torch.arange(Lk, device="cuda") // 64
    lvl = (t >= jump_at).double() if jump_at is not None else t.double()
    b = (step_log2 * lvl / (a * c)).float()
    ai = torch.full((Lq,), a, device="cuda")
    if alt:
        ai[(torch.arange(Lq, device="cuda") // 32) % 2 == 1] = 0.0
    q = x + ai[:, None, None] * u
    k = y + b[:, None, None] * u
    return q, k, randn(g, Lk, Hkv, D)


@pytest.mark.parametrize("D", SWEEP_DS)
def test_growth_at_every_tile(hip, D):
    """The online-softmax rescale (guide: 'rows whose max grew at that tile come out wrong ... silent'): the score rises tile
    by tile along q's direction, so every row's maximum grows at every KV tile; then only the rows of alternating 32-row
    sub-blocks rise, so the rescale decision differs between the row blocks of one item.  Non-causal and causal."""
    Hq, Hkv = heads(D)
    for i, (Lq, Lk, causal, alt) in enumerate([(200, 357, False, False), (200, 357, False, True), (300, 420, True, False),
                                               (300, 420, True, True)]):
        g = gen(7000 + 10 * D + i)
        qv, kv, vv = growth_inputs(g, Lq, Lk, Hq, Hkv, D, step_log2=3.0, alt=alt)
        q, k, v = padded_inputs(Lq, Lk, Hq, Hkv, D, qv, kv, vv)
        run_forms(hip, q, k, v, [(Q0, Lq, K0, Lk, causal)], Hq, Hkv, D, f"growth Lq={Lq} Lk={Lk} causal={causal} alt={alt}")


@pytest.mark.parametrize("jump", [60.0, 68.0])
def test_fwd64_rescale_threshold(hip, jump):
    """flash_fwd64_kernel fixes its softmax reference from a segment's first tile and raises it only when a row maximum
    outgrows it by more than RESCALE_THR = 64 (log2 domain): a jump of 60 stays under it, 68 takes the cold path - for all
    rows, for alternating 32-row sub-blocks, and (causal, max_blocks 7 at 12:2 heads, 3 at 4:2) in stream-K segments whose
    first tile is fully masked for some rows (reference from -1e30)."""
    D, (Hq, Hkv) = 128, heads(128)
    for i, (Lq, Lk, alt) in enumerate([(200, 357, False), (200, 357, True)]):
        g = gen(8000 + i + int(jump))
        qv, kv, vv = growth_inputs(g, Lq, Lk, Hq, Hkv, D, step_log2=jump, alt=alt, jump_at=3)
        q, k, v = padded_inputs(Lq, Lk, Hq, Hkv, D, qv, kv, vv)
        run_forms(hip, q, k, v, [(Q0, Lq, K0, Lk, False)], Hq, Hkv, D, f"jump {jump} alt={alt}")
    Lq, Lk = 200, 500
    wins = [(Q0, Lq, K0, Lk, True)]
    for Hq, Hkv, mb in ((12, 2, 7), (4, 2, 3)):
        plan = hip.make_attn_plan(wins, Hq, "cpu", max_blocks=mb, tile_rows=256)
        tiles, segs = plan.tiles.numpy().reshape(-1, 8), plan.phases[0][0].numpy().reshape(-1, 8)
        masked_first = [s for s in segs[:int(plan.phases[0][1][-1])] if s[2] > 0
                        and (tiles[s[0]][0] - tiles[s[0]][5]) + tiles[s[0]][4] < 64 * s[2]]
        assert masked_first, "no stream-K segment starts on a tile that is fully masked for its first rows"
        g = gen(8100 + Hq + int(jump))
        qv, kv, vv = growth_inputs(g, Lq, Lk, Hq, Hkv, D, step_log2=jump, jump_at=6)
        q, k, v = padded_inputs(Lq, Lk, Hq, Hkv, D, qv, kv, vv)
        run_forms(hip, q, k, v, wins, Hq, Hkv, D, f"jump {jump} causal {Hq}:{Hkv} mb={mb}", max_blocks_list=(mb,))


# ------------------------------------------------------------------------------------------------ sensitivity (section 2)
def narrowed(plan, desc, field, delta):
    """A copy of `plan` whose tile descriptor `desc` has `field` (3 = k_len, 4 = causal_shift) moved by delta."""
    p2 = copy.copy(plan)
    p2.tiles = plan.tiles.clone()
    p2.tiles[desc, field] += delta
    p2._by_owner = {}
    return p2


@pytest.mark.parametrize("variant", ["k_len", "causal_shift"])
def test_row_metric_flags_one_narrowed_tile(hip, variant):
    """Why the row metric exists.  The C3 DINO plan (8 x 1369-row windows over 8 x 1374 rows, 256-row items) with ONE
    256-row tile narrowed by one key - k_len - 1 (window 3, rows 512-767), or, on a causal plan with Lk > Lq,
    causal_shift - 1 (window 5, rows 1024-1279) - must be flagged on exactly that tile's rows (every head) and on no other
    row, while the global rel-L2 of the same output stays under the 6e-3 the aggregate tests use.  Near-uniform scores
    (small q) make every affected row lose ~1/sqrt(keys) of its value.  Both changes only narrow the visible keys."""
    from g2vlm_amd.engine import attn_tile_rows
    Hq, D, P, N = 16, 64, 1369, 8
    C = Hq * D
    g = gen(4242)
    if variant == "k_len":
        Lk, win, t0, field = P, 3, 512, 3
        wins = tuple((i * P, P, i * P, P, False) for i in range(N))
    else:
        Lk, win, t0, field = 1600, 5, 1024, 4
        wins = tuple((i * P, P, i * Lk, Lk, True) for i in range(N))
    rows = N * (P + 5)
    q = randn(g, rows, C, scale=0.05).bfloat16()
    k, v = randn(g, N * Lk + 40, C).bfloat16(), randn(g, N * Lk + 40, C).bfloat16()
    tile_rows = attn_tile_rows(wins, Hq)
    assert tile_rows == 256
    plan = hip.make_attn_plan(wins, Hq, "cuda", tile_rows=tile_rows)
    tiles = plan.tiles.cpu()
    desc = int(((tiles[:, 0] == win * P + t0) & (tiles[:, 5] == win * P)).nonzero()[0])
    assert int(tiles[desc, 1]) == 256
    if variant == "k_len":
        assert Lk % 64 != 1                                   # no KV tile becomes empty
    bad = narrowed(plan, desc, field, -1)
    ref = ref_fp64(q, k, v, wins, Hq, Hq, D)
    ldo = C + 36
    good = Errors(launch(hip, q, k, v, plan, Hq, Hq, D, wins, rows, ldo), ref, Hq, D)
    check_bounds(good, D, f"sensitivity {variant} unchanged plan")
    err = Errors(launch(hip, q, k, v, bad, Hq, Hq, D, wins, rows, ldo), ref, Hq, D)
    flagged, mismatch = err.flagged(D), []
    for q0, f in flagged.items():
        want = torch.zeros_like(f)
        if q0 == win * P:
            want[t0:t0 + 256] = True
        if want.any():
            print(f"ATTN-SENS {variant}: affected rows e_row min {float(err.e_row[q0][want].min()):.3e}, "
                  f"e_max min {float(err.e_max[q0][want].min()):.3e}; other rows of the window e_row max "
                  f"{float(err.e_row[q0][~want].max()):.3e}, e_max max {float(err.e_max[q0][~want].max()):.3e}")
        if not torch.equal(f, want):
            mismatch.append((q0 // P, int(f.sum()), int(want.sum()), int((f & want).sum())))
    print(f"ATTN-SENS {variant}: global rel-L2 {err.rel:.3e} (unchanged plan {good.rel:.3e}); mismatches {mismatch}")
    assert not mismatch, mismatch                             # (window, flagged, expected, flagged and expected)
    assert err.rel < GLOBAL_REL, err.rel


# ------------------------------------------------------------------------------------------------ production call sites (section 5)
def production_check(hip, q, k, v, wins, Hq, Hkv, D, n_rows, what, repeats=10):
    """The call site's plan (tile_rows by engine.attn_tile_rows) against fp64 row by row, 10 repeated launches bit-identical
    to the first, and - when that plan is not already the 4-wave form - the 4-wave 128-row form on the same inputs."""
    from g2vlm_amd.engine import attn_tile_rows
    tile_rows = attn_tile_rows(wins, Hq)
    ref = ref_fp64(q, k, v, wins, Hq, Hkv, D)
    ldo = Hq * D + 64
    plan = hip.make_attn_plan(wins, Hq, "cuda", tile_rows=tile_rows)
    out = launch(hip, q, k, v, plan, Hq, Hkv, D, wins, n_rows, ldo)
    err = Errors(out, ref, Hq, D)
    check_bounds(err, D, f"{what} tile_rows={tile_rows}")
    first = out.clone()
    flick = sum(int(not same_bits(launch(hip, q, k, v, plan, Hq, Hkv, D, wins, n_rows, ldo), first)) for _ in range(repeats))
    assert flick == 0, (what, flick)
    if tile_rows != 128:
        plan4 = hip.make_attn_plan(wins, Hq, "cuda", tile_rows=128)
        e4 = Errors(launch(hip, q, k, v, plan4, Hq, Hkv, D, wins, n_rows, ldo), ref, Hq, D)
        check_bounds(e4, D, f"{what} 4-wave")
        check_vs_4wave(err, e4, what)
    return tile_rows, plan, first, ref


def packed_qkv(g, rows, C, covered):
    """One [rows, 3C] bf16 qkv buffer as a linear layer writes it; rows outside every window are NaN."""
    qkv = randn(g, rows, 3 * C).bfloat16()
    qkv[~covered] = float("nan")
    return qkv


@pytest.mark.parametrize("cfg,N,P,want_rows", [("C3", 8, 1369, 256), ("C2", 2, 777, 128)])
def test_dino(hip, cfg, N, P, want_rows):
    """DINOv2 windows (engine.dino_layers): packed qkv ld 3 x 1024, 16 heads of 64, N windows of P rows over N (P + 5) rows -
    the last 5N rows are in no window (H1) and must keep their bits."""
    Hq, D = 16, 64
    C, rows = Hq * D, N * (P + 5)
    wins = tuple((i * P, P, i * P, P, False) for i in range(N))
    qkv = packed_qkv(gen(11 + N), rows, C, covered_rows(wins, rows))
    tr, *_ = production_check(hip, qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], wins, Hq, Hq, D, rows, f"DINO {cfg}")
    assert tr == want_rows


@pytest.mark.parametrize("cfg,N,P,want_rows", [("C3", 8, 1369, 256), ("C2", 2, 777, 128)])
@pytest.mark.parametrize("kind", ["self", "cross"])
def test_decoder(hip, kind, cfg, N, P, want_rows):
    """Pi3 decoder blocks (engine.decoder), 16 heads of 96: self-attention on the packed qkv (ld 3 x 1536) per view;
    cross-attention with q [N P, 1536] and K / V = the two halves of ckv [P, 3072], every view's window on the same KV range."""
    Hq, D = 16, 96
    C, M = Hq * D, N * P
    g = gen(21 + N)
    if kind == "self":
        wins = tuple((i * P, P, i * P, P, False) for i in range(N))
        qkv = packed_qkv(g, M, C, covered_rows(wins, M))
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    else:
        wins = tuple((i * P, P, 0, P, False) for i in range(N))
        ckv = randn(g, P, 2 * C).bfloat16()
        q, k, v = randn(g, M, C).bfloat16(), ckv[:, :C], ckv[:, C:]
    tr, *_ = production_check(hip, q, k, v, wins, Hq, Hq, D, M, f"decoder {kind} {cfg}")
    assert tr == want_rows


@pytest.mark.parametrize("n_images", [1, 8])
def test_vit(hip, n_images):
    """Qwen2-VL ViT (engine.vit_forward), 16 heads of 80: packed qkv ld 3 x 1280, one window per 756 x 756 image (2916 rows)."""
    Hq, D, S = 16, 80, 2916
    C, rows = Hq * D, n_images * S
    wins = tuple((i * S, S, i * S, S, False) for i in range(n_images))
    qkv = packed_qkv(gen(31 + n_images), rows, C, covered_rows(wins, rows))
    tr, *_ = production_check(hip, qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], wins, Hq, Hq, D, rows, f"ViT x{n_images}")
    assert tr == 256


def kv_cache(g, tot, Hkv=2, D=128, spare=300):
    """A KVCache layer as llm_forward reads it: [capacity, Hkv, 128] viewed [tot, Hkv*128]; rows >= tot are NaN."""
    kc = torch.full((tot + spare, Hkv, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    vc = torch.full_like(kc, float("nan"))
    kc[:tot] = randn(g, tot, Hkv, D).bfloat16()
    vc[:tot] = randn(g, tot, Hkv, D).bfloat16()
    return kc[:tot].view(tot, Hkv * D), vc[:tot].view(tot, Hkv * D)


S_VIT = 731


@pytest.mark.parametrize("case", ["C3", "C2", "text_after_prefix", "vit_staircase"])
def test_mot(hip, case):
    """MoT LLM attention (engine.llm_forward), 12:2 heads of 128: q [L, 1536], K / V views [tot, 256] of the cache.
    C3 / C2 geo prefill (non-causal), a causal text prompt after a KV prefix, and the multi-image ViT prefill's staircase
    windows (j S, S, 0, kv_len + (j + 1) S) with S = 731 and 8 images (G2VLM.forward_cache_update_vit_multi)."""
    Hq, Hkv, D = 12, 2, 128
    g = gen(41)
    if case == "C3":
        L, kv_len, want = 10968, 8, 256
        wins = ((0, L, 0, kv_len + L, False),)
    elif case == "C2":
        L, kv_len, want = 1558, 8, 128
        wins = ((0, L, 0, kv_len + L, False),)
    elif case == "text_after_prefix":
        L, kv_len, want = 40, 10976, 128
        wins = ((0, L, 0, kv_len + L, True),)
    else:
        L, kv_len, want = 8 * S_VIT, 11000, 128
        wins = tuple((j * S_VIT, S_VIT, 0, kv_len + (j + 1) * S_VIT, False) for j in range(8))
    k, v = kv_cache(g, kv_len + L)
    q = randn(g, L, Hq * D).bfloat16()
    tr, *_ = production_check(hip, q, k, v, wins, Hq, Hkv, D, L, f"MoT {case}")
    assert tr == want


@pytest.mark.parametrize("rank", ["first", "middle", "last"])
def test_c4_rank_phases(hip, rank):
    """View-sharded C4 prefill (llm_forward with kv_exchange): a rank's 5484 query rows against 43 880 cache rows in two
    launches - phase 0 = its own K/V block, phase 1 = the prefix and the other ranks' blocks - merged after the last one.
    A rank whose block starts at row 0 (phase 1 = the rows after it only), a middle rank, the last rank (block ends at tot).
    Run as one call (phase=None) and phase by phase as llm_forward does: bit-identical, and both against fp64."""
    Hq, Hkv, D, L, tot = 12, 2, 128, 5484, 43880
    r0 = {"first": 0, "middle": 8 + 3 * L, "last": tot - L}[rank]
    wins = [(0, L, r0, L, False, 0)]
    if r0 > 0:
        wins.append((0, L, 0, r0, False, 1))
    if r0 + L < tot:
        wins.append((0, L, r0 + L, tot - r0 - L, False, 1))
    wins = tuple(wins)
    g = gen(51)
    k, v = kv_cache(g, tot)
    q = randn(g, L, Hq * D).bfloat16()
    tr, plan, whole, ref = production_check(hip, q, k, v, wins, Hq, Hkv, D, L, f"C4 rank {rank}")
    assert tr == 256 and len(plan.phases) == 2
    stepped = launch(hip, q, k, v, plan, Hq, Hkv, D, wins, L, Hq * D + 64, phase_by_phase=True)
    assert same_bits(stepped, whole)
    check_bounds(Errors(stepped, ref, Hq, D), D, f"C4 rank {rank} phase by phase")
