"""GPU: g2v_logprob_rows_bf16 (csrc/logprob.hip) against fp64 on the same bf16 inputs.

Bound on out_lp and out_lse: |got - want| <= 1e-4 + 2^-22 |x_t - max|.  A tree-summed fp32 sum of at most 2^18 terms carries
about 18 x 2^-24 relative error, v_exp_f32 on an argument of magnitude up to 128 at most about 128 x 2^-23 in a term: together
under 2e-5 in the logarithm; the second term is the rounding of the subtraction x_t - max.  `want` is the fp64 value rounded
to fp32, the format the kernel writes: at ordinary magnitudes that moves it by less than 4e-6, and it is what makes the rows at
+- bf16 max checkable at all (their logsumexp, 3.39e38 + log(count), and a log-probability of -6.78e38 are not fp32 numbers;
where the rounded value is infinite the kernel must return exactly it).  out_rank must be exact.
Largest observed errors: DESIGN 6g."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BF16_MAX = 3.3895313892515355e38
VOCAB = 151936
KINDS = ("gauss1", "gauss8", "equal", "spike", "neg_inf", "neg_inf_target", "pos_max", "neg_max", "both_max", "ties", "first", "last",
         "below", "above", "all_neg_inf")


@pytest.fixture(scope="module")
def hip():
    from g2vlm_amd import hip
    hip.lib()
    return hip


def make_row(kind, n, g):
    """(values fp32 [n] that are exactly bf16, target) of one row of kind `kind`."""
    x = torch.randn(n, generator=g)
    t = int(torch.randint(0, n, (1,), generator=g))
    if kind == "gauss8":
        x *= 8
    elif kind == "equal":                                   # expected -log n
        x[:] = 1.25
    elif kind == "spike":                                   # +30 at the target and at one other place
        x[t] = 30.0
        x[(t + n // 2) % n] = 30.0
    elif kind == "neg_inf":
        x[torch.rand(n, generator=g) < 0.3] = -math.inf
        x[t] = 0.5
    elif kind == "neg_inf_target":
        x[torch.rand(n, generator=g) < 0.3] = -math.inf
        x[t] = -math.inf
        x[(t + 1) % n] = 0.25                                # n == 1: the only entry, finite (the row is then not all -inf)
    elif kind == "pos_max":                                 # one entry at +max, the target
        x[t] = BF16_MAX
    elif kind == "neg_max":                                 # everything at -max: -log n, lse = -max
        x[:] = -BF16_MAX
    elif kind == "both_max":                                # +max somewhere, the target at -max: x_t - max is not an fp32 number
        x[:] = -BF16_MAX
        x[(t + 1) % n] = BF16_MAX
        x[(t + 2) % n] = BF16_MAX
    elif kind == "ties":                                    # the target's value again before and after it, and above it once
        x = (x * 4).round() / 4
        t = n // 2
        x[t] = 0.75
        for i in (0, t - 1, t + 1, n - 1):
            x[i % n] = 0.75
        x[n // 3] = 2.0 if n // 3 != t else x[n // 3]
    elif kind == "all_neg_inf":                             # nothing finite: logsumexp -inf, and the -inf target gives -inf as in any row
        x[:] = -math.inf
    elif kind == "first":
        t = 0
    elif kind == "last":
        t = n - 1
    elif kind == "below":
        t = -1
    elif kind == "above":
        t = n + 3
    return x.to(torch.bfloat16).float(), t


def make_case(kinds, n, ld, seed):
    """bf16 [rows, n] view of a [rows, ld] matrix whose pad columns are NaN, int32 targets, both on the device."""
    g = torch.Generator(); g.manual_seed(seed)
    rows = [make_row(k, n, g) for k in kinds]
    full = torch.full((len(kinds), ld), math.nan, dtype=torch.bfloat16)
    full[:, :n] = torch.stack([r[0] for r in rows]).to(torch.bfloat16)
    return full.cuda()[:, :n], torch.tensor([r[1] for r in rows], dtype=torch.int32).cuda()


def reference(x, t):
    """fp64 on the device: (log-probability, logsumexp, rank, x_t - max) per row; NaN / -1 where the target is out of range."""
    n = x.shape[1]
    xd = x.double()
    ok = (t >= 0) & (t < n)
    tc = t.clamp(0, n - 1).long()
    xt = xd.gather(1, tc[:, None])[:, 0]
    mx = xd.max(dim=1).values
    mx0 = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    log_sum = (xd - mx0[:, None]).exp().sum(dim=1).log()   # x_t - lse as (x_t - max) - log_sum: at 3.4e38 fp64 itself has an ulp of 3.8e22
    lse = mx + log_sum
    lp = (xt - mx0) - log_sum
    lp = torch.where(torch.isinf(mx), mx, lp)               # a row of -inf only: -inf by the entry point's definition (torch: NaN)
    idx = torch.arange(n, device=x.device)[None, :]
    rank = ((xd > xt[:, None]) | ((xd == xt[:, None]) & (idx < tc[:, None]))).sum(dim=1)
    nan = torch.full_like(lp, math.nan)
    return torch.where(ok, lp, nan), lse, torch.where(ok, rank, torch.full_like(rank, -1)).int(), torch.where(ok, xt - mx, nan)


def check(hip, x, t, what):
    """One launch with all three outputs against the reference; returns the largest finite errors (lp, lse)."""
    rows = x.shape[0]
    lse = torch.full((rows,), 7.0, dtype=torch.float32, device="cuda")
    rank = torch.full((rows,), 77, dtype=torch.int32, device="cuda")
    lp = hip.logprob_rows_bf16(x, t, lse=lse, rank=rank)
    want_lp, want_lse, want_rank, gap = reference(x, t)
    assert torch.equal(rank, want_rank), (what, rank.tolist(), want_rank.tolist())
    worst = []
    for name, got, want, tol_gap in (("lp", lp, want_lp, gap), ("lse", lse, want_lse, gap.nan_to_num(0.0))):
        w32 = want.float()                                    # the fp64 value in the kernel's output format
        bad_target = torch.isnan(want)
        assert torch.equal(torch.isnan(got), bad_target), (what, name, got.tolist())
        inf = torch.isinf(w32)
        assert torch.equal(got[inf], w32[inf]), (what, name, got[inf].tolist(), w32[inf].tolist())
        fin = ~inf & ~bad_target
        err = (got[fin].double() - w32[fin].double()).abs()
        bound = 1e-4 + 2.0 ** -22 * tol_gap[fin].abs()
        worst.append(float((err).max()) if err.numel() else 0.0)
        assert bool((err <= bound).all()), (what, name, float(err.max()), got[fin].tolist()[:8], w32[fin].tolist()[:8])
    return worst


SHAPES = [(rows, n) for rows in (1, 3, 64, 65) for n in (1, 7, 2048, 2049)] + [(1, VOCAB), (3, VOCAB)]


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("rows,n", SHAPES)
def test_shapes_against_fp64(hip, rows, n, pad):
    """Every row count x row length, ld = n and ld = n + 5 (odd: the rows' bases are 2-byte aligned only) with NaN in the pad;
    the rows cycle through every input kind."""
    kinds = [KINDS[(r + n + rows) % len(KINDS)] for r in range(rows)]
    x, t = make_case(kinds, n, n + pad, seed=1000 * rows + n + pad)
    e_lp, e_lse = check(hip, x, t, (rows, n, pad))
    print(f"[logprob] rows {rows} n {n} ld {n + pad}: max |lp err| {e_lp:.3e}, max |lse err| {e_lse:.3e}")


@pytest.mark.parametrize("n", [1, 7, 2048, 2049, VOCAB])
def test_every_input_kind_at_every_length(hip, n):
    """Gaussian sigma 1 and 8, all-equal (-log n), two +30 spikes, -inf entries, a -inf target, rows at +- bf16 max, exact ties
    before / at / after the target, targets at 0, n - 1 and out of range: three rows per launch (the out-of-range rows sit
    between valid ones, whose results must not move)."""
    order = ("gauss1", "below", "gauss8", "equal", "above", "spike", "neg_inf", "neg_inf_target", "pos_max", "neg_max", "both_max", "ties",
             "first", "last", "all_neg_inf")
    worst = [0.0, 0.0]
    for i in range(0, len(order), 3):
        x, t = make_case(order[i:i + 3], n, n + 5, seed=n + i)
        e = check(hip, x, t, (n, order[i:i + 3]))
        worst = [max(a, b) for a, b in zip(worst, e)]
    x, t = make_case(("equal",), n, n, seed=3)
    lp = hip.logprob_rows_bf16(x, t)
    assert abs(float(lp[0]) + math.log(n)) <= 1e-4
    print(f"[logprob] n {n}, every kind: max |lp err| {worst[0]:.3e}, max |lse err| {worst[1]:.3e}")


@pytest.mark.parametrize("rows", [64, 65])
@pytest.mark.parametrize("n", [20000, 24577])
def test_many_rows_split_over_workgroups_against_fp64(hip, rows, n):
    """3 and 4 chunks per row with 64 / 65 rows: every row dealt out to several workgroups, ticket and merge included, against
    fp64 (the shapes above split a row only at the real vocabulary, with 1 and 3 rows)."""
    assert hip.logprob_rows_workspace(rows, n) > 0
    kinds = [KINDS[(r + rows) % len(KINDS)] for r in range(rows)]
    x, t = make_case(kinds, n, n + 5, seed=rows + n)
    e_lp, e_lse = check(hip, x, t, (rows, n))
    print(f"[logprob] rows {rows} n {n} split: max |lp err| {e_lp:.3e}, max |lse err| {e_lse:.3e}")


def test_a_rows_result_depends_on_nothing_but_the_row(hip):
    """Row 0 alone, inside 65 rows, inside 200 and 600 rows (other splits of a row over workgroups, and none), as row 1 of a
    matrix with odd ld (2-byte aligned base) and without the optional outputs: bit for bit the same three results."""
    for n in (40000, VOCAB):
        g = torch.Generator(); g.manual_seed(n)
        big = (torch.randn((600 if n == 40000 else 65, n), generator=g) * 8).to(torch.bfloat16).cuda()
        tg = torch.randint(0, n, (big.shape[0],), generator=g).int().cuda()

        def run(x, t, full=True):
            lse = torch.empty(x.shape[0], dtype=torch.float32, device="cuda") if full else None
            rank = torch.empty(x.shape[0], dtype=torch.int32, device="cuda") if full else None
            lp = hip.logprob_rows_bf16(x, t, lse=lse, rank=rank)
            return lp, lse, rank
        alone = run(big[:1], tg[:1])
        for rows in (65, 200, 600):
            if rows > big.shape[0]:
                continue
            many = run(big[:rows], tg[:rows])
            for a, b in zip(alone, many):
                assert torch.equal(a[0], b[0]), (n, rows)
        assert torch.equal(run(big[:1], tg[:1], full=False)[0], alone[0])        # NULL out_lse / out_rank
        odd = torch.full((2, n + 5), math.nan, dtype=torch.bfloat16, device="cuda")
        odd[1, :n] = big[0]
        assert odd[1].data_ptr() % 4 == 2
        moved = run(odd[:, :n][1:], tg[:1])
        for a, b in zip(alone, moved):
            assert torch.equal(a, b), n
        # the later rows too: row r of the 65 against row r alone
        many = run(big[:65], tg[:65])
        for r in (1, 31, 64):
            one = run(big[r:r + 1], tg[r:r + 1])
            for a, b in zip(one, many):
                assert torch.equal(a[0], b[r]), (n, r)


def test_graph_replays_equal_eager_launches(hip):
    """Three replays of a captured launch (new logits and targets copied in before each) against three eager launches."""
    rows, n = 3, VOCAB
    g = torch.Generator(); g.manual_seed(5)
    data = [((torch.randn((rows, n), generator=g) * 4).to(torch.bfloat16).cuda(), torch.randint(0, n, (rows,), generator=g).int().cuda())
            for _ in range(3)]
    scratch = torch.zeros(hip.logprob_rows_workspace(rows, n) // 4, dtype=torch.int32, device="cuda")
    assert scratch.numel() > 0
    x, t = torch.empty_like(data[0][0]), torch.empty_like(data[0][1])
    lp, lse = (torch.empty(rows, dtype=torch.float32, device="cuda") for _ in range(2))
    rank = torch.empty(rows, dtype=torch.int32, device="cuda")
    eager = []
    for xd, td in data:
        x.copy_(xd); t.copy_(td)
        hip.logprob_rows_bf16(x, t, lse=lse, rank=rank, out=lp, scratch=scratch)
        eager.append((lp.clone(), lse.clone(), rank.clone()))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            hip.logprob_rows_bf16(x, t, lse=lse, rank=rank, out=lp, scratch=scratch)
    torch.cuda.current_stream().wait_stream(s)
    for (xd, td), want in zip(data, eager):
        x.copy_(xd); t.copy_(td)
        lp.zero_(); lse.zero_(); rank.zero_()
        graph.replay()
        for a, b in zip((lp, lse, rank), want):
            assert torch.equal(a, b)
    assert not bool(scratch[:512].any())                       # the tickets are back at zero
