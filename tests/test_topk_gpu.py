"""GPU: g2v_topk_rows_bf16 (csrc/topk.hip) against an exact reference.

The order is g2v_argmax_rows_bf16's: larger value first, -0 == +0, every NaN above +inf, equal keys by ascending index.  The
reference restates misc.hip's argmax_key on the device and sorts the integer keys stably, descending; no two elements of a
row are equal in that order, so indices and the bit patterns of the values must match exactly - there is no tolerance.
Entries j >= n (k > n) are index -1 and the value NaN (0x7fc00000)."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BF16_MAX = 3.3895313892515355e38
VOCAB = 151936
CHUNK = 8192                                                 # elements of a row one workgroup takes at a time (TK_CHUNK)
SPLIT_ROWS = 512                                             # from this many rows on a row is never dealt out to several workgroups
KS = (1, 2, 5, 31, 32)
ROWS = (1, 3, 64, 65, SPLIT_ROWS - 1, SPLIT_ROWS)
NS = (1, 7, 31, 32, 33, 64, 2048, 2049, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1, VOCAB)
KINDS = ("gauss1", "gauss8", "equal", "quant", "planted", "one_lane", "per_chunk", "zeros", "neg_inf", "all_neg_inf", "pos_inf", "nans",
         "pm_max")
# a lane owns 8 consecutive elements in each of 4 vectors 2048 apart (lane 0: 0 .. 7, .., 6144 .. 6151), a wave 512 consecutive ones
# in each of them (wave 0: 0 .. 511, .., 6144 .. 6655), a chunk 8192: the last element of each share and the first of the next
EDGES = (0, 7, 8, 511, 512, 2047, 2048, 6151, 6152, 6655, 6656, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK)


@pytest.fixture(scope="module")
def hip():
    from g2vlm_amd import hip
    hip.lib()
    return hip


def fill_row(kind, x, g):
    """Row `x` (fp32 [n] on the device, Gaussian on entry) made a row of kind `kind`, in place."""
    n = x.numel()
    at = lambda idx: torch.tensor([i for i in idx if 0 <= i < n], dtype=torch.long, device=x.device)   # noqa: E731
    rnd = lambda: torch.rand(n, generator=g, device=x.device)                                          # noqa: E731
    if kind == "gauss8":
        x *= 8
    elif kind == "equal":                                    # expected: indices 0 .. k-1
        x.fill_(1.25)
    elif kind == "quant":                                    # ties across lanes, waves and chunks
        x.copy_((x * 4).round() / 4)
    elif kind == "planted":                                  # winners at the edges of a lane's, a wave's and a chunk's share
        idx = at(EDGES + (n - 1,)).unique()
        x[idx] = 50.0 + torch.arange(idx.numel(), device=x.device).float().flip(0) % 5    # some of them tie
    elif kind == "one_lane":                                 # all 32 elements of lane 37 of the first chunk: every winner in one lane
        idx = at([2048 * u + 37 * 8 + e for u in range(4) for e in range(8)])
        if idx.numel():
            x[idx] = 60.0 + torch.randperm(idx.numel(), generator=g, device=x.device).float()
    elif kind == "per_chunk":                                # one winner per chunk, descending from the last chunk to the first
        idx = at([c * CHUNK + (977 * c) % CHUNK for c in range((n + CHUNK - 1) // CHUNK)])
        x[idx] = 40.0 + torch.arange(idx.numel(), device=x.device).float()
    elif kind == "zeros":                                    # +0 and -0 are one key: ascending index among them
        x.copy_(torch.where(rnd() < 0.5, torch.zeros_like(x), -torch.zeros_like(x)))
        x[rnd() < 0.3] = -1.0
    elif kind == "neg_inf":
        x[rnd() < 0.3] = -math.inf
    elif kind == "all_neg_inf":
        x.fill_(-math.inf)
    elif kind == "pos_inf":
        x[at([n - 1, n // 2, 5])] = math.inf
    elif kind == "nans":                                     # several NaN: they come first, in index order
        x[at([n - 1, n // 3, 9, CHUNK + 1])] = math.nan
        x[at([n // 2])] = math.inf
    elif kind == "pm_max":
        x[at([3, n - 2, CHUNK])] = BF16_MAX
        x[at([4, n - 3])] = -BF16_MAX
    return x


def make_case(rows, n, ld, seed):
    """bf16 [rows, n] view of a [rows, ld] matrix whose pad columns are NaN; the rows cycle through every kind."""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    x = torch.randn((rows, n), generator=g, device="cuda")
    for r in range(rows):
        fill_row(KINDS[(r + n) % len(KINDS)], x[r], g)
    full = torch.full((rows, ld), math.nan, dtype=torch.bfloat16, device="cuda")
    full[:, :n] = x.to(torch.bfloat16)
    return full[:, :n]


def keys(x):
    """misc.hip's argmax_key of every element, int32."""
    f = x.float()
    b = f.view(torch.int32)
    k = torch.where(b >= 0, b, b ^ 0x7fffffff)
    k = torch.where(f == 0, torch.zeros_like(k), k)
    return torch.where(f != f, torch.full_like(k, 0x7fffffff), k)


def reference(x, k):
    """(indices int32 [rows, k], value bits int32 [rows, k]): a stable descending sort of the keys."""
    rows, n = x.shape
    order = torch.sort(keys(x), dim=1, descending=True, stable=True).indices[:, :k]
    idx = torch.full((rows, k), -1, dtype=torch.int32, device=x.device)
    bits = torch.full((rows, k), 0x7fc00000, dtype=torch.int32, device=x.device)
    idx[:, :order.shape[1]] = order.int()
    bits[:, :order.shape[1]] = x.float().gather(1, order).view(torch.int32)
    return idx, bits


def launch(hip, x, k, scratch=None, with_val=True):
    """One launch into the middle of guarded buffers: (idx, value bits); the guard rows around both outputs must stay."""
    rows = x.shape[0]
    gi = torch.full((rows + 2, k), 77, dtype=torch.int32, device="cuda")
    gv = torch.full((rows + 2, k), 7.0, dtype=torch.float32, device="cuda")
    idx, val = hip.topk_rows_bf16(x, k, out_idx=gi[1:rows + 1], out_val=gv[1:rows + 1], scratch=scratch)
    assert bool((gi[0] == 77).all()) and bool((gi[-1] == 77).all()) and bool((gv[0] == 7.0).all()) and bool((gv[-1] == 7.0).all())
    assert idx.data_ptr() == gi[1].data_ptr() and val.data_ptr() == gv[1].data_ptr()
    return idx.clone(), val.view(torch.int32).clone()


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("n", NS)
def test_every_shape_against_the_exact_reference(hip, n, pad):
    """Every row count x k at one row length, ld = n and ld = n + 5 (odd: the rows' bases are 2-byte aligned only) with NaN in
    the pad.  One matrix and one reference sort per case; the first `rows` rows of it are launched for every row count."""
    x = make_case(max(ROWS), n, n + pad, seed=7 * n + pad)
    want_idx, want_bits = reference(x, max(KS))
    nan_free = ~torch.isnan(x.float()).any(dim=1)
    for rows in ROWS:
        assert (hip.topk_rows_workspace(rows, n, 5) > 0) == (rows < SPLIT_ROWS and n > CHUNK)
        for k in KS:
            idx, bits = launch(hip, x[:rows], k)
            assert bool(((idx >= -1) & (idx < n)).all())
            assert torch.equal(idx, want_idx[:rows, :k]), (rows, n, k, (idx != want_idx[:rows, :k]).nonzero()[:4].tolist())
            assert torch.equal(bits, want_bits[:rows, :k]), (rows, n, k)
        if rows in (3, 65):
            # column 0 is the argmax kernel's pick on every row, NaN rows included
            am = hip.argmax_rows_bf16(x[:rows], torch.empty(rows, dtype=torch.int32, device="cuda"),
                                      torch.zeros(rows * 129, dtype=torch.int32, device="cuda"))
            assert torch.equal(am, idx[:, 0])
            # on NaN-free rows, entry j is the one token whose rank g2v_logprob_rows_bf16 reports as j
            for j in sorted({0, min(1, n - 1), min(n, max(KS)) - 1}):
                rank = torch.empty(rows, dtype=torch.int32, device="cuda")
                hip.logprob_rows_bf16(x[:rows], idx[:, j].contiguous(), rank=rank)
                assert bool((rank[nan_free[:rows]] == j).all()), (rows, n, j)


def test_equal_rows_give_the_first_indices_and_nans_come_first(hip):
    n = 3 * CHUNK + 1
    x = torch.full((2, n), 1.25, dtype=torch.bfloat16, device="cuda")
    x[1, [n - 1, 9, CHUNK + 1]] = math.nan
    x[1, 4] = math.inf
    idx, bits = launch(hip, x, 5)
    assert idx[0].tolist() == [0, 1, 2, 3, 4]
    assert idx[1].tolist() == [9, CHUNK + 1, n - 1, 4, 0]
    assert bits[1].tolist() == [0x7fc00000] * 3 + [0x7f800000, 0x3fa00000]
    z = torch.tensor([[-1.0, -0.0, 0.0, -0.0, 0.0]], dtype=torch.bfloat16, device="cuda")
    idx, bits = launch(hip, z, 4)
    assert idx[0].tolist() == [1, 2, 3, 4] and [b & 0xffffffff for b in bits[0].tolist()] == [0x80000000, 0, 0x80000000, 0]
    idx, bits = launch(hip, z[:, :2], 4)                      # k > n: -1 / NaN behind the row's two entries
    assert idx[0].tolist() == [1, 0, -1, -1] and bits[0, 2:].tolist() == [0x7fc00000] * 2


def test_a_rows_result_depends_on_nothing_but_the_row(hip):
    """Row 0 alone, inside 65 and 600 rows (other splits of a row over workgroups, and none), as row 1 of a matrix with odd ld
    (2-byte aligned base), with a scratch too small to split and without out_val: the same bits."""
    for n, many in ((40000, 600), (VOCAB, 65)):
        g = torch.Generator(device="cuda"); g.manual_seed(n)
        big = ((torch.randn((many, n), generator=g, device="cuda") * 4).round() / 4).to(torch.bfloat16)     # plenty of ties
        for k in (5, 32):
            alone = launch(hip, big[:1], k)
            for rows in (65, many):
                got = launch(hip, big[:rows], k)
                assert torch.equal(got[0][0], alone[0][0]) and torch.equal(got[1][0], alone[1][0]), (n, rows, k)
            assert hip.topk_rows_workspace(1, n, k) > 4
            none = launch(hip, big[:1], k, scratch=torch.zeros(1, dtype=torch.int32, device="cuda"))   # too few bytes: no split
            assert torch.equal(none[0], alone[0]) and torch.equal(none[1], alone[1])
            own = torch.zeros(hip.topk_rows_workspace(1, n, k) // 4, dtype=torch.int32, device="cuda")
            mine = launch(hip, big[:1], k, scratch=own)
            assert torch.equal(mine[0], alone[0]) and torch.equal(mine[1], alone[1]) and not bool(own[:SPLIT_ROWS].any())
            odd = torch.full((2, n + 5), math.nan, dtype=torch.bfloat16, device="cuda")
            odd[1, :n] = big[0]
            assert odd[1].data_ptr() % 4 == 2
            moved = launch(hip, odd[:, :n][1:], k)
            assert torch.equal(moved[0], alone[0]) and torch.equal(moved[1], alone[1])
            r = many - 1                                      # a later row too
            one, got = launch(hip, big[r:r + 1], k), launch(hip, big, k)
            assert torch.equal(got[0][r], one[0][0]) and torch.equal(got[1][r], one[1][0])


def test_graph_replays_equal_eager_launches(hip):
    """Three replays of a captured launch (new logits copied in before each) against three eager launches."""
    rows, n, k = 3, VOCAB, 5
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    data = [(torch.randn((rows, n), generator=g, device="cuda") * 4).to(torch.bfloat16) for _ in range(3)]
    scratch = torch.zeros(hip.topk_rows_workspace(rows, n, k) // 4, dtype=torch.int32, device="cuda")
    assert scratch.numel() > SPLIT_ROWS
    x = torch.empty_like(data[0])
    idx = torch.empty((rows, k), dtype=torch.int32, device="cuda")
    val = torch.empty((rows, k), dtype=torch.float32, device="cuda")
    eager = []
    for xd in data:
        x.copy_(xd)
        hip.topk_rows_bf16(x, k, out_idx=idx, out_val=val, scratch=scratch)
        eager.append((idx.clone(), val.clone()))
        want = reference(x, k)
        assert torch.equal(idx, want[0]) and torch.equal(val.view(torch.int32), want[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            hip.topk_rows_bf16(x, k, out_idx=idx, out_val=val, scratch=scratch)
    torch.cuda.current_stream().wait_stream(s)
    for xd, want in zip(data, eager):
        x.copy_(xd)
        idx.zero_(); val.zero_()
        graph.replay()
        assert torch.equal(idx, want[0]) and torch.equal(val, want[1])
    assert not bool(scratch[:SPLIT_ROWS].any())                # the tickets are back at zero
