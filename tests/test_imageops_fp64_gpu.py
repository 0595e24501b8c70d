"""GPU: the token pickers, the camera tail, the point head tail, the DINO front end (csrc/misc.hip) and swiglu_bf16
(csrc/decode.hip), element by element against the fp64 references and exact restatements of tests/imageop_check.py (the rule
behind each bound is in its docstring).

A case passes with zero flagged elements.  Outputs live in caller-allocated buffers prefilled with sentinels (bf16 0x7FA5,
fp32 0x7FA5A5A5, int32 -1) with guard rows that must keep them; where the Python wrapper allocates the output itself the C
entry point is called directly.  Every call runs twice and the two results must be bit-identical.

Kernel paths reached.
  argmax: the 1-workgroup form at n = 1 .. 65535 (a lone element, one partial wave, the wave boundary 63|64, the 256-thread
  stride 255|256, 256 strides at 65535) and the 64-workgroup form at n = 65536, 65537, 151936 (winners on both sides of
  workgroup boundaries 1, 32 and 63, a last workgroup of 962 elements at 65537), through g2v_argmax_bf16 and through
  g2v_argmax_rows_bf16 with rows = 1, 5, 64 and ld = n + 8; the sampler on both forms at 65535 | 65536 | 65537, eager and
  replayed from a captured graph.
  camera tail: P = 1, 2, 3 (the tail loop alone), 4, 8 (the unrolled body alone), 5, 7, 37 (both); both SVD branches (four
  views with det < 0, four with det > 0, and the exact-input reflection); every Jacobi rotation skipped at M = I.
  point head: both patch sizes (14, 16), one exact block (16 x 16, N = 1) and partial last blocks, square and both
  non-square orientations, modes 0 and 1, pixel_shuffle with C = 1, 2, 3.
  im2col14 / dino_assemble: one patch up to 36 patches per view, Kpad 592 and 640; C = 4 .. 1024.
  swiglu_bf16: n = 16 (one partial block), 512 (two blocks), 1000 (a partial last block and a partial group of 16), 8960.

Measured on an MI355X (the module's teardown prints them as STATS lines, visible with -s):
  camera B1 largest |got - ref| / e: 0.0191 (t), 0.0314 (m9); the check flags at 2; on the rotation views' mixed-sign
  layers 2.9e-05 (t), 3.83e-05 (m9)
  rotation largest error / bound: 0.0308 (8 random views, smallest gap 0.457), 0.0258 (exact inputs);
  |R^T R - I| 0.933 u, |det R - 1| 0.8 u (both asserted <= 8 u)
  pts mode 1 largest error / bound: z 0.163, lx / ly 0.223, world 0.257
  swiglu share of elements with two admissible inner values: 0.2 % (n = 1000), 0.167 % (n = 8960), 0 at 16 and 512
  sampler on the sparse row: 4 of the 5 live indices drawn in 24 draws, none outside them
Before argmax_bf16_kernel merged ordered keys with NaN on top, exactly the rows with +inf below a NaN failed here (at every
n >= 2, in one wave, across waves, in one thread and across workgroups) and nothing else in section A.  Before
siluf_ (common.h) took its x < -87 tail through x exp(x + 44) exp(-44), the element with g = -88 was flagged at every n (the
fast form's reciprocal is flushed to zero there) and nothing else; swiglu_bf16_kernel and the decode kernels' fused SwiGLU
share siluf_ (the GEMM tile epilogues keep the fast form under gemm_check.py's absolute floor).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imageop_check as I  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
GUARD = 0x5A5A5A5A
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


def dev(t):
    return t.cuda()


def twice(run):
    """run() -> tuple of tensors: both launches' results must be bit-identical."""
    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(I.bits(x) if x.is_floating_point() else x, I.bits(y) if y.is_floating_point() else y), "two launches differ"
    return a


# ------------------------------------------------------------------------------------------ A. token pickers
def scratch_for(rows, guard=2):
    """int32 [(rows + guard) 129]: the rows' slabs zeroed (once), the guard slabs filled with a pattern they must keep."""
    s = torch.full(((rows + guard) * 129,), GUARD, dtype=I32, device="cuda")
    s[:rows * 129] = 0
    return s


def assert_scratch(s, rows, what):
    s = s.cpu().view(-1, 129)
    assert s[:rows, 0].tolist() == [0] * rows, f"{what}: a ticket word is not back at 0"
    assert bool((s[rows:] == GUARD).all()), f"{what}: a slab of a row that was not launched changed"


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 65535, 65536, 65537, 151936])
def test_argmax_every_placement(hip, n):
    cases = I.argmax_cases(n)
    names = [c[0] for c in cases]
    x = I.argmax_matrix(cases, n)
    m, ld = x.shape
    want = I.argmax_ref(x[:, :n])
    M = max(m, 64)
    sel = torch.arange(M) % m
    xd = dev(x[sel].contiguous())                                   # [M, ld]: the cases, repeated up to 64 rows
    wantM = want[sel]
    lib = hip.lib()

    def report(got, wnt, form):
        bad = (got != wnt).nonzero().flatten().tolist()
        return f"n={n} {form}: " + "; ".join(f"'{names[int(sel[r])]}' gave {int(got[r])}, want {int(wnt[r])}" for r in bad[:40])

    def single():
        out = torch.full((m + 2,), -1, dtype=I32, device="cuda")
        scr = scratch_for(1)
        for r in range(m):
            hip._ck(lib.g2v_argmax_bf16(hip._p(xd[r]), n, hip._p(out[r:]), hip._p(scr), hip._stream()), "g2v_argmax_bf16")
        return out, scr
    out, scr = twice(single)
    assert_scratch(scr, 1, "single")
    o = out.cpu()
    assert o[m:].tolist() == [-1, -1]
    assert torch.equal(o[:m].long(), want), report(o[:m].long(), want, "g2v_argmax_bf16")

    for rows in (1, 5, 64):
        starts = sorted({min(g * rows, M - rows) for g in range(-(-m // rows))})

        def batched():
            outs = torch.full((len(starts), rows + 2), -1, dtype=I32, device="cuda")
            scr = scratch_for(rows)                                  # zeroed once, reused by every group
            for g, r0 in enumerate(starts):
                hip._ck(lib.g2v_argmax_rows_bf16(hip._p(xd[r0]), rows, n, ld, hip._p(outs[g]), hip._p(scr), hip._stream()),
                        "g2v_argmax_rows_bf16")
            return outs, scr
        outs, scr = twice(batched)
        assert_scratch(scr, rows, f"rows={rows}")
        o = outs.cpu()
        assert bool((o[:, rows:] == -1).all()), f"rows={rows}: an out slot past the launched rows changed"
        for g, r0 in enumerate(starts):
            w = wantM[r0:r0 + rows]
            assert torch.equal(o[g, :rows].long(), w), report(torch.cat([wantM[:r0], o[g, :rows].long(), wantM[r0 + rows:]]), wantM,
                                                              f"g2v_argmax_rows_bf16 rows={rows}")


@pytest.mark.parametrize("n", [65535, 65536])
@pytest.mark.parametrize("rows", [1, 5, 64])
def test_argmax_scratch_protocol(hip, n, rows):
    """The slabs are zeroed once; three calls follow without re-zeroing.  After each, every launched row's ticket word is 0
    again, and the rows not launched keep their slab and their out slot."""
    x = (I.rnd(rows + 2, n + 8, seed=n + rows) * 3).bfloat16()
    x[:, n:] = float("inf")
    x[rows:] = float("nan")
    want = I.argmax_ref(x[:rows, :n])
    xd = dev(x)
    out = torch.full((rows + 2,), -1, dtype=I32, device="cuda")
    scr = scratch_for(rows)
    for call in range(3):
        out[:rows] = -1
        hip.argmax_rows_bf16(xd[:rows, :n], out, scr)
        assert_scratch(scr, rows, f"call {call}")
        o = out.cpu()
        assert o[rows:].tolist() == [-1, -1] and torch.equal(o[:rows].long(), want), (call, o.tolist())


def sample_ok(x_row, inv_t, seed, step, row, got):
    sc = I.gumbel_scores(x_row, inv_t, seed, step, row)
    return sc[got] >= sc.max() - 1e-4 * max(1.0, abs(sc.max()))


@pytest.mark.parametrize("n", [65535, 65536, 65537])
def test_sample_rows_across_the_workgroup_switch(hip, n):
    rows, seed, T = 3, 0x1234567890ABCDEF, 0.7
    x = torch.full((rows, n + 8), float("nan"))
    x[:, :n] = I.rnd(rows, n, seed=n) * 3
    x = x.bfloat16()
    xd = dev(x)
    xf = x[:, :n].float().numpy()
    inv_t = float(np.float32(1.0 / T))

    def run():
        out = torch.full((rows + 2,), -1, dtype=I32, device="cuda")
        scr = scratch_for(rows)
        rng = hip.make_rng(seed, T, "cuda")
        rng0 = rng.cpu().clone()
        outs = []
        for step in range(2):
            hip.sample_rows_bf16(xd[:, :n], out, scr, rng)
            outs.append(out.clone())
            r = rng.cpu()
            assert r[[0, 1, 3]].tolist() == rng0[[0, 1, 3]].tolist() and int(r[2]) == step + 1
        assert_scratch(scr, rows, "sample")
        return tuple(outs)
    outs = twice(run)
    for step, o in enumerate(outs):
        o = o.cpu().tolist()
        assert o[rows:] == [-1, -1]
        for r in range(rows):
            assert 0 <= o[r] < n and sample_ok(xf[r], inv_t, seed, step, r, o[r]), (n, step, r, o[r])


def test_sample_rows_never_draws_a_dead_index(hip):
    """A row that is -inf except at five scattered indices, one of them in the last workgroup: every draw is one of the five."""
    n, rows, seed, T = 65537, 3, 99, 0.7
    live = [3, 700, 40000, 65000, 65536]
    x = torch.full((rows, n + 8), float("nan"))
    x[:, :n] = float("-inf")
    x[:, live] = torch.tensor([0.5, -1.0, 2.0, 0.0, 1.0])
    xd = dev(x.bfloat16())
    out = torch.full((rows,), -1, dtype=I32, device="cuda")
    scr = scratch_for(rows)
    rng = hip.make_rng(seed, T, "cuda")
    seen = set()
    for step in range(8):
        hip.sample_rows_bf16(xd[:, :n], out, scr, rng)
        got = out.cpu().tolist()
        assert all(g in live for g in got), (step, got)
        for r in range(rows):
            assert sample_ok(x[r, :n].numpy(), float(np.float32(1.0 / T)), seed, step, r, got[r])
        seen.update(got)
    assert int(rng.cpu()[2]) == 8
    note("sampler: distinct live indices drawn in 24 draws", len(seen))


def test_sample_rows_graph_replay_equals_eager(hip):
    """One captured call replayed three times draws what three eager calls draw from the same starting step, and the step
    word ends 3 higher."""
    n, rows, seed, T = 65536, 3, 4242, 0.9
    xd = dev((I.rnd(rows, n, seed=17) * 3).bfloat16())
    out = torch.full((rows,), -1, dtype=I32, device="cuda")
    scr = scratch_for(rows)
    rng = hip.make_rng(seed, T, "cuda")
    start = 5
    rng[2] = start
    eager = []
    for _ in range(3):
        hip.sample_rows_bf16(xd, out, scr, rng)
        eager.append(out.cpu().tolist())
    assert int(rng.cpu()[2]) == start + 3
    rng[2] = start
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        hip.sample_rows_bf16(xd, out, scr, rng)                     # warm-up on the capture stream
        side.synchronize()
        rng[2] = start
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            hip.sample_rows_bf16(xd, out, scr, rng)
    torch.cuda.synchronize()
    assert int(rng.cpu()[2]) == start                               # capturing runs nothing
    replayed = []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        replayed.append(out.cpu().tolist())
    assert replayed == eager, (replayed, eager)
    r = rng.cpu()
    assert int(r[2]) == start + 3
    assert_scratch(scr, rows, "graph replay")


# --------------------------------------------------------------------------------------------- B. camera tail
def camera_launch(hip, fd, N, P, wd, wt, bt):
    """One launch into a sentinel buffer with a guard view; returns pose [N, 4, 4] on the host."""
    def run():
        buf = I.sentinel((N + 1, 4, 4), F32, "cuda")
        hip._ck(hip.lib().g2v_camera_tail(hip._p(fd), N, P, *[hip._p(a) for a in wd[:4]], hip._p(wt), hip._p(bt), hip._p(wd[6]),
                                          hip._p(wd[7]), hip._p(buf), hip._stream()), "g2v_camera_tail")
        return (buf,)
    buf, = twice(run)
    assert bool(I.is_sentinel(buf[N:]).all()), "camera_tail wrote past its N views"
    return buf[:N].cpu()


def camera_run(hip, feat, w):
    """(pose, t, m9): the pose launch and the kernel's own fp32 m9, read back through the translation column in three more
    launches with wt, bt = rows 0-2, 3-5, 6-8 of wr, br.  t comes from a launch of its own (another buffer, the rotation
    head fed the translation rows too); the pose's translation must equal it bit for bit, and the three recovery launches,
    which share wr and br with the pose launch, must return its rotation block bit for bit."""
    N, P = feat.shape[0], feat.shape[1]
    fd, wd = dev(feat), [dev(a.contiguous()) for a in w]
    pose = camera_launch(hip, fd, N, P, wd, wd[4], wd[5])
    rec = [camera_launch(hip, fd, N, P, wd, wd[6][3 * k:3 * k + 3].contiguous(), wd[7][3 * k:3 * k + 3].contiguous()) for k in range(3)]
    for k in range(3):
        assert torch.equal(I.bits(rec[k][:, :3, :3]), I.bits(pose[:, :3, :3])), f"recovery launch {k}: another rotation"
    wt9 = wd[:6] + [torch.cat([wd[4]] * 3).contiguous(), torch.cat([wd[5]] * 3).contiguous()]
    t = camera_launch(hip, fd, N, P, wt9, wd[4], wd[5])[:, :3, 3].clone()
    assert torch.equal(I.bits(pose[:, :3, 3]), I.bits(t)), "the pose's translation differs from an independent launch's t"
    return pose, t, torch.cat([r[:, :3, 3] for r in rec], 1)


def assert_rotation_always(pose, what):
    orth, det, row3 = I.rotation_defects(pose)
    note("rotation |RtR - I| / u", orth); note("rotation |det - 1| / u", det)
    assert orth <= 8 and det <= 8 and row3, (what, orth, det, row3)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 7, 8, 37])
def test_camera_mean_and_mlp(hip, P):
    feat = I.camera_features(3, P, seed=200 + P)
    w = I.camera_weights_b1(300)
    pose, t, m9 = camera_run(hip, feat, w)
    for name, got, W, b in (("t", t, w[4], w[5]), ("m9", m9, w[6], w[7])):
        ref, e = I.camera_ref64(feat, *w[:4], W, b)
        res = I.check_camera_linear(got, ref, e)
        print(f"camera P={P} {name}: largest |got - ref| / e = {res.max_ratio:.3g}")
        note(f"camera B1 err/e ({name})", res.max_ratio)
        assert res.count == 0, res.report(f"camera {name} P={P}")
    assert_rotation_always(pose, f"P={P}")


def test_camera_rotation_random_views(hip):
    feat, w = I.rotation_views()
    m9_ref, _ = I.camera_ref64(feat, *w[:4], w[6], w[7])
    _, gap0, d0 = I.rotation_ref64(m9_ref.float())
    assert int((d0 < 0).sum()) >= 3 and int((d0 > 0).sum()) >= 3 and float(gap0.min()) >= 0.125   # before launching
    pose, t, m9 = camera_run(hip, feat, w)
    R_ref, gap, d = I.rotation_ref64(m9)
    assert torch.equal(d, d0) and float(gap.min()) >= 0.125
    note("rotation: smallest gap of the 8 views", float(gap.min()))
    res = I.check_rotation(pose[:, :3, :3], R_ref, gap)
    print(f"rotation, 8 views: largest error / bound = {res.max_ratio:.3g}")
    note("rotation err/bound (random views)", res.max_ratio)
    assert res.count == 0, res.report("rotation")
    assert_rotation_always(pose, "random views")
    # the same launches under B1's bound: layers of mixed signs (the bound is wide there, see imageop_check.py)
    for name, got, W, b in (("t", t, w[4], w[5]), ("m9", m9, w[6], w[7])):
        ref, e = I.camera_ref64(feat, *w[:4], W, b)
        r1 = I.check_camera_linear(got, ref, e)
        note(f"camera B1 err/e, mixed signs ({name})", r1.max_ratio)
        assert r1.count == 0, r1.report(f"camera {name}, mixed signs")


def test_camera_rotation_exact_inputs(hip):
    """wr = 0 and br = M: m9 = M exactly."""
    feat = I.camera_features(1, 3, seed=77)
    w = list(I.camera_weights(310))
    w[6] = torch.zeros(9, 512)
    refs = {}
    for name, M, share in I.exact_rotation_inputs():
        w[7] = M.reshape(9).clone()
        R_ref, gap, d = I.rotation_ref64(M.reshape(1, 9))
        assert float(gap) >= 0.125, (name, float(gap))
        refs[name] = R_ref
        pose, t, m9 = camera_run(hip, feat, w)
        assert torch.equal(I.bits(m9), I.bits(M.reshape(1, 9))), f"{name}: m9 is not M"
        R = pose[:, :3, :3]
        res = I.check_rotation(R, R_ref, gap)
        print(f"rotation {name}: gap {float(gap):.3g}, error / bound = {res.max_ratio:.3g}")
        note("rotation err/bound (exact inputs)", res.max_ratio)
        assert res.count == 0, res.report(name)
        assert_rotation_always(pose, name)
        if name == "identity":
            assert torch.equal(I.bits(R[0]), I.bits(torch.eye(3)))
        if name.startswith("axis"):
            assert I.check_rotation(M[None], R_ref, gap).count == 0 and abs(float(gap) - 2) < 1e-6
        if share:
            assert I.check_rotation(R, refs[share], gap).count == 0
        if name.startswith("reflection"):
            assert float(d) < 0


# ----------------------------------------------------------------------------------------- C. point head tail
PS_SHAPES = [(14, 14, 14), (14, 28, 42), (14, 42, 28), (16, 16, 16), (16, 48, 32)]


@pytest.mark.parametrize("ps,H,W", PS_SHAPES)
@pytest.mark.parametrize("N", [1, 3])
def test_pts_mode0_and_pixel_shuffle_exact(hip, ps, H, W, N):
    P = (H // ps) * (W // ps)
    lib = hip.lib()
    for C in (1, 2, 3):
        K = C * ps * ps
        fd = dev(I.coded_feat(N * P, K))

        def shuffle():
            buf = I.sentinel((N * H * W * C + 64,), F32, "cuda")
            hip._ck(lib.g2v_pixel_shuffle(hip._p(fd), N, H, W, C, ps, hip._p(buf), hip._stream()), "g2v_pixel_shuffle")
            return (buf,)
        buf, = twice(shuffle)
        assert bool(I.is_sentinel(buf[N * H * W * C:]).all())
        bad, msg = I.check_coded(buf[:N * H * W * C], N, H, W, C, ps)
        assert int(bad.sum()) == 0, f"pixel_shuffle ps={ps} {H}x{W} N={N} C={C}: {int(bad.sum())} wrong; {msg}"
    fd = dev(I.coded_feat(N * P, 3 * ps * ps))

    def mode0():
        buf = I.sentinel((N * H * W * 3 + 64,), F32, "cuda")
        hip._ck(lib.g2v_pts_epilogue_ps(hip._p(fd), N, H, W, ps, 0, None, hip._p(buf), None, hip._stream()), "g2v_pts_epilogue_ps")
        return (buf,)
    buf, = twice(mode0)
    assert bool(I.is_sentinel(buf[N * H * W * 3:]).all())
    bad, msg = I.check_coded(buf[:N * H * W * 3], N, H, W, 3, ps)
    assert int(bad.sum()) == 0, f"pts_epilogue mode 0 ps={ps} {H}x{W} N={N}: {int(bad.sum())} wrong; {msg}"


@pytest.mark.parametrize("ps,H,W", PS_SHAPES)
@pytest.mark.parametrize("N", [1, 3])
def test_pts_mode1(hip, ps, H, W, N):
    feat, pose = I.pts_inputs(N, H, W, ps, seed=7 * H + W + N)
    fd, pd = dev(feat), dev(pose)
    n3 = N * H * W * 3

    def run():
        loc, wld = I.sentinel((n3 + 64,), F32, "cuda"), I.sentinel((n3 + 64,), F32, "cuda")
        hip._ck(hip.lib().g2v_pts_epilogue_ps(hip._p(fd), N, H, W, ps, 1, hip._p(pd), hip._p(loc), hip._p(wld), hip._stream()),
                "g2v_pts_epilogue_ps")
        return loc, wld
    loc, wld = twice(run)
    assert bool(I.is_sentinel(loc[n3:]).all()) and bool(I.is_sentinel(wld[n3:]).all())
    res = I.check_pts_mode1(feat, pose, N, H, W, ps, loc[:n3], wld[:n3])
    print(f"pts mode 1 ps={ps} {H}x{W} N={N}: error / bound z {res.z.max_ratio:.3g}, lx/ly {res.xy.max_ratio:.3g}, world {res.world.max_ratio:.3g}")
    for k, r in (("z", res.z), ("lx/ly", res.xy), ("world", res.world)):
        note(f"pts mode 1 err/bound ({k})", r.max_ratio)
    assert res.count == 0, res.report(f"pts mode 1 ps={ps} {H}x{W} N={N}")
    if N == 3:                                                       # each view has its own pose: swapped poses are flagged
        assert I.check_pts_mode1(feat, pose.roll(1, 0), N, H, W, ps, loc[:n3], wld[:n3]).world.flagged_rows() == [0, 1, 2]


# ------------------------------------------------------------------------------------------- D. DINO front end
@pytest.mark.parametrize("H,W", [(14, 14), (42, 56), (56, 42)])
@pytest.mark.parametrize("N", [1, 3])
def test_im2col14_exact(hip, H, W, N):
    rows = N * (H // 14) * (W // 14)
    for family, img in (("coded", I.coded_image(N, H, W)), ("special", I.special_image(N, H, W))):
        imd = dev(img)
        for Kpad in (592, 640):
            def run():
                buf = I.sentinel((rows + 2, Kpad), BF, "cuda")
                hip._ck(hip.lib().g2v_im2col14(hip._p(imd), N, H, W, hip._p(buf), Kpad, hip._stream()), "g2v_im2col14")
                return (buf,)
            buf, = twice(run)
            assert bool(I.is_sentinel(buf[rows:]).all()), "im2col14 wrote past its rows"
            got = buf[:rows].cpu()
            assert not bool((I.bits(got[:, 588:]) != 0).any()), "padding columns are not +0"
            bad, msg = I.check_im2col14(got, img, Kpad, coded=family == "coded")
            assert int(bad.sum()) == 0, f"im2col14 {family} {H}x{W} N={N} Kpad={Kpad}: {int(bad.sum())} wrong; {msg}"


@pytest.mark.parametrize("N,P,C", [(1, 1, 4), (3, 12, 128), (2, 5, 1024)])
def test_dino_assemble_exact(hip, N, P, C):
    patch, cls, regs, pos = I.dino_inputs(N, P, C, seed=N + P + C)
    pd, cd, rd, od = dev(patch), dev(cls), dev(regs), dev(pos)
    rows = N * (P + 5)

    def run():
        buf = I.sentinel((rows + 2, C), F32, "cuda")
        hip._ck(hip.lib().g2v_dino_assemble(hip._p(pd), hip._p(cd), hip._p(rd), hip._p(od), hip._p(buf), N, P, C, hip._stream()),
                "g2v_dino_assemble")
        return (buf,)
    buf, = twice(run)
    assert bool(I.is_sentinel(buf[rows:]).all()), "dino_assemble wrote past its rows"
    want = I.dino_assemble_ref(patch, cls, regs, pos, N, P)
    bad = I.bits(buf[:rows].cpu()) != I.bits(want)
    assert int(bad.sum()) == 0, f"dino_assemble N={N} P={P} C={C}: {int(bad.sum())} differ, first at {bad.nonzero()[0].tolist()}"


# ------------------------------------------------------------------------------------------------ E. swiglu
@pytest.mark.parametrize("n", [16, 512, 1000, 8960])
def test_swiglu_bf16(hip, n):
    gu = I.swiglu_inputs(n, seed=n)
    gd = dev(gu)

    def run():
        buf = I.sentinel((n + 16,), BF, "cuda")
        hip._ck(hip.lib().g2v_swiglu_bf16(hip._p(gd), hip._p(buf), n, hip._stream()), "g2v_swiglu_bf16")
        return (buf,)
    buf, = twice(run)
    assert bool(I.is_sentinel(buf[n:]).all()), "swiglu wrote past n"
    res = I.check_swiglu(buf[:n], gu, n)
    g, _ = I.swiglu_split(gu, n)
    print(f"swiglu n={n}: multi share {res.multi_share:.3g}; flagged gates {[float(g[i[0]]) for i in res.where()[:8]]}")
    note(f"swiglu multi share n={n}", res.multi_share)
    assert res.count == 0, res.report(f"swiglu n={n}")
    if n >= 1000:
        assert res.multi_share <= I.MULTI_CAP
