"""CPU (no GPU): the checks of tests/imageop_check.py against honest emulations and injected faults.

Honest emulations - fp32 restatements of argmax_bf16_kernel's merge tree, camera_tail_kernel (the 4-way unrolled mean with
its tail, matvec512's 8 fma + xor tree + bias, the fp32-normalised double-precision Jacobi), pts_epilogue_kernel mode 1,
swiglu_bf16_kernel, and the exact index maps - must give zero flags; the camera, rotation and point-head checks must stay
under half of their bounds, and swiglu's share of multi-valued elements under the 2 % cap.  The maxima are printed (STATS
lines, visible with -s) and quoted in imageop_check.py's docstring.

Every injected fault must be flagged: the argmax rule the kernel had before (NaN merged as +inf) on exactly the
inf-before-NaN rows; in the camera tail the last patch row left out of the mean (P = 37 and 5), s1 dropped from the four
partial sums, one bias dropped, ReLU skipped on one unit, another view's mean; a rotation without the reflection flip or with
the wrong direction flipped; in the point head iy / ix swapped, channel stride PS for PS^2, gw replaced by gh on the
non-square shapes, the pose of view n - 1, one pixel reading its neighbour's feature; in im2col14 a ky / kx transpose
(which a GEMM on smooth input does not see); in dino_assemble a shifted position row and another view's patches; in swiglu
a skipped inner rounding and exchanged gate / up.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imageop_check as I  # noqa: E402

STATS = {}
PS_SHAPES = [(14, 14, 14), (14, 28, 42), (14, 42, 28), (16, 16, 16), (16, 48, 32)]


@pytest.fixture(scope="module", autouse=True)
def measured():
    yield
    for k, v in sorted(STATS.items(), key=str):
        print("STATS", k, f"{v:.3g}")


def note(k, v):
    STATS[k] = max(STATS.get(k, 0.0), float(v))


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------ A. token pickers
def test_philox_known_answer():
    """Random123's known-answer vector for philox4x32-10 with an all-zero counter and key (first word)."""
    assert int(I.philox_first(0, 0, 0, 0, 0, 0)) == 0x6627E8D5


def test_argmax_reference_rules():
    nan, inf = float("nan"), float("inf")
    assert int(I.argmax_ref(torch.tensor([1, inf, 2, nan, 3]))) == 3
    assert int(I.argmax_ref(torch.tensor([nan, inf, nan]))) == 0
    assert int(I.argmax_ref(torch.full((7,), -inf))) == 0
    assert int(I.argmax_ref(torch.tensor([-1.0, -0.0, 0.0]))) == 1 and int(I.argmax_ref(torch.tensor([-1.0, 0.0, -0.0]))) == 1
    assert int(I.argmax_ref(torch.tensor([1.0, 3.0, 3.0]).bfloat16())) == 1


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 65535, 65536, 65537, 151936])
def test_argmax_emulation_and_the_old_nan_rule(n):
    cases = I.argmax_cases(n)
    x = I.argmax_matrix(cases, n)
    assert bool(torch.isinf(x[:, n::2].float()).all()) and bool(torch.isnan(x[:, n + 1::2].float()).all())
    want = I.argmax_ref(x[:, :n]).tolist()
    rows = x[:, :n].float().numpy()
    names = [c[0] for c in cases]
    for r, name in enumerate(names):
        assert I.argmax_emul(rows[r]) == want[r], (n, name)
        if name.startswith(("decr max@", "const max@")):
            assert want[r] == int(name.split("@")[1])
        if " tie@" in name:
            assert want[r] == int(name.split("@")[1].split(",")[0])
    # the rule before the fix: flagged on the rows with +inf below a NaN, and on no other row
    old_wrong = {name for r, name in enumerate(names) if I.argmax_emul(rows[r], nan_as_inf=True) != want[r]}
    inf_first = {name for name in names if name.startswith("inf@")}
    assert old_wrong == inf_first, (n, old_wrong ^ inf_first)
    if n >= 2:
        assert inf_first
    # a 64-workgroup walk of a short row and a 1-workgroup walk of a long one agree with the reference too
    if n in (257, 65536):
        for r in range(len(names)):
            assert I.argmax_emul(rows[r], nb=64 if n == 257 else 1) == want[r]


def test_argmax_cases_reach_every_boundary():
    names = {c[0] for c in I.argmax_cases(65537)}
    per = 1025
    for i in (0, 65536, 63, 64, 255, 256, per - 1, per, 32 * per - 1, 32 * per, 63 * per - 1, 63 * per):
        assert f"decr max@{i}" in names and f"const max@{i}" in names
    for t in ("63,64", "255,256", f"{per - 1},{per}", f"{32 * per - 1},{32 * per}", f"{63 * per - 1},{63 * per}", "0,65536"):
        assert f"decr tie@{t}" in names
    for s in ("inf@0 NaN@1", "NaN@0 inf@1", "inf@100 NaN@356", "inf@5 NaN@65534", "NaN@5 inf@65534", "NaN@62 NaN@65", "all -inf"):
        assert s in names


def test_gumbel_criterion_on_a_sparse_row():
    """The sampler's criterion on a row that is -inf except at five indices: the host maximiser is one of the five."""
    n = 65537
    x = np.full(n, -np.inf, dtype=np.float32)
    live = [3, 700, 40000, 65000, 65536]
    x[live] = [0.5, -1.0, 2.0, 0.0, 1.0]
    for step in range(8):
        sc = I.gumbel_scores(x, 1.0 / 0.7, 0x1234567890ABCDEF, step, 2)
        assert int(sc.argmax()) in live


# --------------------------------------------------------------------------------------------- B. camera tail
PS_CAMERA = [1, 2, 3, 4, 5, 7, 8, 37]


@pytest.mark.parametrize("P", PS_CAMERA)
def test_camera_emulation_stays_under_half_the_bound(P):
    feat = I.camera_features(3, P, seed=200 + P)
    w = I.camera_weights_b1(300)
    for name, W, b in (("t", w[4], w[5]), ("m9", w[6], w[7])):
        ref, e = I.camera_ref64(feat, *w[:4], W, b)
        res = I.check_camera_linear(I.camera_emul32(feat, *w[:4], W, b), ref, e)
        assert res.count == 0, res.report(f"camera {name} P={P}")
        note(f"camera B1 err/e ({name})", res.max_ratio)
        assert res.max_ratio < 0.5, (name, P, res.max_ratio)
    # the all-zero view's output comes from the biases alone
    zero_ref, _ = I.camera_ref64(torch.zeros(1, P, 512), *w[:4], w[4], w[5])
    ref, _ = I.camera_ref64(feat, *w[:4], w[4], w[5])
    assert float((ref[2] - zero_ref[0]).abs().max()) < 1e-12


@pytest.mark.parametrize("fault,P", [("drop_last_patch", 37), ("drop_last_patch", 5), ("drop_s1", 37), ("drop_s1", 5), ("drop_bias", 5),
                                     ("skip_relu", 5), ("other_view_mean", 5), ("other_view_mean", 1)])
def test_camera_faults_are_flagged(fault, P):
    feat = I.camera_features(3, P, seed=200 + P)
    w = I.camera_weights_b1(300)
    unit = 0
    if fault == "skip_relu":                                  # a first-layer unit that is negative before its ReLU in view 0
        pre = feat.double().mean(1) @ w[0].double().T + w[1].double()
        unit = int(pre[0].argmin())
        assert float(pre[0, unit]) < -0.1
    for W, b in ((w[4], w[5]), (w[6], w[7])):
        ref, e = I.camera_ref64(feat, *w[:4], W, b)
        res = I.check_camera_linear(I.camera_emul32(feat, *w[:4], W, b, fault=fault, unit=unit), ref, e)
        rows = res.flagged_rows()
        if fault in ("drop_last_patch", "drop_s1"):
            assert 0 in rows and 2 not in rows, (fault, P, rows)      # the zero view has nothing to lose
        elif fault == "skip_relu":
            assert 0 in rows
        elif fault == "drop_bias":
            assert rows == [0, 1, 2]
        else:
            assert rows == [0, 1, 2]


def test_rotation_emulation_random_views():
    feat, w = I.rotation_views()
    m9 = I.camera_emul32(feat, *w[:4], w[6], w[7])
    R_ref, gap, d = I.rotation_ref64(m9)
    assert int((d < 0).sum()) >= 3 and int((d > 0).sum()) >= 3 and float(gap.min()) >= 0.125
    note("rotation: smallest gap of the 8 views", float(gap.min()))
    for name, W, b in (("t", w[4], w[5]), ("m9", w[6], w[7])):      # B1's bound on layers of mixed signs: holds, but is wide
        ref, e = I.camera_ref64(feat, *w[:4], W, b)
        r1 = I.check_camera_linear(I.camera_emul32(feat, *w[:4], W, b), ref, e)
        note(f"camera B1 err/e, mixed signs ({name})", r1.max_ratio)
        assert r1.count == 0 and r1.max_ratio < 0.5
    R = torch.stack([I.svd_emul(m9[i].numpy()) for i in range(8)])
    res = I.check_rotation(R, R_ref, gap)
    assert res.count == 0, res.report("rotation")
    note("rotation err/bound (random views)", res.max_ratio)
    assert res.max_ratio < 0.5
    pose = torch.eye(4).repeat(8, 1, 1)
    pose[:, :3, :3] = R
    orth, det, row3 = I.rotation_defects(pose)
    note("rotation |RtR - I| / u", orth); note("rotation |det - 1| / u", det)
    assert orth <= 8 and det <= 8 and row3
    # the reflection branch against fp64: no flip, or the wrong direction flipped, is flagged on every det < 0 view only
    for fault in ("no_flip", "flip_largest"):
        Rf = torch.stack([I.svd_emul(m9[i].numpy(), fault) for i in range(8)])
        assert I.check_rotation(Rf, R_ref, gap).flagged_rows() == (d < 0).nonzero().flatten().tolist()
    # what the older test asserts on a reflection (|det - 1| < 1e-4) accepts the wrong direction
    assert float((torch.linalg.det(torch.stack([I.svd_emul(m9[i].numpy(), "flip_largest") for i in range(8)]).double()) - 1).abs().max()) < 1e-4


def test_rotation_exact_inputs():
    refs = {}
    for name, M, share in I.exact_rotation_inputs():
        m9 = M.reshape(1, 9)
        R_ref, gap, d = I.rotation_ref64(m9)
        assert float(gap) >= 0.125, (name, float(gap))
        refs[name] = R_ref
        R = I.svd_emul(m9[0].numpy())[None]
        res = I.check_rotation(R, R_ref, gap)
        assert res.count == 0, res.report(name)
        note("rotation err/bound (exact inputs)", res.max_ratio)
        assert res.max_ratio < 0.5, (name, res.max_ratio)
        if name == "identity":
            assert torch.equal(R[0], torch.eye(3))
        if name.startswith("axis"):
            assert abs(float(gap) - 2) < 1e-6 and float(d) > 0
            assert I.check_rotation(M[None], R_ref, gap).count == 0             # R = M within the bound
        if share:
            assert I.check_rotation(R, refs[share], gap).count == 0
        if name.startswith("reflection"):
            assert float(d) < 0
            assert I.check_rotation(I.svd_emul(m9[0].numpy(), "no_flip")[None], R_ref, gap).count > 0


# ----------------------------------------------------------------------------------------- C. point head tail
@pytest.mark.parametrize("ps,H,W", PS_SHAPES)
@pytest.mark.parametrize("N", [1, 3])
def test_shuffle_map_is_pixel_shuffle(ps, H, W, N):
    """The index restatement against F.pixel_shuffle, as the older GPU test states the operation."""
    import torch.nn.functional as F
    for C in (1, 2, 3):
        P, K = (H // ps) * (W // ps), C * ps * ps
        feat = I.coded_feat(N * P, K)
        row, col = I.shuffle_map(N, H, W, C, ps)
        want = F.pixel_shuffle(feat.view(N, P, K).transpose(-1, -2).reshape(N, K, H // ps, W // ps), ps).permute(0, 2, 3, 1)
        assert torch.equal(feat[row, col], want)
        assert I.check_coded(feat[row, col], N, H, W, C, ps)[0].sum() == 0
        for fault in ("swap", "stride_ps") + (("gw_as_gh",) if H != W else ()):
            if fault == "stride_ps" and C == 1:
                continue                                          # no second channel to stride to
            r2, c2 = I.shuffle_map(N, H, W, C, ps, fault)
            bad, msg = I.check_coded(feat[r2, c2], N, H, W, C, ps)
            assert int(bad.sum()) > 0 and "read feat[" in msg, (fault, C)


@pytest.mark.parametrize("ps,H,W", PS_SHAPES)
@pytest.mark.parametrize("N", [1, 3])
def test_pts_mode1_emulation_and_faults(ps, H, W, N):
    feat, pose = I.pts_inputs(N, H, W, ps, seed=7 * H + W + N)
    local, world = I.pts_emul32(feat, pose, N, H, W, ps)
    res = I.check_pts_mode1(feat, pose, N, H, W, ps, local, world)
    assert res.count == 0, res.report(f"pts ps={ps} {H}x{W} N={N}")
    for k, r in (("z", res.z), ("lx/ly", res.xy), ("world", res.world)):
        note(f"pts mode 1 err/bound ({k})", r.max_ratio)
        assert r.max_ratio < 0.5, (k, r.max_ratio)
    # the planted pixels: the first six of the last view's last patch
    gw = W // ps
    y0, x0 = H - ps, (gw - 1) * ps
    z = local[N - 1, y0, x0:x0 + 6, 2]
    assert float(z[2]) == 1.0 and float(z[3]) > 1e38 and bool(torch.isinf(z[4:6]).all()) and float(z[0]) < 1e-40
    assert bool(torch.isnan(local[N - 1, y0, x0 + 4, 0])) and bool(torch.isinf(local[N - 1, y0, x0 + 5, 0]))
    assert float(local[N - 1, y0, x0, 0]) == 0.0
    # a flushed subnormal passes; a finite z where z* overflows does not
    l2 = local.clone(); l2[N - 1, y0, x0, 2] = 0.0
    assert I.check_pts_mode1(feat, pose, N, H, W, ps, l2, world).z.count == 0
    l2 = local.clone(); l2[N - 1, y0, x0 + 5, 2] = I.FLT_MAX
    assert I.check_pts_mode1(feat, pose, N, H, W, ps, l2, world).z.count == 1
    for fault in ("swap", "stride_ps") + (("gw_as_gh",) if H != W else ()) + (("prev_pose",) if N == 3 else ()):
        lf, wf = I.pts_emul32(feat, pose, N, H, W, ps, fault)
        rf = I.check_pts_mode1(feat, pose, N, H, W, ps, lf, wf)
        assert rf.count > 0, fault
        if fault == "prev_pose":
            assert rf.z.count == 0 and rf.xy.count == 0 and rf.world.flagged_rows() == [0, 1, 2]
    # one pixel reading its neighbour's feature is named
    if N == 3 and H > 14:
        l1, w1 = local.clone(), world.clone()
        l1[0, 3, 5], w1[0, 3, 5] = local[0, 3, 6], world[0, 3, 6]
        r1 = I.check_pts_mode1(feat, pose, N, H, W, ps, l1, w1)
        assert r1.count > 0 and r1.world.where()[0][:3] == (0, 3, 5)


# ------------------------------------------------------------------------------------------- D. DINO front end
@pytest.mark.parametrize("H,W", [(14, 14), (42, 56), (56, 42)])
@pytest.mark.parametrize("N", [1, 3])
def test_im2col14_reference_and_faults(H, W, N):
    import torch.nn.functional as F
    img = I.coded_image(N, H, W)
    assert img.unique().numel() == img.numel() and torch.equal(img.bfloat16().float(), img)
    for Kpad in (592, 640):
        ref = I.im2col14_ref(img, Kpad)
        # the restatement is Conv2d's own unfolding
        assert torch.equal(ref[:, :588].float(), F.unfold(img, 14, stride=14).transpose(1, 2).reshape(-1, 588))
        assert float(ref[:, 588:].float().abs().max()) == 0 and not bool((I.bits(ref[:, 588:]) != 0).any())
        assert int(I.check_im2col14(ref, img, Kpad, coded=True)[0].sum()) == 0
        for fault in ("swap",) + (("gw_as_gh",) if H != W else ()):
            bad, msg = I.check_im2col14(I.im2col14_ref(img, Kpad, fault), img, Kpad, coded=True)
            assert int(bad.sum()) > 0 and "read img[" in msg
    sp = I.special_image(N, H, W)
    ref = I.im2col14_ref(sp, 592)
    assert int(torch.isnan(ref.float()).sum()) == int(torch.isnan(sp).sum()) > 0
    assert int(I.check_im2col14(ref, sp, 592)[0].sum()) == 0
    trunc = (I.bits(ref).to(torch.int32) & 0xFFFF).clone()
    t2 = ((I.bits(sp).view(N, 3, H // 14, 14, W // 14, 14).permute(0, 2, 4, 1, 3, 5).reshape(-1, 588) >> 16) & 0xFFFF)
    trunc[:, :588] = t2                                           # a truncating conversion instead of round-to-nearest-even
    tr = (trunc - (trunc >= 32768) * 65536).to(torch.int16).view(torch.bfloat16)
    assert int(I.check_im2col14(tr, sp, 592)[0].sum()) > 0


def test_im2col14_transpose_survives_a_gemm_on_smooth_input():
    """Why the direct check: on a smooth image a ky / kx transpose inside the patch moves a bf16 GEMM output by less than the
    older test's tolerance (rel-L2 4e-3), while the exact comparison flags most of the elements."""
    H = W = 28
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    img = (1.0 + 1e-3 * (y + 2 * x))[None, None].repeat(1, 3, 1, 1)
    w = torch.ones(64, 588) * 0.05 + I.rnd(64, 588, seed=1) * 1e-3
    good, swapped = I.im2col14_ref(img, 592), I.im2col14_ref(img, 592, "swap")
    assert rel(swapped[:, :588].float() @ w.T, good[:, :588].float() @ w.T) < 4e-3
    assert int(I.check_im2col14(swapped, img, 592)[0].sum()) > 1000


@pytest.mark.parametrize("N,P,C", [(1, 1, 4), (3, 12, 128), (2, 5, 1024)])
def test_dino_assemble_reference_and_faults(N, P, C):
    patch, cls, regs, pos = I.dino_inputs(N, P, C, seed=N + P + C)
    ref = I.dino_assemble_ref(patch, cls, regs, pos, N, P).view(N, P + 5, C)
    assert torch.equal(I.bits(ref[:, 1:5]), I.bits(regs)[None].expand(N, 4, C))
    assert torch.equal(ref[0, 0], cls + pos[0]) and torch.equal(ref[N - 1, P + 4], patch[N * P - 1].float() + pos[P])
    for fault in ("pos_shift",) + (("other_view",) if N > 1 else ()):
        bad = I.bits(I.dino_assemble_ref(patch, cls, regs, pos, N, P, fault)) != I.bits(ref.view(-1, C))
        assert int(bad.sum()) > 0 and not bool(bad.view(N, P + 5, C)[:, :5].any())


# ------------------------------------------------------------------------------------------------ E. swiglu
@pytest.mark.parametrize("n", [16, 512, 1000, 8960])
def test_swiglu_emulation_and_faults(n):
    gu = I.swiglu_inputs(n, seed=n)
    g, u = I.swiglu_split(gu, n)
    assert not bool(torch.isnan(g.float()).any() | torch.isnan(u.float()).any())
    assert g[:6].tolist() == [20.0, -20.0, 88.0, -88.0, 0.0, -0.0]
    res = I.check_swiglu(I.swiglu_emul32(gu, n), gu, n)
    assert res.count == 0, res.report(f"swiglu n={n}")
    note(f"swiglu multi share n={n}", res.multi_share)
    if n >= 1000:
        assert res.multi_share <= I.MULTI_CAP
    if n >= 512:
        for fault in ("one_rounding", "swap"):
            assert I.check_swiglu(I.swiglu_emul32(gu, n, fault), gu, n).count > 0, fault
    # the inner value flushed to zero at g = -88 (silu* = -5.3e-37, a normal bf16 value) is flagged
    out = I.swiglu_emul32(gu, n)
    out[3] = 0.0
    assert I.check_swiglu(out, gu, n).where() == [(3,)]
