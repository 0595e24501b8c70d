"""GPU: g2v_cloud_render (csrc/render.hip) against the fp32 rule of tests/render_check.py, byte for byte: the synthetic scene at
every shape class, hand-built inputs for each branch of the rule, contention on one target pixel, scenes that a fused multiply-add
would get wrong, determinism, untouched inputs and graph capture."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import consistency_check as cc  # noqa: E402
import render_check as rc  # noqa: E402
from g2vlm_amd import hip  # noqa: E402

pytestmark = pytest.mark.gpu
# (N, H, W) -> (M, OH, OW), skip = self?
CLASSES = [((1, 1, 1), (1, 1, 1), False), ((2, 1, 7), (1, 1, 7), False), ((2, 5, 1), (2, 3, 2), False), ((3, 17, 33), (2, 9, 13), False),
           ((4, 37, 70), (3, 37, 70), False), ((4, 37, 70), (2, 20, 90), False), ((8, 56, 70), (8, 56, 70), True), ((300, 2, 3), (1, 4, 4), False),
           ((2, 518, 518), (2, 518, 518), False)]
BG = 0x2040C0


def ident(c):
    return "x".join(map(str, c[0])) + "-" + "x".join(map(str, c[1]))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(points, colors, mask, poses, K, skip, OH, OW, radius, background, outputs="cdi"):
    """the raw entry point with exactly the optional outputs asked for: c(olor), d(epth), i(ndex)"""
    n, h, w = points.shape[:3]
    M = poses.shape[0]
    t = dict(points=dev(points), colors=dev(colors), mask=dev(mask), poses=dev(poses), K=dev(K),
             skip=None if skip is None else torch.tensor(list(skip), dtype=torch.int32).cuda())
    before = {k: v.clone() for k, v in t.items() if v is not None}
    out = dict(c=torch.full((M, OH, OW, 3), 77, dtype=torch.uint8, device="cuda"), d=torch.full((M, OH, OW), -5.0, dtype=torch.float32, device="cuda"),
               i=torch.full((M, OH, OW), -9, dtype=torch.int32, device="cuda"))
    ws = torch.full((hip.cloud_render_workspace(M, OH, OW) // 8,), 0x0123456789, dtype=torch.int64, device="cuda")   # junk: needs no initialisation
    ptr = {k: hip._p(out[k]) if k in outputs else None for k in "cdi"}
    rcode = hip.lib().g2v_cloud_render(hip._p(t["points"]), hip._p(t["colors"]), hip._p(t["mask"]), n, h, w, hip._p(t["poses"]), hip._p(t["K"]),
                                       hip._p(t["skip"]), M, OH, OW, radius, background, ptr["c"], ptr["d"], ptr["i"], hip._p(ws),
                                       ws.numel() * 8, hip._stream())
    assert rcode == 0
    torch.cuda.synchronize()
    assert all(torch.equal(t[k].view(torch.uint8), v.view(torch.uint8)) for k, v in before.items())   # the inputs are untouched
    for k, sentinel in (("c", 77), ("d", -5.0), ("i", -9)):
        if k not in outputs:
            assert bool((out[k] == sentinel).all()), k                                              # an output not asked for is not written
    return {k: out[k].cpu().numpy() for k in outputs}


def check(got, want):
    if "c" in got:
        assert np.array_equal(got["c"], want["color"]), int((got["c"] != want["color"]).sum())
    if "d" in got:
        assert np.array_equal(got["d"].view(np.int32), want["depth"].view(np.int32)), int((got["d"].view(np.int32) != want["depth"].view(np.int32)).sum())
    if "i" in got:
        assert np.array_equal(got["i"], want["index"]), int((got["i"] != want["index"]).sum())


@pytest.fixture(scope="module")
def scenes():
    """per class: (args without mask / radius, mask, {(masked, radius): rule}), computed once"""
    out = {}
    for n, (src, tgt, self_skip) in enumerate(CLASSES):
        s = cc.scene(*src, seed=n)
        colors = rc.scene_colors(*src, seed=n)
        mask = cc.random_mask(src, 200 + n)
        poses, K = rc.targets(s, *tgt)
        skip = list(range(tgt[0])) if self_skip else None
        want = {(masked, r): rc.rule(s["points"], colors, mask if masked else None, poses, K, skip, tgt[1], tgt[2], r, BG)
                for masked in (False, True) for r in (0, 1)}
        out[ident((src, tgt))] = (s["points"], colors, mask, poses, K, skip, tgt[1], tgt[2], want)
    return out


@pytest.mark.parametrize("cls", CLASSES, ids=ident)
def test_kernel_equals_the_rule_byte_for_byte(scenes, cls):
    points, colors, mask, poses, K, skip, OH, OW, want = scenes[ident(cls)]
    for (masked, r), w in want.items():
        check(run(points, colors, mask if masked else None, poses, K, skip, OH, OW, r, BG), w)
    if points.shape[1] * points.shape[2] > 100:
        assert all((w["index"] >= 0).any() for w in want.values()) and (want[(True, 0)]["index"] < 0).any()      # holes at radius 0
    if points.shape[0] * points.shape[1] * points.shape[2] < 100000:                               # every optional output on and off
        for outputs in ("c", "d", "i", "cd", "ci", "di"):
            check(run(points, colors, mask, poses, K, skip, OH, OW, 1, BG, outputs), want[(True, 1)])
        check(run(points, None, mask, poses, K, skip, OH, OW, 1, BG, "di"), want[(True, 1)])        # no colours needed without color_out


@pytest.mark.parametrize("radius", [3, 8])
def test_large_radii(scenes, radius):
    points, colors, mask, poses, K, skip, OH, OW, _ = scenes["4x37x70-3x37x70"]
    for m in (None, mask):
        check(run(points, colors, m, poses, K, skip, OH, OW, radius, BG), rc.rule(points, colors, m, poses, K, skip, OH, OW, radius, BG))


def hand(points, OH, OW, K=None, pose=None):
    """one source view of 1 x len(points) pixels, one target with the identity pose; K defaults to fx = fy = 1, cx = cy = 0: u = x / z"""
    p = np.asarray(points, np.float32).reshape(1, 1, -1, 3)
    Km = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32) if K is None else np.asarray(K, np.float32)
    pm = np.eye(4, dtype=np.float32) if pose is None else np.asarray(pose, np.float32)
    colors = rc.scene_colors(1, 1, p.shape[2], seed=p.shape[2])
    return p, colors, pm[None], Km[None]


def both(p, colors, mask, poses, K, skip, OH, OW, radius, bg=BG):
    """the kernel's outputs after they were found equal to the rule's"""
    want = rc.rule(p, colors, mask, poses, K, skip, OH, OW, radius, bg)
    check(run(p, colors, mask, poses, K, skip, OH, OW, radius, bg), want)
    return want


def test_every_branch_of_the_rule_on_hand_built_inputs():
    f = np.float32
    down = lambda x: np.nextafter(f(x), f(-np.inf))  # noqa: E731
    OH, OW = 3, 5
    # u == OW and v == OH are outside, one ulp below is inside; u = 0 and -0.0 are inside, one denormal below 0 is outside.
    # Were u == OW taken as inside, the key would go to the next row; v == OH, past the target's plane.
    pts = [(OW, 0.5, 1), (down(OW), 0.5, 1), (0.5, OH, 1), (0.5, down(OH), 1), (0.0, 1.5, 1), (-0.0, 2.5, 1), (down(0.0), 1.5, 1), (OW, OH, 1),
           (down(OW), down(OH), 1)]
    p, colors, pose, K = hand(pts, OH, OW)
    w = both(p, colors, None, pose, K, None, OH, OW, 0)
    want = np.full((OH, OW), -1)
    want[0, 4], want[2, 0], want[1, 0], want[2, 4] = 1, 3, 4, 8                                     # point 5 ties with 3 on (2, 0): the lower index
    assert np.array_equal(w["index"][0], want) and w["landed"][0] == 5
    K0 = np.array([[-1, 0, -0.0], [0, 1, 0], [0, 0, 1]], np.float32)                                # u = -1 * 0 + -0.0 = -0.0: inside (>= 0 holds)
    p, colors, pose, K = hand([(0.0, 0.5, 1)], 1, 2, K=K0)
    assert both(p, colors, None, pose, K, None, 1, 2, 0)["index"].tolist() == [[[0, -1]]]
    # q2 = 0, negative, +inf, NaN or inf coordinates: nothing lands; a positive denormal depth lands and comes back with its bits
    tiny = np.frombuffer(np.uint32(5).tobytes(), np.float32)[0]
    p, colors, pose, K = hand([(0, 0, 0), (0, 0, -1), (0, 0, np.inf), (np.nan, 0, 1), (0, np.inf, 1), (0, 0, tiny), (1, 1, np.nan)], 1, 1)
    w = both(p, colors, None, pose, K, None, 1, 1, 0)
    assert w["index"].tolist() == [[[5]]] and w["depth"].view(np.uint32).tolist() == [[[5]]]
    # q2 = +inf from finite coordinates, q0 = q1 = 0 so that u = v = 0 would be inside: refused by the finite test
    p, colors, pose, K = hand([(0, 0, 3e38)], 1, 1, pose=np.diag([1, 1, 2, 1]))
    assert both(p, colors, None, pose, K, None, 1, 1, 0)["index"].tolist() == [[[-1]]]
    # a NaN in a target's K or pose: that view is background / 0 / -1 as a whole; a skip out of range skips nobody
    s = cc.scene(2, 5, 7)
    colors = rc.scene_colors(2, 5, 7)
    poses, K = rc.targets(s, 4, 5, 7)
    K[1, 0, 2] = np.nan
    poses[2, 1, 3] = np.nan
    poses[3, 0, 0] = np.inf
    w = both(s["points"], colors, None, poses, K, [2, -1, 0, 2 ** 31 - 1], 5, 7, 1, 0xFF8001)
    assert (w["index"][1:] == -1).all() and (w["depth"][1:] == 0).all() and (w["color"][1:] == [255, 128, 1]).all() and (w["index"][0] >= 0).any()
    assert np.array_equal(w["index"][0], rc.rule(s["points"], None, None, poses, K, None, 5, 7, 1, 0)["index"][0])
    assert both(s["points"], colors, None, poses, K, [-2 ** 31, 5, 1, 0], 5, 7, 0, 0)["index"].max() >= 0
    # bit-identical q2 on one target pixel: the lower index wins; a nearer point with a higher index still beats both
    p, colors, pose, K = hand([(0.9, 0.5, 2), (0.5, 0.5, 1), (0.2, 0.2, 1), (0.7, 0.1, 1.5)], 1, 1)
    assert both(p, colors, None, pose, K, None, 1, 1, 0)["index"].tolist() == [[[1]]]
    p, colors, pose, K = hand([(0.5, 0.5, 1), (0.2, 0.2, 1), (0.35, 0.05, 0.5)], 1, 1)
    assert both(p, colors, None, pose, K, None, 1, 1, 3)["index"].tolist() == [[[2]]]
    # radius 8 centred on each corner of a 20 x 30 image: a clipped 9 x 9 square per corner; the background is not black
    OH, OW = 20, 30
    p, colors, pose, K = hand([(0.5, 0.5, 1), (OW - 0.5, 0.5, 1), (0.5, OH - 0.5, 1), (OW - 0.5, OH - 0.5, 1)], OH, OW)
    w = both(p, colors, None, pose, K, None, OH, OW, 8, 0xFEDCBA)
    want = np.full((OH, OW), -1)
    want[:9, :9], want[:9, -9:], want[-9:, :9], want[-9:, -9:] = 0, 1, 2, 3
    assert np.array_equal(w["index"][0], want) and (w["color"][0, 10, 15] == [0xFE, 0xDC, 0xBA]).all()
    assert both(p, colors, None, pose, K, None, OH, OW, 8, 0)["color"][0, 10, 15].tolist() == [0, 0, 0]


@pytest.mark.parametrize("radius", [0, 8])
def test_contention_every_point_on_one_target_pixel(scenes, radius):
    """a camera far above the scene with a tiny focal length: all 4 x 37 x 70 points fall into the centre pixel of a 17 x 17 target"""
    points, colors, mask, _, _, _, _, _, _ = scenes["4x37x70-3x37x70"]
    poses = np.eye(4, dtype=np.float32)[None].copy()
    poses[0, :3, :3] = cc.look_at_origin(np.array([0.3, 0.2, 500.0]))
    poses[0, :3, 3] = (0.3, 0.2, 500.0)
    K = np.array([[[1.0, 0, 8.5], [0, 1.0, 8.5], [0, 0, 1]]], np.float32)
    for m in (None, mask):
        want = rc.rule(points, colors, m, poses, K, None, 17, 17, radius, BG)
        eligible = np.isfinite(points).all(-1) & (True if m is None else m != 0)
        assert want["landed"][0] == eligible.sum() > 5000
        side = min(2 * radius + 1, 17)
        assert (want["index"][0] >= 0).sum() == side * side and len(np.unique(want["index"][0])) == (1 if side == 17 else 2)
        check(run(points, colors, m, poses, K, None, 17, 17, radius, BG), want)


def test_a_scene_that_a_fused_u_or_v_would_get_wrong():
    """consistency_check.fma_scene's points and cameras: view 0's points fall into another pixel when u = fx r + cx is rounded once"""
    s, picked = cc.fma_scene()
    assert picked.sum() >= 32
    H, W = s["points"].shape[1:3]
    colors = rc.scene_colors(*s["points"].shape[:3])
    a = (s["points"], colors, None, s["poses"], s["K"], None, H, W, 0, BG)
    want, fused = rc.rule(*a), rc.rule(*a, fused_uv=True)
    differ = want["index"] != fused["index"]
    assert differ.sum() >= 32 and differ.any((1, 2)).all()                                          # in every target
    got = run(*a)
    check(got, want)
    assert (got["i"] != fused["index"])[differ].all()


def test_a_posed_scene_that_contracted_rotation_sums_would_get_wrong():
    """consistency_check.fma_pose_scene's points under its generic pose: every way of contracting (a d0 + b d1) + c d2 moves some q2
    by an ulp, which the depth map shows bit for bit; the kernel gives the unfused bytes"""
    s, _ = cc.fma_pose_scene()
    H, W = s["points"].shape[1:3]
    colors = rc.scene_colors(*s["points"].shape[:3])
    a = (s["points"], colors, None, s["poses"][1:], s["K"][1:], None, H, W, 0, BG)
    want = rc.rule(*a)
    assert (want["index"] >= 0).sum() >= 32
    got = run(*a)
    check(got, want)
    for form in cc.FUSED_Q:
        fused = rc.rule(*a, fused_q=form)
        differ = fused["depth"].view(np.int32) != want["depth"].view(np.int32)
        assert differ.sum() >= 8, form
        assert (got["d"].view(np.int32) != fused["depth"].view(np.int32))[differ].all(), form


def test_two_runs_give_the_same_bytes_and_the_wrapper_equals_the_entry_point(scenes):
    points, colors, mask, poses, K, skip, OH, OW, want = scenes["8x56x70-8x56x70"]
    first, second = run(points, colors, mask, poses, K, skip, OH, OW, 1, BG), run(points, colors, mask, poses, K, skip, OH, OW, 1, BG)
    assert all(np.array_equal(first[k], second[k]) for k in first)
    color, depth, index = hip.cloud_render(dev(points), dev(colors), dev(mask).view(torch.bool), dev(poses), dev(K), (OH, OW), 1, BG,
                                           torch.arange(8, dtype=torch.int32, device="cuda"))
    check(dict(c=color.cpu().numpy(), d=depth.cpu().numpy(), i=index.cpu().numpy()), want[(True, 1)])
    only = hip.cloud_render(dev(points), None, None, dev(poses), dev(K), (OH, OW), 0, 0, torch.arange(8, dtype=torch.int32, device="cuda"),
                            color=False, depth=False)
    assert only[0] is None and only[1] is None
    check(dict(i=only[2].cpu().numpy()), want[(False, 0)])


def test_the_call_is_capturable_and_the_replay_equals_the_eager_run(scenes):
    points, colors, mask, poses, K, skip, OH, OW, want = scenes["4x37x70-3x37x70"]
    t = [dev(points), dev(colors), dev(mask), dev(poses), dev(K)]
    eager = hip.cloud_render(*t, (OH, OW), 1, BG)                                                   # loads the code object, sizes the workspace
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            out = hip.cloud_render(*t, (OH, OW), 1, BG)
    for _ in range(2):
        for o in out:
            o.fill_(9)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o.view(torch.uint8), e.view(torch.uint8)) for o, e in zip(out, eager))
        check(dict(c=out[0].cpu().numpy(), d=out[1].cpu().numpy(), i=out[2].cpu().numpy()), want[(True, 1)])
