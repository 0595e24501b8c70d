"""GPU: g2v_cloud_consistency (csrc/consistency.hip) against the fp32 rule of tests/consistency_check.py, byte for byte: the
synthetic scene at every shape class, hand-built inputs for each branch of the rule, a scene that a fused multiply-add would get
wrong, determinism, untouched inputs and graph capture."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import consistency_check as cc  # noqa: E402
from g2vlm_amd import hip  # noqa: E402

pytestmark = pytest.mark.gpu
TILE_H, TILE_W = 16, 32                                     # the larger extent of the two tile shapes the kernel has been built with
SHAPES = [(1, 1, 1), (2, 1, 7), (2, 5, 1), (3, TILE_H + 1, TILE_W + 1), (4, 37, 70), (8, 56, 70), (256, 2, 3), (2, 518, 518)]
THRESHOLDS = [(0, -1), (1, 0), (2, -1), (1, 1), (0, 0)]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(s, mask, rtol, min_agree=0, max_in_front=-1, outputs="afpm"):
    """the raw entry point with exactly the optional outputs asked for: a(gree), (in_)f(ront), p(airs), m(ask_out)"""
    n, h, w = s["points"].shape[:3]
    t = {k: dev(s[k]) for k in ("points", "local", "poses", "K")}
    m = dev(mask)
    before = {k: v.clone() for k, v in t.items()}
    out = dict(a=torch.full((n, h, w), 77, dtype=torch.uint8, device="cuda"), f=torch.full((n, h, w), 77, dtype=torch.uint8, device="cuda"),
               p=torch.full((n, n, 2), -5, dtype=torch.int32, device="cuda"), m=torch.full((n, h, w), 77, dtype=torch.uint8, device="cuda"))
    ws = torch.full((hip.cloud_consistency_workspace(n, h, w) // 4,), -7.0, dtype=torch.float32, device="cuda")   # needs no initialisation
    ptr = {k: hip._p(out[k]) if k in outputs else None for k in "afpm"}
    rc = hip.lib().g2v_cloud_consistency(hip._p(t["points"]), hip._p(t["local"]), hip._p(m), hip._p(t["poses"]), hip._p(t["K"]), n, h, w,
                                         float(rtol), min_agree, max_in_front, ptr["a"], ptr["f"], ptr["p"], ptr["m"], hip._p(ws),
                                         ws.numel() * 4, hip._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert all(torch.equal(t[k].view(torch.int32), before[k].view(torch.int32)) for k in t)         # the inputs are untouched
    for k in "afpm":
        if k not in outputs:
            assert bool((out[k] == (-5 if k == "p" else 77)).all()), k                               # an output not asked for is not written
    return {k: out[k].cpu().numpy() for k in outputs}


def check(got, want, min_agree=0, max_in_front=-1):
    if "a" in got:
        assert np.array_equal(got["a"], want["agree"]), int((got["a"] != want["agree"]).sum())
    if "f" in got:
        assert np.array_equal(got["f"], want["in_front"]), int((got["f"] != want["in_front"]).sum())
    if "p" in got:
        assert np.array_equal(got["p"], want["pairs"])
    if "m" in got:
        assert np.array_equal(got["m"], cc.mask_out(want, min_agree, max_in_front).astype(np.uint8))


@pytest.fixture(scope="module")
def scenes():
    """per shape: (scene, mask, rule without the mask, rule with it), computed once"""
    out = {}
    for i, shape in enumerate(SHAPES):
        s = cc.scene(*shape, seed=i)
        mask = cc.random_mask(shape, 100 + i)
        a = (s["points"], s["local"], s["poses"], s["K"])
        out[shape] = (s, mask, cc.rule(*a, None, 0.03), cc.rule(*a, mask, 0.03))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_rule_byte_for_byte(scenes, shape):
    s, mask, plain, masked = scenes[shape]
    for m, want in ((None, plain), (mask, masked)):
        for mn, mx in THRESHOLDS:
            check(run(s, m, 0.03, mn, mx), want, mn, mx)
        for outputs in ("a", "f", "p", "m", "af", "pm", "afm", "afp"):                              # every optional output on and off
            check(run(s, m, 0.03, 1, 0, outputs), want, 1, 0)
    if shape[0] > 1 and shape[1] * shape[2] > 100:
        assert plain["agree"].any() and plain["in_front"].any() and masked["pairs"].sum() > 0


def test_two_runs_give_the_same_bits_and_the_wrapper_equals_the_entry_point(scenes):
    s, mask, _, want = scenes[(8, 56, 70)]
    first, second = run(s, mask, 0.03, 1, 0), run(s, mask, 0.03, 1, 0)
    assert all(np.array_equal(first[k], second[k]) for k in first)
    agree, in_front, mask_out, pairs = hip.cloud_consistency(dev(s["points"]), dev(s["local"]), dev(mask).view(torch.bool), dev(s["poses"]),
                                                             dev(s["K"]), 0.03, 1, 0, pairs=True)
    check(dict(a=agree.cpu().numpy(), f=in_front.cpu().numpy(), m=mask_out.cpu().numpy(), p=pairs.cpu().numpy()), want, 1, 0)
    assert hip.cloud_consistency(dev(s["points"]), dev(s["local"]), None, dev(s["poses"]), dev(s["K"]), 0.03)[3] is None


def hand_scene(px, zt_row, rtol, K=None, W=None):
    """Two views with identity poses.  View 0's pixels are the points (px[k], 0, pz[k]) given as (x, z) pairs; view 1's depth plane
    is zt_row repeated on every row.  fx = fy = 1, cx = 0.5 + 2, cy = 0.5: u = x / z + 2.5 on row 0."""
    px = np.asarray(px, np.float32)
    W = W or max(len(px), len(zt_row))
    points = np.full((2, 1, W, 3), np.nan, np.float32)
    points[0, 0, :len(px)] = np.stack([px[:, 0], np.zeros(len(px), np.float32), px[:, 1]], 1)
    local = np.zeros((2, 1, W, 3), np.float32)
    local[0, ..., 2] = 1.0
    local[1, 0, :len(zt_row), 2] = np.asarray(zt_row, np.float32)
    poses = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    Km = np.tile(np.array([[1, 0, 2.5], [0, 1, 0.5], [0, 0, 1]], np.float32), (2, 1, 1)) if K is None else K
    return dict(points=points, local=local, poses=poses, K=Km)


def test_every_branch_of_the_rule_on_hand_built_inputs():
    f = np.float32
    up, down = (lambda x: np.nextafter(f(x), f(np.inf))), (lambda x: np.nextafter(f(x), f(-np.inf)))
    # |diff| == tol exactly: zt = 1, rtol = 0.25, q2 = 1.25 and 0.75 and one ulp either side; x = 0 keeps u = 2.5 (column 2)
    zs = [1.25, up(1.25), down(1.25), 0.75, up(0.75), down(0.75), 1.0, -1.0, 0.0, np.inf, np.nan]
    s = hand_scene([(0.0, z) for z in zs], [1.0] * 16, 0.25)
    want = cc.rule(s["points"], s["local"], s["poses"], s["K"], None, 0.25)
    assert want["agree"][0, 0, :11].tolist() == [1, 0, 1, 1, 1, 0, 1, 0, 0, 0, 0] and want["in_front"][0, 0, :11].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0]
    check(run(s, None, 0.25), want)
    # the target depth: 0, negative, NaN, inf, a masked pixel; the points sit over columns 0..5 at depth 1 (u = x + 2.5)
    s = hand_scene([(c - 2.0, 1.0) for c in range(6)], [0.0, -1.0, np.nan, np.inf, 1.0, 1.0], 0.25)
    mask = np.ones((2, 1, 6), np.uint8)
    mask[1, 0, 5] = 0
    want = cc.rule(s["points"], s["local"], s["poses"], s["K"], mask, 0.25)
    assert want["agree"][0, 0].tolist() == [0, 0, 0, 0, 1, 0] and not want["in_front"].any()
    check(run(s, mask, 0.25), want)
    # u on an integer, u = -0.0, just below 0, u = W, just below W, 1e30, inf (x / 0 with z = 0 is not inside: q2 > 0 fails), NaN
    W = 12                                                                                         # the image is as wide as the list is long
    xs = [0.5, -2.5, down(-2.5), W - 2.5, down(W - 2.5), 1e30, np.inf, -np.inf, np.nan]
    s = hand_scene([(x, 1.0) for x in xs] + [(1.0, 1e-38), (1.0, 0.0), (-1.0, 1e-45)], [1.0] * W, 0.25)
    assert s["points"].shape[2] == W and f(W - 2.5) + f(2.5) == f(W) and down(W - 2.5) + f(2.5) == down(W)   # u = W and one ulp below it
    want = cc.rule(s["points"], s["local"], s["poses"], s["K"], None, 0.25)
    assert want["agree"][0, 0, :5].tolist() == [1, 1, 0, 0, 1] and want["agree"][0, 0, 5:].sum() == 0
    check(run(s, None, 0.25), want)
    u0 = hand_scene([(-2.5, 1.0)], [1.0] * 4, 0.25)
    u0["K"][:, 0, 2] = 2.5                                                                         # u = -2.5 + 2.5 = +0.0; and with cx = -0.0:
    z0 = hand_scene([(0.0, 1.0), (-0.0, 1.0)], [1.0] * 4, 0.25)
    z0["K"][:, 0, 0], z0["K"][:, 0, 2] = -1.0, -0.0                                                 # u = -1 * 0 + -0 = -0.0: inside (>= 0 holds)
    for sc in (u0, z0):
        want = cc.rule(sc["points"], sc["local"], sc["poses"], sc["K"], None, 0.25)
        assert want["agree"][0, 0, 0] == 1
        check(run(sc, None, 0.25), want)
    # a view with NaN in K confirms nobody (but is confirmed by others); identical poses throughout; a point behind the camera
    s = cc.scene(3, 9, 11, seed=5)
    s["K"][1, 0, 0] = np.nan
    s["points"][0, 0, 0] = (0.0, 0.0, 50.0)                                                         # above every camera: q2 < 0 there
    s["points"][2, 1, 1, 1] = np.inf                                                                # a non-finite P
    want = cc.rule(s["points"], s["local"], s["poses"], s["K"], None, 0.03)
    assert want["pairs"][:, 1].sum() == 0 and want["pairs"][1].sum() > 0 and want["agree"][2, 1, 1] == 0 and not want["eligible"][2, 1, 1]
    check(run(s, None, 0.03, 1, 0), want, 1, 0)


def test_u_equal_W_and_v_equal_H_are_outside_and_one_ulp_below_is_inside():
    """The upper bounds of the inside test.  Two views of 2 x 8 with identity poses, fx = fy = 1, cx = cy = 0 and depth 1 everywhere;
    the pixels of view 1 hold points (x, y, 1), so u = x and v = y exactly in view 0, and view 0's own pixels are not eligible.
    The target is the FIRST plane of the workspace on purpose: were u == W or v == H taken as inside, the lookup at [y W + W] or
    [H W + x] would land on the next row or on view 1's plane - inside the workspace, depth 1 - and count as agree."""
    f, H, W = np.float32, 2, 8
    down = lambda x: np.nextafter(f(x), f(-np.inf))  # noqa: E731
    xy = [(W, 0.5), (down(W), 0.5), (0.5, H), (0.5, down(H)), (W, H), (down(W), down(H)), (W, down(H)), (down(W), H),
          (W, 1.5), (down(W), 1.5), (0.0, 0.0), (W - 0.5, H - 0.5)]
    inside = [0, 1, 0, 1, 0, 1, 0, 0, 0, 1, 1, 1]
    points = np.full((2, H, W, 3), np.nan, np.float32)
    points[1].reshape(-1, 3)[:len(xy)] = [(x, y, 1.0) for x, y in xy]
    local = np.zeros((2, H, W, 3), np.float32)
    local[..., 2] = 1.0
    s = dict(points=points, local=local, poses=np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)),
             K=np.tile(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32), (2, 1, 1)))
    want = cc.rule(s["points"], s["local"], s["poses"], s["K"], None, 0.25)
    assert want["agree"][1].reshape(-1)[:len(xy)].tolist() == inside and not want["agree"][0].any() and not want["in_front"].any()
    assert want["pairs"][1, 0, 0] == sum(inside)
    check(run(s, None, 0.25, 1, 0), want, 1, 0)


def test_a_scene_that_a_fused_multiply_add_would_get_wrong():
    s, picked = cc.fma_scene()
    assert picked.sum() >= 32
    want = cc.rule(s["points"], s["local"], s["poses"], s["K"], None, 0.25)
    fused = cc.rule(s["points"], s["local"], s["poses"], s["K"], None, 0.25, fused_uv=True)
    assert ((want["agree"] != fused["agree"]) | (want["in_front"] != fused["in_front"]))[picked].all()
    got = run(s, None, 0.25)
    check(got, want)
    assert (got["a"] != fused["agree"])[picked].any()


def test_a_posed_scene_that_contracted_rotation_sums_would_get_wrong():
    """the same for the sums of R^T d: a view with a generic rotation and translation, points on its plane q2 = 1.25, where an ulp
    of q2 decides; every way of contracting (a d0 + b d1) + c d2 changes at least 32 pixels, and the kernel gives the rule's bytes"""
    s, picked = cc.fma_pose_scene()
    assert set(picked) == set(cc.FUSED_Q) and all(p.sum() >= 32 for p in picked.values()), {k: int(p.sum()) for k, p in picked.items()}
    want = cc.rule(s["points"], s["local"], s["poses"], s["K"], None, 0.25)
    got = run(s, None, 0.25)
    check(got, want)
    for form, p in picked.items():
        fused = cc.rule(s["points"], s["local"], s["poses"], s["K"], None, 0.25, fused_q=form)
        assert (got["a"] != fused["agree"])[p].all(), form


def test_the_call_is_capturable_and_the_replay_equals_the_eager_run(scenes):
    s, mask, _, want = scenes[(4, 37, 70)]
    t = [dev(s[k]) for k in ("points", "local")] + [dev(mask)] + [dev(s[k]) for k in ("poses", "K")]
    hip.cloud_consistency(*t, 0.03, 1, 0, pairs=True)                                               # loads the code object, sizes the workspace
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            out = hip.cloud_consistency(*t, 0.03, 1, 0, pairs=True)
    for o in out:
        o.fill_(9)
    g.replay()
    torch.cuda.synchronize()
    check(dict(a=out[0].cpu().numpy(), f=out[1].cpu().numpy(), m=out[2].cpu().numpy(), p=out[3].cpu().numpy()), want, 1, 0)
