"""CPU (no GPU): rendering the cloud from any camera (csrc/render.hip, g2vlm_utils.render_point_cloud / orbit_poses /
save_rendered_views), in the style of tests/test_consistency_cpu.py.

1. The C ABI: the entry point and its workspace query are exported, declared and bound; every argument error comes back as -22
   before anything touches a device.
2. The public functions refuse bad arguments before any launch; the inference_recon flags; orbit_poses.
3. The rule of tests/render_check.py - what the kernel is held to on the GPU - on the synthetic scene: fp32 against fp64 outside
   the near-threshold set, against a point-by-point loop, identity, occlusion and the special cases."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import render_check as rc  # noqa: E402
from g2vlm_amd import hip  # noqa: E402

NAMES = ("points", "colors", "mask", "N", "H", "W", "poses", "K", "skip", "M", "OH", "OW", "radius", "background", "color_out", "depth_out",
         "index_out", "workspace", "workspace_bytes", "stream")


# ------------------------------------------------------------------------------------------------ 1. the C ABI
@pytest.fixture(scope="module")
def lib():
    from g2vlm_amd import build
    lib = C.CDLL(build.build())
    for name in ("g2v_cloud_render", "g2v_cloud_render_workspace"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = hip._SIGS[name]
    return lib


def test_library_exports_and_declares_the_entry_points(lib):
    from g2vlm_amd import build
    hdr = open(os.path.join(ROOT, "include", "g2vlm_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    name = "g2v_cloud_render"
    assert hasattr(lib, name) and name in hip.EXPORTS and ("`%s`" % name) in integration
    decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, re.S).group(1)
    assert len(decl.split(",")) == len(hip._SIGS[name][0]) == len(NAMES)
    assert [d.split()[-1].lstrip("*") for d in decl.split(",")] == list(NAMES)
    q = name + "_workspace"
    assert hasattr(lib, q) and q in hip.EXPORTS and ("`%s`" % q) in integration
    decl = re.search(r"\bint64_t %s\((.*?)\);" % q, hdr, re.S).group(1)
    assert [d.split()[-1] for d in decl.split(",")] == ["M", "OH", "OW"] and hip._SIGS[q] == ([C.c_int] * 3, C.c_int64)
    assert "render.hip" in build.SOURCES and "render.hip" not in build.RESOURCE_AUDIT
    assert list(inspect.signature(hip.cloud_render).parameters)[:9] == ["points", "colors", "mask", "poses", "K", "size", "radius", "background",
                                                                        "skip"]
    assert lib.g2v_version() == 1


def call(lib, **kw):
    """A valid argument set (no pointer is dereferenced: every call below is refused before any launch), with overrides."""
    a = dict(points=16, colors=16, mask=16, N=3, H=37, W=70, poses=16, K=16, skip=16, M=2, OH=20, OW=90, radius=1, background=0x102030,
             color_out=16, depth_out=16, index_out=16, workspace=16, workspace_bytes=1 << 20, stream=None)
    a.update(kw)
    return lib.g2v_cloud_render(*[a[k] for k in NAMES])


BAD = [dict(N=0), dict(N=-1), dict(H=0), dict(W=-1), dict(M=0), dict(OH=0), dict(OW=-3), dict(N=4, H=32768, W=32768),
       dict(M=4, OH=32768, OW=32768, workspace_bytes=1 << 40), dict(M=65536, OH=1, OW=1), dict(radius=-1), dict(radius=9), dict(background=-1),
       dict(background=0x1000000), dict(points=None), dict(poses=None), dict(K=None), dict(workspace=None), dict(colors=None),
       dict(color_out=None, depth_out=None, index_out=None), dict(points=18), dict(colors=17), dict(poses=18), dict(K=22), dict(skip=18),
       dict(depth_out=18), dict(index_out=17), dict(workspace=20), dict(workspace=18), dict(workspace_bytes=0),
       dict(workspace_bytes=8 * 2 * 20 * 90 - 1)]


@pytest.mark.parametrize("bad", BAD)
def test_argument_errors_return_einval_without_a_device(lib, bad):
    assert call(lib, **bad) == -22


def test_the_workspace_query(lib):
    ws = lib.g2v_cloud_render_workspace
    for bad in ((0, 5, 5), (3, 0, 5), (3, 5, -1), (4, 32768, 32768), (65536, 1, 1), (2, 2 ** 31 - 1, 1)):
        assert ws(*bad) == 0                                                                       # 0 for every shape the entry point refuses
    assert ws(1, 1, 1) == 8 and ws(2, 20, 90) == 8 * 2 * 20 * 90 and ws(65535, 1, 1) == 8 * 65535 and ws(8, 518, 518) == 8 * 8 * 518 * 518
    assert ws(1, 2 ** 31 - 1, 1) == 8 * (2 ** 31 - 1)


# ------------------------------------------------------------------------------------------------ 2. the public surface
def test_public_functions_refuse_bad_arguments_before_any_launch(monkeypatch):
    import torch
    import g2vlm_utils as top
    from g2vlm_amd import g2vlm_utils as gu
    for name in ("render_point_cloud", "orbit_poses", "save_rendered_views"):
        assert getattr(top, name) is getattr(gu, name) and name in top.__all__
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("a refused call reached the library"))
    pred = dict(points=torch.zeros(1, 2, 4, 6, 3), local_points=torch.ones(1, 2, 4, 6, 3), conf=None, images=torch.zeros(1, 2, 3, 4, 6),
                camera_poses=torch.eye(4).repeat(1, 2, 1, 1))
    eye2, eye3 = torch.eye(4).repeat(2, 1, 1), torch.eye(4).repeat(3, 1, 1)
    K = torch.eye(3)
    for kw in (dict(splat_radius=-1), dict(splat_radius=9), dict(splat_radius=1.0), dict(splat_radius=True), dict(splat_radius=None),
               dict(size=(0, 5)), dict(size=(4, -1)), dict(size=(4.0, 6)), dict(size=5), dict(size=(4, 6, 3)),
               dict(background=(0, 0)), dict(background=(0, 0, 256)), dict(background=(-1, 0, 0)), dict(background=(0.5, 0, 0)), dict(background=7),
               dict(exclude_view="self", camera_poses=eye3, intrinsics=K), dict(exclude_view="others"), dict(exclude_view=[0]),
               dict(exclude_view=[0, 1.5]), dict(exclude_view=3), dict(camera_poses=eye2), dict(camera_poses=eye2, intrinsics=torch.zeros(3, 3, 3)),
               dict(camera_poses=torch.zeros(2, 3, 4), intrinsics=K), dict(camera_poses=eye2.numpy(), intrinsics=K),
               dict(camera_poses=eye2.long(), intrinsics=K), dict(camera_poses=torch.zeros(2, 2, 4, 4), intrinsics=K),
               dict(intrinsics=torch.zeros(3, 3, 3)), dict(intrinsics=np.eye(3)), dict(intrinsics=torch.eye(3).long()),
               dict(mask=torch.ones(2, 4, 5, dtype=torch.bool)), dict(mask=torch.ones(2, 4, 6)), dict(mask=np.ones((2, 4, 6), bool)),
               dict(edge_rtol=-1.0), dict(conf_threshold=0.5)):
        with pytest.raises(ValueError):
            gu.render_point_cloud(pred, **kw)
    with pytest.raises(ValueError, match=r"estimate_intrinsics\(pred\)\[0, i\]"):
        gu.render_point_cloud(pred, camera_poses=eye2)
    for poses in (None, torch.eye(4).repeat(1, 3, 1, 1)):
        bad = dict(pred, camera_poses=poses)
        if poses is None:
            del bad["camera_poses"]
        with pytest.raises(ValueError, match="camera_poses"):
            gu.render_point_cloud(bad)
        with pytest.raises(ValueError, match="camera_poses"):
            gu.orbit_poses(bad)
    with pytest.raises(ValueError):
        gu.render_point_cloud(dict(pred, images=torch.zeros(1, 2, 3, 4, 5)))
    for kw in (dict(frames=0), dict(frames=2.0), dict(frames=True), dict(mask=torch.ones(2, 4, 5, dtype=torch.bool)),
               dict(mask=torch.zeros(2, 4, 6, dtype=torch.bool))):                                 # the last: no kept point
        with pytest.raises(ValueError):
            gu.orbit_poses(pred, **kw)
    with pytest.raises(ValueError, match="up"):                                                    # two cameras whose up directions cancel
        flipped = torch.eye(4).repeat(1, 2, 1, 1)
        flipped[0, 1, 1, 1] = -1.0
        gu.orbit_poses(dict(pred, camera_poses=flipped))
    with pytest.raises(ValueError):                                                                # all points NaN
        gu.orbit_poses(dict(pred, points=torch.full((1, 2, 4, 6, 3), float("nan"))))
    for bad in (dict(color=torch.zeros(2, 4, 6, 3)), dict(color=torch.zeros(2, 4, 6, dtype=torch.uint8)), dict(color=None)):
        with pytest.raises(ValueError):
            gu.save_rendered_views(bad, "unused_dir")
    assert not os.path.exists("unused_dir")


def test_signatures_of_the_public_functions():
    from g2vlm_amd import g2vlm_utils as gu
    sp = inspect.signature(gu.render_point_cloud).parameters
    assert list(sp) == ["pred_dict", "camera_poses", "intrinsics", "size", "splat_radius", "exclude_view", "background", "mask", "conf_threshold",
                        "edge_rtol", "edge_atol", "filter_nan"]
    assert [sp[k].default for k in list(sp)[1:]] == [None, None, None, 0, None, (0, 0, 0), None, None, None, None, True]
    so = inspect.signature(gu.orbit_poses).parameters
    assert list(so) == ["pred_dict", "frames", "mask"] and so["frames"].default == 36 and so["mask"].default is None
    ss = inspect.signature(gu.save_rendered_views).parameters
    assert list(ss) == ["render", "directory", "prefix"] and ss["prefix"].default == "view"


def test_save_rendered_views_writes_pngs_that_decode_to_the_bytes(tmp_path):
    import torch
    from PIL import Image
    from g2vlm_amd import g2vlm_utils as gu
    color = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (3, 5, 7, 3), dtype=np.uint8))
    paths = gu.save_rendered_views(dict(color=color), str(tmp_path / "out"), prefix="orbit")
    assert [os.path.basename(p) for p in paths] == ["orbit_000.png", "orbit_001.png", "orbit_002.png"]
    for p, want in zip(paths, color.numpy()):
        assert np.array_equal(np.asarray(Image.open(p).convert("RGB")), want)


def test_inference_recon_has_the_render_flags_off_by_default():
    import inference_recon
    a = inference_recon.parser.parse_args([])
    assert a.render_dir is None and a.render_orbit is None and a.render_radius == 1 and a.render_size is None
    b = inference_recon.parser.parse_args(["--render-dir", "out", "--render-orbit", "4", "--render-radius", "2", "--render-size", "30", "40",
                                           "--min-views", "1"])
    assert (b.render_dir, b.render_orbit, b.render_radius, b.render_size, b.min_views) == ("out", 4, 2, [30, 40], 1)
    for flag in ("--render-dir", "--render-orbit", "--render-radius", "--render-size"):
        assert flag in inference_recon.__doc__
    for bad in (["--render-orbit", "4"], ["--render-dir", "out", "--render-orbit", "0"], ["--render-dir", "out", "--render-radius", "9"]):
        with pytest.raises(SystemExit):                                                            # refused before the model is loaded
            inference_recon.main(["--image_folder", HERE] + bad)


def scene_pred(s):
    import torch
    return dict(points=torch.from_numpy(s["points"])[None], local_points=torch.from_numpy(s["local"])[None],
                camera_poses=torch.from_numpy(s["poses"])[None])


def test_orbit_poses_on_the_synthetic_scene():
    import torch
    from g2vlm_amd import g2vlm_utils as gu
    s = rc.scene(4, 37, 70)
    mask = rc.random_mask((4, 37, 70), 7)
    for m in (None, torch.from_numpy(mask), torch.from_numpy(mask).bool()):
        out = gu.orbit_poses(scene_pred(s), frames=12, mask=m)
        assert out.dtype == torch.float32 and tuple(out.shape) == (12, 4, 4) and not out.is_cuda
        T = out.numpy().astype(np.float64)
        keep = np.isfinite(s["points"]).all(-1) & (True if m is None else mask != 0)
        c = np.median(s["points"][keep].astype(np.float64), axis=0)
        cam = s["poses"].astype(np.float64)
        up = -cam[:, :3, 1].mean(0)
        up /= np.linalg.norm(up)
        assert up[2] > 0.9                                                                          # the scene's cameras stand upright: z is up
        for k in range(12):
            R, pos = T[k, :3, :3], T[k, :3, 3]
            assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(R) - 1) <= 1e-6 and T[k, 3].tolist() == [0, 0, 0, 1]
            to_c = (c - pos) / np.linalg.norm(c - pos)
            assert np.abs(R[:, 2] - to_c).max() <= 1e-6                                             # forward points at c
            assert R[:, 1] @ up < 0 and abs(R[:, 0] @ up) <= 1e-6                                   # down points down, right is level
        off = T[:, :3, 3] - c
        along, perp = off @ up, off - (off @ up)[:, None] * up
        coff = cam[:, :3, 3] - c
        cperp = coff - (coff @ up)[:, None] * up
        assert np.abs(along - (coff @ up).mean()).max() <= 1e-5                                     # one height: the cameras' mean
        assert np.abs(np.linalg.norm(perp, axis=1) - np.linalg.norm(cperp, axis=1).mean()).max() <= 1e-5   # one radius: the cameras' mean
        e1 = cperp[0] / np.linalg.norm(cperp[0])
        assert np.abs(perp[0] / np.linalg.norm(perp[0]) - e1).max() <= 1e-6                         # frame 0 at camera 0's azimuth
        az = np.arctan2(perp @ np.cross(up, e1), perp @ e1)
        assert np.abs(np.exp(1j * az) - np.exp(2j * np.pi * np.arange(12) / 12)).max() <= 1e-5      # equal steps, counter-clockwise about up
    assert tuple(gu.orbit_poses(scene_pred(s), frames=1).shape) == (1, 4, 4)


# ------------------------------------------------------------------------------------------------ 3. the rule
@pytest.fixture(scope="module")
def evaluated():
    """(4,37,70) -> 3 targets of 37 x 70, radius 1: scene, colours, targets, the rule in fp32 and in fp64"""
    s = rc.scene(4, 37, 70)
    colors = rc.scene_colors(4, 37, 70)
    poses, K = rc.targets(s, 3, 37, 70)
    a = (s["points"], colors, None, poses, K, None, 37, 70, 1, 0x204060)
    return s, colors, poses, K, rc.rule(*a, dtype=np.float32), rc.rule(*a, dtype=np.float64)


def test_fp32_equals_fp64_outside_the_near_threshold_set(evaluated):
    _, _, _, _, r32, r64 = evaluated
    near = r64["near"]
    differ = r32["index"] != r64["index"]
    print(f"near-threshold share {near.mean():.4%}; index differs on {int(differ.sum())} target pixels, {int((differ & ~near).sum())} outside near")
    assert near.mean() <= 0.05 and (r64["index"] >= 0).mean() > 0.5
    assert np.array_equal(r32["index"][~near], r64["index"][~near])
    ok = ~near & (r64["index"] >= 0)
    assert np.abs(r32["depth"][ok] - r64["depth"][ok]).max() <= 1e-5 * r64["depth"][ok].max()
    assert np.array_equal(r32["color"], r64["color"]) or differ.any()


def test_the_rule_equals_a_point_by_point_loop():
    s = rc.scene(2, 5, 7, seed=3)
    mask = rc.random_mask((2, 5, 7), 11)
    poses, K = rc.targets(s, 2, 6, 8)
    for m, skip, radius in ((None, None, 0), (mask, None, 1), (None, [1, 0], 2), (mask, [0, -1], 8)):
        r64 = rc.rule(s["points"], None, m, poses, K, skip, 6, 8, radius, 0, dtype=np.float64)
        depth, index = rc.brute(s["points"], m, poses, K, skip, 6, 8, radius)
        assert np.array_equal(r64["index"], index) and np.array_equal(r64["depth"], depth) and (index >= 0).any()
        r32 = rc.rule(s["points"], None, m, poses, K, skip, 6, 8, radius, 0)
        assert np.array_equal(r32["index"][~r64["near"]], index[~r64["near"]])


def test_identity_a_view_rendered_from_its_own_pixels_maps_every_pixel_to_itself():
    """The scene's rays go through pixel centres: u and v of a view's own point sit half a pixel from any border, far beyond fp32
    rounding, so at radius 0 every eligible pixel lands on itself and nothing else does."""
    N, H, W = 4, 37, 70
    s = rc.scene(N, H, W)
    eligible = np.isfinite(s["points"]).all(-1)
    for i in range(N):
        mask = np.zeros((N, H, W), np.uint8)
        mask[i] = 1
        r = rc.rule(s["points"], None, mask, s["poses"][i:i + 1], s["K"][i:i + 1], None, H, W, 0, 0)
        own = i * H * W + np.arange(H * W).reshape(H, W)
        assert np.array_equal(r["index"][0], np.where(eligible[i], own, -1))
        assert int((r["index"][0] == own).sum()) == int(eligible[i].sum()) == int(r["landed"][0]) > 0.5 * H * W
        # the depth that comes back is the view's own local depth up to the rounding of the round trip through world coordinates
        z = s["local"][i, ..., 2]
        assert np.abs(r["depth"][0][eligible[i]] - z[eligible[i]]).max() <= 1e-5 * np.nanmax(z)


NOISE, FLYING = 0.002, 0.02                                  # consistency_check.scene's defaults, restated: the margin below hangs on them


def test_occlusion_no_rendered_depth_lies_behind_the_views_own_surface():
    """Leave-one-out on the floor-and-sphere scene with the planted flying pixels left out: wherever target view j has a depth of
    its own and a rendered one, the rendered depth - the nearest of the other views' points that cover the pixel - does not lie
    behind j's own surface by more than MARGIN.  A z-buffer that let the floor behind the sphere show through would fail by
    tens of per cent (the sphere's radius, 0.8, against depths of about 4).
    MARGIN: both depths carry the scene's multiplicative noise, sigma = NOISE each, so their ratio has sigma sqrt(2) NOISE; six
    sigma of that.  On top of it the rendered point need not be the surface point at this pixel's centre but any point within
    the splat's reach, radius + 1 pixels of the target in each direction; SLOPE bounds the relative change of depth per pixel of
    the target over the scene's surfaces, measured below on the target's own noise-free neighbours (its median is asserted to
    be what the geometry gives, a few per cent at this resolution).  The flying pixels (a share FLYING, pulled 10 - 50 % toward
    the camera) are left out on both sides through s["flying"]: as sources they would only make rendered depths smaller, as
    the target's own depth they are wrong by construction."""
    N, H, W, radius = 4, 37, 70, 2
    s = rc.scene(N, H, W, flying=FLYING, noise=NOISE)
    clean = rc.scene(N, H, W, flying=0.0, noise=0.0)
    mask = (~s["flying"]).astype(np.uint8)
    r = rc.rule(s["points"], None, mask, s["poses"], s["K"], list(range(N)), H, W, radius, 0)
    checked = 0
    for j in range(N):
        z = clean["local"][j, ..., 2].astype(np.float64)
        own = s["local"][j, ..., 2].astype(np.float64)
        # the largest relative step of the clean depth to a neighbour within reach, per pixel; NaN neighbours (sky) count as none
        step = np.zeros((H, W))
        reach = radius + 1
        pad = np.pad(z, reach, constant_values=np.nan)
        for dy in range(-reach, reach + 1):
            for dx in range(-reach, reach + 1):
                nb = pad[reach + dy:reach + dy + H, reach + dx:reach + dx + W]
                step = np.fmax(step, np.where(np.isfinite(nb), (nb - z) / z, 0.0))
        margin = 6 * np.sqrt(2) * NOISE + step
        both = (r["index"][j] >= 0) & np.isfinite(own) & ~s["flying"][j]
        excess = r["depth"][j].astype(np.float64) / own - 1.0
        assert z[H // 2, W // 2] < np.nanmax(z) - 0.5 and both.sum() > 0.5 * H * W                  # the sphere at the centre, floor behind it
        print(f"target {j}: {int(both.sum())} pixels with both depths, largest excess {np.nanmax(excess[both]):.4f}, "
              f"largest excess over the margin {np.nanmax((excess - margin)[both]):.4f}")
        assert (excess[both] <= margin[both]).all()
        checked += int(both.sum())
    assert checked > 0.6 * N * H * W


def hand(points, OH, OW, K=None, pose=None):
    """one source view of 1 x len(points) pixels, one target with the identity pose; K defaults to fx = fy = 1, cx = cy = 0: u = x / z"""
    p = np.asarray(points, np.float32).reshape(1, 1, -1, 3)
    Km = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32) if K is None else np.asarray(K, np.float32)
    pm = np.eye(4, dtype=np.float32) if pose is None else np.asarray(pose, np.float32)
    return p, pm[None], Km[None]


def test_the_special_cases_give_what_the_rule_text_says():
    f = np.float32
    down = lambda x: np.nextafter(f(x), f(-np.inf))  # noqa: E731
    OH, OW = 3, 5
    # u == OW and v == OH are outside, one ulp below is inside; u = 0 and -0.0 are inside
    pts = [(OW, 0.5, 1), (down(OW), 0.5, 1), (0.5, OH, 1), (0.5, down(OH), 1), (0.0, 1.5, 1), (-0.0, 2.5, 1), (down(0.0), 1.5, 1)]
    p, pose, K = hand(pts, OH, OW)
    r = rc.rule(p, None, None, pose, K, None, OH, OW, 0, 0)
    want = np.full((OH, OW), -1)
    want[0, 4], want[2, 0], want[1, 0] = 1, 3, 4
    assert np.array_equal(r["index"][0], want) and r["landed"][0] == 4                               # points 1, 3, 4 and 5 land
    assert r["index"][0, 2, 0] == 3 and r["depth"][0, 2, 0] == 1.0                                  # 5 meets 3 there at an equal depth: the lower index
    # q2 = 0, negative, +inf, NaN or inf coordinates: nothing lands; a positive denormal depth lands with its bits
    tiny = np.frombuffer(np.uint32(5).tobytes(), np.float32)[0]
    p, pose, K = hand([(0, 0, 0), (0, 0, -1), (0, 0, np.inf), (np.nan, 0, 1), (0, np.inf, 1), (0, 0, tiny)], 1, 1)
    r = rc.rule(p, None, None, pose, K, None, 1, 1, 0, 0)
    assert r["index"].tolist() == [[[5]]] and r["depth"].view(np.uint32).tolist() == [[[5]]] and r["landed"][0] == 1
    # q2 = +inf from finite coordinates (an overflowing sum), with q0 = 0 so that u = 0 would be inside: the finite test refuses it
    p, pose, K = hand([(0, 0, 3e38)], 1, 1, pose=np.diag([1, 1, 2, 1]))
    assert rc.rule(p, None, None, pose, K, None, 1, 1, 0, 0)["index"].tolist() == [[[-1]]]
    # a NaN in a target's K or pose: that view is background / 0 / -1 as a whole; skip out of range skips nobody
    s = rc.scene(2, 5, 7)
    colors = rc.scene_colors(2, 5, 7)
    poses, K = rc.targets(s, 3, 5, 7)
    K[1, 0, 2] = np.nan
    poses[2, 1, 3] = np.nan
    r = rc.rule(s["points"], colors, None, poses, K, [7, -1, 0], 5, 7, 1, 0xFF8001)
    assert (r["index"][1:] == -1).all() and (r["depth"][1:] == 0).all() and (r["color"][1:] == [255, 128, 1]).all() and (r["index"][0] >= 0).any()
    same = rc.rule(s["points"], colors, None, poses, K, None, 5, 7, 1, 0xFF8001)
    assert np.array_equal(r["index"][0], same["index"][0])
    # bit-identical q2 on one target pixel: the lower index wins, whatever the order of the points
    p, pose, K = hand([(0.9, 0.5, 2), (0.5, 0.5, 1), (0.2, 0.2, 1), (0.7, 0.1, 1.5)], 1, 1)
    assert rc.rule(p, None, None, pose, K, None, 1, 1, 0, 0)["index"].tolist() == [[[1]]]
    # radius 8 centred on each corner of a 20 x 30 image: a clipped 9 x 9 square per corner
    OH, OW = 20, 30
    p, pose, K = hand([(0.5, 0.5, 1), (OW - 0.5, 0.5, 1), (0.5, OH - 0.5, 1), (OW - 0.5, OH - 0.5, 1)], OH, OW)
    r = rc.rule(p, None, None, pose, K, None, OH, OW, 8, 0)
    want = np.full((OH, OW), -1)
    want[:9, :9], want[:9, -9:], want[-9:, :9], want[-9:, -9:] = 0, 1, 2, 3
    assert np.array_equal(r["index"][0], want)
    # colours: the PLY export's bytes (clipped, truncated), the background elsewhere
    c = np.array([-0.5, 0.0, 0.5, 0.999, 1.0, 7.0], np.float32)
    assert rc.colour_bytes(c).tolist() == [0, 0, 127, 254, 255, 255]
