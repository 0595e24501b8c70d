"""CPU (no GPU): the multi-view consistency filter (csrc/consistency.hip, g2vlm_utils.multiview_consistency / point_cloud_mask /
save_point_cloud_masked), in the style of tests/test_cloud_cpu.py.

1. The C ABI: the entry point and its workspace query are exported, declared and bound; every argument error comes back as -22
   before anything touches a device.
2. The public functions refuse bad arguments before any launch; the inference_recon flags.
3. The rule of tests/consistency_check.py - what the kernel is held to on the GPU - on the synthetic scene: fp32 against fp64
   outside the near-threshold set, what the filter removes and keeps, and the special cases."""
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

import consistency_check as cc  # noqa: E402
from g2vlm_amd import hip  # noqa: E402

NAMES = ("points", "local", "mask", "poses", "K", "N", "H", "W", "depth_rtol", "min_agree", "max_in_front", "agree", "in_front", "pairs",
         "mask_out", "workspace", "workspace_bytes", "stream")


# ------------------------------------------------------------------------------------------------ 1. the C ABI
@pytest.fixture(scope="module")
def lib():
    from g2vlm_amd import build
    lib = C.CDLL(build.build())
    for name in ("g2v_cloud_consistency", "g2v_cloud_consistency_workspace"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = hip._SIGS[name]
    return lib


def test_library_exports_and_declares_the_entry_points(lib):
    from g2vlm_amd import build
    hdr = open(os.path.join(ROOT, "include", "g2vlm_hip.h")).read()
    name = "g2v_cloud_consistency"
    assert hasattr(lib, name) and name in hip.EXPORTS and name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, re.S).group(1)
    assert len(decl.split(",")) == len(hip._SIGS[name][0]) == len(NAMES)
    assert [d.split()[-1].lstrip("*") for d in decl.split(",")] == list(NAMES)
    q = name + "_workspace"
    assert hasattr(lib, q) and q in hip.EXPORTS
    decl = re.search(r"\bint64_t %s\((.*?)\);" % q, hdr, re.S).group(1)
    assert len(decl.split(",")) == len(hip._SIGS[q][0]) == 3 and hip._SIGS[q][1] is C.c_int64
    assert "consistency.hip" in build.SOURCES and "consistency.hip" not in build.RESOURCE_AUDIT
    assert list(inspect.signature(hip.cloud_consistency).parameters)[:9] == ["points", "local", "mask", "poses", "K", "depth_rtol", "min_agree",
                                                                             "max_in_front", "pairs"]
    assert lib.g2v_version() == 1


def call(lib, **kw):
    """A valid argument set (no pointer is dereferenced: every call below is refused before any launch), with overrides."""
    a = dict(points=16, local=16, mask=16, poses=16, K=16, N=3, H=37, W=70, depth_rtol=0.03, min_agree=1, max_in_front=0, agree=16,
             in_front=16, pairs=16, mask_out=16, workspace=16, workspace_bytes=1 << 20, stream=None)
    a.update(kw)
    return lib.g2v_cloud_consistency(*[a[k] for k in NAMES])


BAD = [dict(N=0), dict(N=-1), dict(H=0), dict(W=-1), dict(N=4, H=32768, W=32768), dict(N=257, H=2, W=3), dict(points=None), dict(local=None),
       dict(poses=None), dict(K=None), dict(workspace=None), dict(workspace_bytes=0), dict(workspace_bytes=4 * 3 * 37 * 70 - 1),
       dict(points=18), dict(local=17), dict(poses=18), dict(K=22), dict(workspace=18), dict(pairs=18), dict(depth_rtol=-0.01),
       dict(depth_rtol=float("nan")), dict(depth_rtol=-float("inf")), dict(agree=None, in_front=None, pairs=None, mask_out=None),
       dict(N=1, H=8 * 65536, W=1), dict(N=1, H=8 * 65535 + 1, W=1, workspace_bytes=1 << 30)]


@pytest.mark.parametrize("bad", BAD)
def test_argument_errors_return_einval_without_a_device(lib, bad):
    assert call(lib, **bad) == -22


def test_the_workspace_query(lib):
    ws = lib.g2v_cloud_consistency_workspace
    for bad in ((0, 5, 5), (3, 0, 5), (3, 5, -1), (4, 32768, 32768), (257, 2, 3), (1, 8 * 65535 + 1, 1), (1, 8 * 65536, 1), (2, 2 ** 31 - 1, 1)):
        assert ws(*bad) == 0                                                                       # 0 for every shape the entry point refuses
    assert ws(1, 8 * 65535, 1) == 4 * 8 * 65535                                                     # the most rows a launch covers
    # one fp32 depth per pixel
    assert ws(3, 37, 70) == 4 * 3 * 37 * 70 and ws(1, 1, 1) == 4 and ws(256, 2, 3) == 4 * 256 * 6 and ws(32, 518, 518) == 4 * 32 * 518 * 518


# ------------------------------------------------------------------------------------------------ 2. the public surface
def test_public_functions_refuse_bad_arguments_before_any_launch(monkeypatch):
    import torch
    import g2vlm_utils as top
    from g2vlm_amd import g2vlm_utils as gu
    for name in ("multiview_consistency", "save_point_cloud_masked", "point_cloud_mask"):
        assert getattr(top, name) is getattr(gu, name) and name in top.__all__
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("a refused call reached the library"))
    pred = dict(points=torch.zeros(1, 2, 4, 6, 3), local_points=torch.ones(1, 2, 4, 6, 3), conf=None, images=torch.zeros(1, 2, 3, 4, 6),
                camera_poses=torch.eye(4).repeat(1, 2, 1, 1))
    for kw in (dict(min_views=0), dict(min_views=256), dict(min_views=1.0), dict(min_views=True), dict(min_views=-1), dict(max_in_front=-1),
               dict(max_in_front=256), dict(max_in_front=0.5), dict(min_views=1, depth_rtol=-0.1), dict(min_views=1, depth_rtol=float("nan")),
               dict(max_in_front=0, depth_rtol=float("inf")), dict(min_views=1, intrinsics=torch.zeros(3, 3, 3)),
               dict(min_views=1, intrinsics=torch.zeros(1, 2, 3, 4)), dict(min_views=1, intrinsics=np.zeros((2, 3, 3))),
               dict(min_views=1, edge_rtol=-1.0), dict(min_views=1, conf_threshold=0.5)):
        with pytest.raises(ValueError):
            gu.point_cloud_mask(pred, **kw)
    for kw in (dict(depth_rtol=-1.0), dict(depth_rtol=float("nan")), dict(depth_rtol="x"), dict(intrinsics=torch.zeros(1, 3, 3, 3)),
               dict(mask=torch.ones(2, 4, 5, dtype=torch.bool)), dict(mask=np.ones((2, 4, 6), bool)), dict(edge_atol=-1.0)):
        with pytest.raises(ValueError):
            gu.multiview_consistency(pred, **kw)
    for poses in (None, torch.eye(4).repeat(2, 1, 1), torch.eye(4).repeat(1, 3, 1, 1), torch.zeros(1, 2, 3, 4)):
        bad = dict(pred, camera_poses=poses)
        if poses is None:
            del bad["camera_poses"]
        with pytest.raises(ValueError, match="camera_poses"):
            gu.multiview_consistency(bad)
        with pytest.raises(ValueError, match="camera_poses"):
            gu.point_cloud_mask(bad, min_views=1)
    big = dict(points=torch.zeros(1, 257, 1, 2, 3), local_points=torch.ones(1, 257, 1, 2, 3), camera_poses=torch.eye(4).repeat(1, 257, 1, 1))
    with pytest.raises(ValueError, match="256"):
        gu.multiview_consistency(big)
    for kw in (dict(mask=torch.ones(2, 4, 5, dtype=torch.bool)), dict(mask=torch.ones(2, 4, 6)), dict(mask=None),
               dict(mask=torch.ones(2, 4, 6, dtype=torch.bool), voxel_size=0.0), dict(mask=torch.ones(2, 4, 6, dtype=torch.bool), voxel_size=0.1, min_points=0)):
        with pytest.raises(ValueError):
            gu.save_point_cloud_masked(pred, "unused.ply", **kw)
    assert not os.path.exists("unused.ply")


def test_signatures_of_the_public_functions():
    from g2vlm_amd import g2vlm_utils as gu
    sp = inspect.signature(gu.point_cloud_mask).parameters
    assert list(sp) == ["pred_dict", "conf_threshold", "edge_rtol", "edge_atol", "filter_nan", "min_views", "max_in_front", "depth_rtol", "intrinsics"]
    assert sp["min_views"].default is None and sp["max_in_front"].default is None and sp["depth_rtol"].default == 0.03
    assert sp["intrinsics"].default is None
    assert list(inspect.signature(gu.multiview_consistency).parameters) == ["pred_dict", "depth_rtol", "intrinsics", "conf_threshold", "edge_rtol",
                                                                             "edge_atol", "filter_nan", "mask"]
    assert inspect.signature(gu.multiview_consistency).parameters["depth_rtol"].default == 0.03
    assert list(inspect.signature(gu.save_point_cloud_masked).parameters) == ["pred_dict", "save_path", "mask", "verbose", "voxel_size",
                                                                               "voxel_origin", "min_points"]


def test_inference_recon_has_the_consistency_flags_off_by_default():
    import inference_recon
    a = inference_recon.parser.parse_args([])
    assert a.min_views is None and a.max_in_front is None and a.consistency_rtol == 0.03
    b = inference_recon.parser.parse_args(["--min-views", "2", "--max-in-front", "0", "--consistency-rtol", "0.05", "--voxel-size", "0.1"])
    assert (b.min_views, b.max_in_front, b.consistency_rtol, b.voxel_size) == (2, 0, 0.05, 0.1)


# ------------------------------------------------------------------------------------------------ 3. the rule
@pytest.fixture(scope="module", params=[(4, 37, 70), (8, 56, 70)], ids=lambda s: "x".join(map(str, s)))
def evaluated(request):
    s = cc.scene(*request.param)
    a = (s["points"], s["local"], s["poses"], s["K"], None, 0.03)
    return s, cc.rule(*a, dtype=np.float32, min_agree=1, max_in_front=0), cc.rule(*a, dtype=np.float64, min_agree=1, max_in_front=0)


def test_fp32_equals_fp64_outside_the_near_threshold_set(evaluated):
    _, r32, r64 = evaluated
    near = r64["near"]
    print(f"near-threshold share {near.mean():.4%}; counts differ on {int(((r32['agree'] != r64['agree']) | (r32['in_front'] != r64['in_front'])).sum())} pixels")
    assert near.mean() <= 0.01
    assert np.array_equal(r32["agree"][~near], r64["agree"][~near]) and np.array_equal(r32["in_front"][~near], r64["in_front"][~near])


def test_the_filter_drops_the_flying_pixels_and_keeps_the_scene(evaluated):
    s, r32, _ = evaluated
    fly, kept = s["flying"], r32["mask_out"]
    print(f"flying {int(fly.sum())}, kept of them {int((kept & fly).sum())}; clean kept {(kept & ~fly).sum() / (~fly).sum():.3f}")
    assert fly.sum() > 100 and not (kept & fly).any()
    assert (kept & ~fly).sum() >= 0.75 * (~fly).sum()
    assert np.array_equal(kept, cc.mask_out(r32, 1, 0))


def test_pairs_are_the_sums_of_the_per_pixel_classes(evaluated):
    _, r32, _ = evaluated
    n = r32["pairs"].shape[0]
    assert np.array_equal(r32["pairs"][..., 0], r32["agree_in"].sum((2, 3))) and np.array_equal(r32["pairs"][..., 1], r32["front_in"].sum((2, 3)))
    assert (r32["pairs"][np.arange(n), np.arange(n)] == 0).all() and r32["pairs"].sum() > 0
    assert np.array_equal(r32["pairs"][..., 0].sum(1), r32["agree"].astype(np.int64).sum((1, 2)))
    assert np.array_equal(r32["pairs"][..., 1].sum(1), r32["in_front"].astype(np.int64).sum((1, 2)))


def test_one_view_gives_zeros_and_a_copied_view_agrees_with_itself():
    s = cc.scene(1, 9, 11)
    r = cc.rule(s["points"], s["local"], s["poses"], s["K"], None, 0.03)
    assert not r["agree"].any() and not r["in_front"].any() and r["pairs"].tolist() == [[[0, 0]]] and r["eligible"].all()
    two = {k: np.concatenate([v, v]) for k, v in cc.scene(1, 37, 70).items()}
    mask = cc.random_mask((1, 37, 70), 3)
    mask = np.concatenate([mask, mask])
    for m in (None, mask):
        r = cc.rule(two["points"], two["local"], two["poses"], two["K"], m, 0.03)
        valid = np.isfinite(two["points"]).all(-1) & (two["local"][..., 2] > 0) & (True if m is None else m != 0)
        # a pixel projects to its own centre up to rounding, far from the pixel's border: the lookup is its own depth
        assert np.array_equal(r["agree"], valid.astype(np.uint8)) and not r["in_front"].any() and valid.sum() > 2000


def test_the_contraction_scenes_tell_the_rule_from_its_fused_forms():
    """what the GPU tests rely on, checked where the scenes are built: >= 32 pixels per fused form, in both scenes"""
    s, picked = cc.fma_scene()
    assert picked.sum() >= 32 and not picked[1:].any()                                             # the pixels of view 0
    s, picked = cc.fma_pose_scene()
    assert tuple(picked) == cc.FUSED_Q and all(p.sum() >= 32 for p in picked.values()), {k: int(p.sum()) for k, p in picked.items()}
    assert not np.allclose(s["poses"][1, :3, :3], np.round(s["poses"][1, :3, :3])) and np.abs(s["poses"][1, :3, :3]).min() > 0.05   # no axis-aligned entry
    r = cc.rule(s["points"], s["local"], s["poses"], s["K"], None, 0.25)
    assert r["eligible"][0].all() and 0 < r["agree"][0].sum() < r["eligible"][0].sum() and not r["in_front"].any()
