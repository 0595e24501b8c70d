"""GPU, end to end: surface normals of a recon result through the public functions - estimate_normals, view_angle_mask,
save_point_cloud_normals, save_normal_maps - on a pred_dict that holds the synthetic floor-and-sphere scene of
tests/normals_check.py (what `recon` returns, with known geometry), against the numpy rule byte for byte; the normals shown through
render_point_cloud and save_point_cloud_masked, which did not change; the exports that existed before write the same bytes whether or
not the normals code has run; inference_recon's flags on the tiny synthetic model."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import normals_check as nc  # noqa: E402
from render_check import colour_bytes  # noqa: E402
from g2vlm_amd.g2vlm_utils import (estimate_normals, point_cloud_mask, render_point_cloud, save_normal_maps, save_ply_visualization,  # noqa: E402
                                   save_point_cloud, save_point_cloud_masked, save_point_cloud_normals, view_angle_mask)

pytestmark = pytest.mark.gpu
SHAPE = (3, 37, 70)
PLAIN_DTYPE = np.dtype([("p", "<f4", (3,)), ("c", "u1", (3,))])


@pytest.fixture(scope="module")
def scene():
    s = nc.scene(*SHAPE, seed=4)
    s["images"] = nc.scene_colors(*SHAPE, seed=4)
    return s


@pytest.fixture(scope="module")
def pred(scene):
    def t(a):
        return torch.from_numpy(a).cuda()[None]
    return dict(points=t(scene["points"]), local_points=t(scene["local"]), images=t(scene["images"]), camera_poses=t(scene["poses"]), conf=None)


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def equal(out, want, colors=False):
    assert set(out) == {"normals", "valid", "cos_view"} | ({"images"} if colors else set()) and all(v.is_cuda for v in out.values())
    assert (out["normals"].dtype, out["valid"].dtype, out["cos_view"].dtype) == (torch.float32, torch.bool, torch.float32)
    assert tuple(out["normals"].shape) == SHAPE + (3,) and tuple(out["valid"].shape) == SHAPE and tuple(out["cos_view"].shape) == SHAPE
    assert np.array_equal(bits(out["normals"].cpu().numpy()), bits(want["normals"]))
    assert np.array_equal(out["valid"].cpu().numpy(), want["valid"] != 0)
    assert np.array_equal(bits(out["cos_view"].cpu().numpy()), bits(want["cos_view"]))
    if colors:
        assert tuple(out["images"].shape) == (1, SHAPE[0], 3) + SHAPE[1:] and out["images"].dtype == torch.float32
        assert np.array_equal(bits(out["images"][0].cpu().numpy()), bits(want["colors"]))


def parse(path):
    """(header, the 27-byte records) of a PLY with normals"""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    m = int(lines[2].split()[-1])
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and lines[2].startswith("element vertex ")
    assert [ln.split()[-1] for ln in lines[3:12]] == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"] and len(body) == 27 * m
    return head, np.frombuffer(body, nc.RECORD_DTYPE)


def test_estimate_normals_in_both_frames_equals_the_rule(pred, scene):
    snap = {k: v.clone() for k, v in pred.items() if torch.is_tensor(v)}
    keep = point_cloud_mask(pred, edge_rtol=0.03).cpu().numpy()
    assert 0 < keep.sum() < keep.size
    world = nc.rule(scene["points"], keep, scene["poses"])
    assert 0 < world["valid"].sum() < keep.sum()
    equal(estimate_normals(pred), world)                                                            # frame="world", edge_rtol = 0.03: the defaults
    equal(estimate_normals(pred, colors=True), world, colors=True)
    equal(estimate_normals(pred, frame="camera", colors=True), nc.rule(scene["local"], keep, None), colors=True)
    median, exact = nc.edge_limits(scene["points"], keep, scene["poses"], 2)
    equal(estimate_normals(pred, step=2, max_edge=median), nc.rule(scene["points"], keep, scene["poses"], 2, median))
    # other filters and an explicit mask in its three forms
    for kw in (dict(edge_rtol=None), dict(edge_rtol=None, filter_nan=False), dict(edge_rtol=0.1, edge_atol=0.5)):
        m = point_cloud_mask(pred, **kw).cpu().numpy()
        equal(estimate_normals(pred, **kw), nc.rule(scene["points"], m, scene["poses"]))
    mine = nc.random_mask(SHAPE, 8, keep=0.7)
    want = nc.rule(scene["local"], mine, None, 1)
    t = torch.from_numpy(mine).cuda()
    for mask in (t, t.view(torch.bool), t[None]):
        equal(estimate_normals(pred, frame="camera", mask=mask), want)
    none = estimate_normals(pred, mask=torch.zeros_like(t))
    assert not none["valid"].any() and not none["normals"].any()
    assert all(torch.equal(pred[k], v) for k, v in snap.items())                                    # the inputs are untouched


def test_view_angle_mask_equals_the_numpy_statement(pred, scene):
    keep = point_cloud_mask(pred, edge_rtol=0.03).cpu().numpy()
    r = nc.rule(scene["points"], keep, scene["poses"])
    valid = r["valid"] != 0
    for angle in (30, 60.0, 75, 89.9, 90):
        thr = np.float32(np.cos(np.radians(np.float64(angle))))
        got = view_angle_mask(pred, angle)
        assert got.dtype == torch.bool and got.is_cuda and np.array_equal(got.cpu().numpy(), valid & (r["cos_view"] >= thr)), angle
    assert np.array_equal(view_angle_mask(pred, 90).cpu().numpy(), valid)                           # cos_view >= 6e-17: every valid pixel but cos_view == 0
    assert 0 < int(view_angle_mask(pred, 30).sum()) < int(view_angle_mask(pred, 50).sum()) < int(valid.sum())
    # a threshold that equals some pixel's cos_view exactly: `>=` keeps that pixel
    hit = None
    for c in np.unique(r["cos_view"][valid & (r["cos_view"] < 0.99) & (r["cos_view"] > 0.1)])[::7]:
        angle = float(np.degrees(np.arccos(np.float64(c))))
        if np.float32(np.cos(np.radians(angle))) == c:
            hit = (angle, c)
            break
    assert hit is not None
    angle, c = hit
    got = view_angle_mask(pred, angle).cpu().numpy()
    assert np.array_equal(got, valid & (r["cos_view"] >= c)) and got[valid & (r["cos_view"] == c)].all() and (r["cos_view"] == c).any()
    # the camera frame and an explicit mask
    cam = nc.rule(scene["local"], keep, None, 2)
    thr = np.float32(np.cos(np.radians(70.0)))
    assert np.array_equal(view_angle_mask(pred, 70, step=2, frame="camera").cpu().numpy(), (cam["valid"] != 0) & (cam["cos_view"] >= thr))
    assert np.array_equal(view_angle_mask(pred, 70, step=2, frame="camera", mask=torch.from_numpy(keep).cuda()).cpu().numpy(),
                          (cam["valid"] != 0) & (cam["cos_view"] >= thr))


def test_save_point_cloud_normals_writes_the_rules_records(pred, scene, tmp_path, capsys):
    keep = point_cloud_mask(pred, edge_rtol=0.03)
    k = keep.cpu().numpy()
    r = nc.rule(scene["points"], k, scene["poses"])
    path = str(tmp_path / "sub" / "normals.ply")
    info = save_point_cloud_normals(pred, path)
    want = nc.records(scene["points"], r["normals"], scene["images"], k)
    assert info == dict(num_points=len(want), counts=k.reshape(SHAPE[0], -1).sum(1).tolist(), num_normals=int((r["valid"] != 0).sum()))
    assert "normals.ply" in capsys.readouterr().out
    head, rec = parse(path)
    assert np.array_equal(rec.view(np.uint8).reshape(-1, 27), want)
    assert (rec["n"][~(r["valid"][k != 0] != 0)] == 0).all() and (r["valid"][k != 0] == 0).any()    # kept without a valid normal: a zero normal
    # with the same mask, x y z r g b are save_point_cloud_masked's file
    cloud = str(tmp_path / "cloud.ply")
    save_point_cloud_masked(pred, cloud, keep, verbose=False)
    plain = np.frombuffer(open(cloud, "rb").read().split(b"end_header\n", 1)[1], PLAIN_DTYPE)
    assert np.array_equal(plain["p"].view(np.int32), rec["p"].view(np.int32)) and np.array_equal(plain["c"], rec["c"])
    # max_view_angle drops the pixels without a normal along with the grazing ones; an explicit mask, a step and a limit, quietly
    quiet = str(tmp_path / "quiet.ply")
    mine = nc.random_mask(SHAPE, 8, keep=0.7)
    median, _ = nc.edge_limits(scene["points"], mine, scene["poses"], 2)
    r2 = nc.rule(scene["points"], mine, scene["poses"], 2, median)
    sel = (r2["valid"] != 0) & (r2["cos_view"] >= np.float32(np.cos(np.radians(60.0))))
    info = save_point_cloud_normals(pred, quiet, step=2, max_edge=median, max_view_angle=60, mask=torch.from_numpy(mine).cuda(), verbose=False)
    assert capsys.readouterr().out == "" and info["num_points"] == info["num_normals"] == int(sel.sum()) > 0
    assert np.array_equal(parse(quiet)[1].view(np.uint8).reshape(-1, 27), nc.records(scene["points"], r2["normals"], scene["images"], sel))


def test_the_normals_show_through_the_renderer_and_the_cloud_export(pred, scene, tmp_path):
    r = estimate_normals(pred, colors=True)
    shown = dict(pred, images=r["images"])
    out = render_point_cloud(shown, splat_radius=1)
    index = out["index"].cpu().numpy()
    covered = index >= 0
    assert covered.any()
    flat = colour_bytes(np.moveaxis(r["images"][0].cpu().numpy(), 1, -1).reshape(-1, 3))            # [N H W, 3]
    assert np.array_equal(out["color"].cpu().numpy()[covered], flat[index[covered]])
    path = str(tmp_path / "as_colours.ply")
    save_point_cloud_masked(shown, path, r["valid"], verbose=False)
    rec = np.frombuffer(open(path, "rb").read().split(b"end_header\n", 1)[1], PLAIN_DTYPE)
    assert np.array_equal(rec["c"], flat[r["valid"].cpu().numpy().reshape(-1)]) and len(rec) > 0


def test_save_normal_maps_writes_one_png_per_view(pred, scene, tmp_path):
    from PIL import Image
    keep = point_cloud_mask(pred, edge_rtol=0.03).cpu().numpy()
    for kw, pts, poses in ((dict(), scene["local"], None), (dict(frame="world", step=2, prefix="w"), scene["points"], scene["poses"])):
        paths = save_normal_maps(pred, str(tmp_path / "maps"), **kw)
        assert [os.path.basename(p) for p in paths] == [f"{kw.get('prefix', 'normal')}_{i:03d}.png" for i in range(SHAPE[0])]
        want = nc.rule(pts, keep, poses, kw.get("step", 1))
        img = colour_bytes(np.moveaxis(want["colors"], 1, -1))                                      # [N,H,W,3]
        for i, p in enumerate(paths):
            got = np.asarray(Image.open(p))
            assert got.shape == SHAPE[1:] + (3,) and np.array_equal(got, img[i])
            assert (got[want["valid"][i] == 0] == 0).all() and (want["valid"][i] == 0).any()        # black where no normal is valid


def test_the_exports_of_before_write_the_same_bytes(pred, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                              # save_ply_visualization writes results/input_images.png relative to cwd

    def exports(tag):
        save_point_cloud(pred, str(tmp_path / f"cloud_{tag}.ply"), verbose=False)
        save_point_cloud(pred, str(tmp_path / f"atol_{tag}.ply"), edge_rtol=None, edge_atol=0.5, verbose=False)
        save_ply_visualization(pred, str(tmp_path / f"vis_{tag}.ply"), verbose=False)
        return [(tmp_path / f"{name}_{tag}.ply").read_bytes() for name in ("cloud", "atol", "vis")]

    before = exports("before")
    estimate_normals(pred, colors=True)
    view_angle_mask(pred, 60)
    save_point_cloud_normals(pred, str(tmp_path / "normals.ply"), max_edge=0.5, verbose=False)
    save_normal_maps(pred, str(tmp_path / "maps"))
    assert exports("after") == before


def test_inference_recon_with_the_normal_flags(tiny_checkpoint, golden_dir, tmp_path, monkeypatch):
    from PIL import Image
    from safetensors.torch import load_file
    path, _, _ = tiny_checkpoint
    monkeypatch.chdir(tmp_path)
    g = load_file(os.path.join(golden_dir, "recon_real2_dl3dv_2v.safetensors"))
    folder = tmp_path / "frames"
    folder.mkdir()
    for i, name in enumerate(("a_first.png", "b_second.png")):
        Image.fromarray(g["inp.images_u8"][i].permute(1, 2, 0).numpy()).save(folder / name)
    import inference_recon
    args = ["--image_folder", str(folder), "--model_path", path]
    # an absolute edge tolerance nothing exceeds keeps every finite pixel (this checkpoint's depth is noise from pixel to pixel: the
    # relative rule would keep nothing); the PLY of before is save_point_cloud's under the same flag
    pred = inference_recon.main(args + ["--save_path", str(tmp_path / "f.ply"), "--edge-atol", "1e9", "--normals-ply", str(tmp_path / "n.ply"),
                                        "--normal-maps", str(tmp_path / "maps"), "--normal-step", "2", "--max-view-angle", "80"])
    save_point_cloud(pred, str(tmp_path / "fwant.ply"), edge_rtol=None, edge_atol=1e9, verbose=False)
    assert (tmp_path / "f.ply").read_bytes() == (tmp_path / "fwant.ply").read_bytes()
    mask = point_cloud_mask(pred, edge_atol=1e9)
    save_point_cloud_normals(pred, str(tmp_path / "nwant.ply"), step=2, max_view_angle=80, mask=mask, verbose=False)
    assert (tmp_path / "n.ply").read_bytes() == (tmp_path / "nwant.ply").read_bytes() and len(parse(str(tmp_path / "n.ply"))[1]) > 0
    want = save_normal_maps(pred, str(tmp_path / "mwant"), step=2, mask=mask)
    got = sorted((tmp_path / "maps").glob("normal_*.png"))
    assert len(got) == len(want) == 2 and all(a.read_bytes() == open(b, "rb").read() for a, b in zip(got, want))
