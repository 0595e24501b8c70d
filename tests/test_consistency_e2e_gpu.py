"""GPU, end to end: the multi-view consistency filter through the public functions (multiview_consistency, point_cloud_mask
(min_views=..., max_in_front=...), save_point_cloud_masked), on a pred dict built from the synthetic scene of
tests/consistency_check.py, on the tiny synthetic model's recon output, and through inference_recon.main --min-views."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cloud_check  # noqa: E402
import consistency_check as cc  # noqa: E402
import voxel_check  # noqa: E402
from g2vlm_amd import host  # noqa: E402
from g2vlm_amd.g2vlm_utils import (estimate_intrinsics, multiview_consistency, point_cloud_mask, save_point_cloud,  # noqa: E402
                                   save_point_cloud_masked)

pytestmark = pytest.mark.gpu


def scene_pred(n=4, h=37, w=70):
    s = cc.scene(n, h, w)
    rng = np.random.default_rng(1)
    pred = dict(points=torch.from_numpy(s["points"])[None].cuda(), local_points=torch.from_numpy(s["local"])[None].cuda(),
                camera_poses=torch.from_numpy(s["poses"])[None].cuda(), images=torch.from_numpy(rng.random((1, n, 3, h, w), np.float32)).cuda(),
                conf=None)
    return s, pred


def rule_for(pred, base, K, **kw):
    return cc.rule(pred["points"][0].cpu().numpy(), pred["local_points"][0].cpu().numpy(), pred["camera_poses"][0].float().cpu().numpy(),
                   K.reshape(-1, 3, 3).cpu().numpy(), base, 0.03, **kw)


def check_public_functions(pred, edge_rtol):
    """multiview_consistency and point_cloud_mask against the rule evaluated with the K that estimate_intrinsics returned"""
    snap = {k: v.clone() for k, v in pred.items() if torch.is_tensor(v)}
    base = point_cloud_mask(pred, edge_rtol=edge_rtol)
    K = estimate_intrinsics(pred, base)
    out = multiview_consistency(pred, edge_rtol=edge_rtol)
    assert set(out) == {"agree", "in_front", "covisibility", "intrinsics", "mask"} and all(v.is_cuda for v in out.values())
    assert torch.equal(out["intrinsics"].view(torch.int32), K.view(torch.int32)) and torch.equal(out["mask"], base)
    want = rule_for(pred, base.cpu().numpy(), K)
    assert np.array_equal(out["agree"].cpu().numpy(), want["agree"]) and np.array_equal(out["in_front"].cpu().numpy(), want["in_front"])
    assert np.array_equal(out["covisibility"].cpu().numpy(), want["pairs"]) and out["covisibility"].dtype == torch.int32
    for mv, mf in ((1, 0), (2, None), (None, 0)):
        m = point_cloud_mask(pred, edge_rtol=edge_rtol, min_views=mv, max_in_front=mf)
        assert m.dtype == torch.bool and np.array_equal(m.cpu().numpy(), cc.mask_out(want, mv or 0, -1 if mf is None else mf)), (mv, mf)
    explicit = multiview_consistency(pred, intrinsics=K[0], mask=base)                              # the same through the explicit arguments
    assert torch.equal(explicit["agree"], out["agree"]) and torch.equal(explicit["covisibility"], out["covisibility"])
    assert all(torch.equal(pred[k].view(torch.uint8), v.view(torch.uint8)) for k, v in snap.items())
    return want


def test_public_functions_on_the_scene_and_the_exported_file(tmp_path):
    s, pred = scene_pred()
    want = check_public_functions(pred, None)
    keep = cc.mask_out(want, 1, 0)
    mask = point_cloud_mask(pred, min_views=1, max_in_front=0)
    p, c = s["points"].reshape(-1, 3), pred["images"][0].cpu().numpy().transpose(0, 2, 3, 1).reshape(-1, 3)
    host.write_ply_binary(str(tmp_path / "want.ply"), p[keep.reshape(-1)], c[keep.reshape(-1)])
    info = save_point_cloud_masked(pred, str(tmp_path / "got.ply"), mask, verbose=False)
    assert (tmp_path / "got.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()
    assert info["num_points"] == int(keep.sum()) and info["counts"] == keep.reshape(4, -1).sum(1).tolist()
    fly = s["flying"]
    print(f"kept {int(keep.sum())} of {keep.size}; flying {int(fly.sum())}, kept of them {int((keep & fly).sum())}")
    assert fly.sum() > 100 and not (keep & fly).any()                                               # the flying pixels are gone from the file
    # with voxel_size: the voxel export of the same mask (tests/voxel_check.py is what that path is held to)
    v = 0.05
    vox = voxel_check.downsample(s["points"], pred["images"][0].cpu().numpy(), keep, v, voxel_check.default_origin(s["points"], keep, v))
    host.write_ply_records(str(tmp_path / "vox_want.ply"), vox["records"])
    info = save_point_cloud_masked(pred, str(tmp_path / "vox.ply"), mask, verbose=False, voxel_size=v)
    assert (tmp_path / "vox.ply").read_bytes() == (tmp_path / "vox_want.ply").read_bytes() and info["num_input_points"] == int(keep.sum())
    # save_point_cloud still writes what it wrote: it is the masked export of its own mask
    save_point_cloud(pred, str(tmp_path / "a.ply"), verbose=False)
    save_point_cloud_masked(pred, str(tmp_path / "b.ply"), point_cloud_mask(pred, edge_rtol=0.03), verbose=False)
    assert (tmp_path / "a.ply").read_bytes() == (tmp_path / "b.ply").read_bytes()


def test_public_functions_on_the_tiny_models_recon_output(tiny_checkpoint):
    from g2vlm_amd.g2vlm_utils import load_model_and_tokenizer
    from oracle import synth
    path, _, _ = tiny_checkpoint
    model, tokenizer, new_token_ids, _, dino_tf = load_model_and_tokenizer(path)
    pred = model.recon(tokenizer, new_token_ids, dino_tf, synth.synth_images(3, 56, 70, 3))
    assert pred["camera_poses"].shape == (1, 3, 4, 4)
    check_public_functions(pred, None)                                                              # random geometry: equality only


def test_inference_recon_with_min_views(tiny_checkpoint, golden_dir, tmp_path, monkeypatch):
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
    pred = inference_recon.main(["--image_folder", str(folder), "--model_path", path, "--save_path", str(tmp_path / "mv.ply"), "--min-views", "1"])
    base = point_cloud_mask(pred)
    want = rule_for(pred, base.cpu().numpy(), estimate_intrinsics(pred, base))
    keep = cc.mask_out(want, 1, -1).reshape(-1)
    p = pred["points"][0].float().cpu().numpy().reshape(-1, 3)
    c = pred["images"][0].float().cpu().numpy().transpose(0, 2, 3, 1).reshape(-1, 3)
    host.write_ply_binary(str(tmp_path / "want.ply"), p[keep], c[keep])
    assert (tmp_path / "mv.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()
    print(f"--min-views 1 kept {int(keep.sum())} of {keep.size}")
