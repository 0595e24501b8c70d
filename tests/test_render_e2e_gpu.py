"""GPU, end to end: rendering the cloud of what `recon` returns from its own and from new cameras, on the tiny synthetic model with
a confidence head as tests/test_cloud_e2e_gpu.py builds it (the fixture is restated here), through render_point_cloud,
orbit_poses, save_rendered_views and inference_recon.main --render-dir / --render-orbit."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import render_check as rc  # noqa: E402
from g2vlm_amd import hip  # noqa: E402
from g2vlm_amd.g2vlm_utils import (estimate_intrinsics, orbit_poses, point_cloud_mask, render_point_cloud, save_ply_visualization,  # noqa: E402
                                   save_rendered_views)
from oracle import synth  # noqa: E402  checker-side helpers only (synthetic weights)

pytestmark = pytest.mark.gpu
POINT_HEAD_DAMP = 2.0 ** -8                                 # see conf_pred


@pytest.fixture(scope="module")
def conf_pred(tmp_path_factory):
    """recon of two 56 x 70 views by a train_conf_pi3 checkpoint whose point head's output layer is scaled by POINT_HEAD_DAMP:
    tests/test_cloud_e2e_gpu.py::conf_pred, restated.  Undamped, the synthetic depth is independent noise from pixel to pixel and
    the depth-edge rule at rtol 0.03 keeps nothing; damped by 2^-8 it keeps some pixels and drops some."""
    from conftest import write_tiny_checkpoint
    from safetensors.torch import save_file
    from g2vlm_amd.g2vlm_utils import LazySafetensors
    from g2vlm_amd.modeling.g2vlm import (G2VLM, G2VLMConfig, Dinov2WithRegistersConfig, Dinov2WithRegistersModel, Qwen2VLConfig,
                                          Qwen2VLForCausalLM, Qwen2VLVisionConfig, Qwen2VisionTransformerPretrainedModel)
    path = str(tmp_path_factory.mktemp("g2vlm_conf_ckpt_render"))
    dims, sd = write_tiny_checkpoint(path, conf=True)
    sd = dict(sd)
    for k in ("point_head.proj.weight", "point_head.proj.bias"):
        sd[k] = sd[k] * POINT_HEAD_DAMP
    save_file(sd, os.path.join(path, "model.safetensors"))
    llm = Qwen2VLConfig.from_json_file(os.path.join(path, "text_config.json"))
    vit = Qwen2VLVisionConfig.from_json_file(os.path.join(path, "vit_config.json"))
    dino = Dinov2WithRegistersConfig.from_json_file(os.path.join(path, "dino_config.json"))
    cfg = G2VLMConfig(llm_config=llm, vit_config=vit, dino_config=dino, train_conf_pi3=True)
    model = G2VLM(Qwen2VLForCausalLM(llm), Qwen2VisionTransformerPretrainedModel(vit), Dinov2WithRegistersModel(dino), cfg)
    model.load_state_dict(LazySafetensors(os.path.join(path, "model.safetensors")))
    model = model.to("cuda").eval()
    tok = synth.FakeTokenizer(dims["llm"]["vocab"])
    pred = model.recon(tok, tok.new_token_ids, None, synth.synth_images(2, 56, 70, 3))
    assert pred["conf"].shape == (1, 2, 56, 70, 1)
    return pred


def host(pred):
    return (pred["points"][0].float().cpu().numpy(), pred["images"][0].float().cpu().numpy(), pred["camera_poses"][0].float().cpu().numpy())


def equal(out, want):
    assert np.array_equal(out["color"].cpu().numpy(), want["color"])
    assert np.array_equal(out["depth"].cpu().numpy().view(np.int32), want["depth"].view(np.int32))
    assert np.array_equal(out["index"].cpu().numpy(), want["index"])


def test_leave_one_out_rendering_equals_the_rule_and_maps_into_the_mask(conf_pred):
    snap = {k: v.clone() for k, v in conf_pred.items() if torch.is_tensor(v)}
    n, h, w = conf_pred["points"].shape[1:4]
    base = point_cloud_mask(conf_pred, edge_rtol=0.03)
    K = estimate_intrinsics(conf_pred, base)
    points, images, poses = host(conf_pred)
    keep = base.cpu().numpy()

    out = render_point_cloud(conf_pred, exclude_view="self", splat_radius=1, edge_rtol=0.03)
    assert set(out) == {"color", "depth", "index", "intrinsics"} and all(v.is_cuda for v in out.values())
    assert (out["color"].dtype, out["depth"].dtype, out["index"].dtype) == (torch.uint8, torch.float32, torch.int32)
    assert tuple(out["color"].shape) == (n, h, w, 3) and tuple(out["depth"].shape) == tuple(out["index"].shape) == (n, h, w)
    assert torch.equal(out["intrinsics"].view(torch.int32), K[0].view(torch.int32))
    want = rc.rule(points, images, keep, poses, K[0].cpu().numpy(), list(range(n)), h, w, 1, 0)
    equal(out, want)

    # the scene's own cameras with nobody left out: every view sees at least its own kept pixels
    full = render_point_cloud(conf_pred, splat_radius=0, edge_rtol=0.03, background=(9, 8, 7))
    want_full = rc.rule(points, images, keep, poses, K[0].cpu().numpy(), None, h, w, 0, 0x090807)
    equal(full, want_full)
    print(f"kept {int(keep.sum())} of {keep.size}; covered leave-one-out {int((want['index'] >= 0).sum())}, with every view {int((want_full['index'] >= 0).sum())}")
    assert (want_full["index"] >= 0).any()

    # cameras that see the cloud whatever geometry the tiny model's random weights give: a turntable that looks at the cloud's median
    # with a focal length of 4 pixels (half a field of view of more than 80 degrees); target 0 leaves out view 0, target 1 view 1
    orbit = orbit_poses(conf_pred, frames=3, mask=base)
    Kw = torch.tensor([[4.0, 0.0, w / 2], [0.0, 4.0, h / 2], [0.0, 0.0, 1.0]])
    wide = render_point_cloud(conf_pred, camera_poses=orbit, intrinsics=Kw, exclude_view=[0, 1, -1], splat_radius=1, mask=base, background=(9, 8, 7))
    equal(wide, rc.rule(points, images, keep, orbit.numpy(), np.broadcast_to(Kw.numpy(), (3, 3, 3)), [0, 1, -1], h, w, 1, 0x090807))
    # every index >= 0 is a kept pixel, and where a view is left out, one of ANOTHER view
    for res, left_out in ((out, [0, 1]), (full, [-1, -1]), (wide, [0, 1, -1])):
        idx = res["index"].cpu().numpy()
        hit = idx >= 0
        assert keep.reshape(-1)[idx[hit]].all()
        for m, skipped in enumerate(left_out):
            assert (idx[m][hit[m]] // (h * w) != skipped).all()
    idx, hit = wide["index"].cpu().numpy(), wide["index"].cpu().numpy() >= 0
    print(f"turntable: covered {hit.sum((1, 2)).tolist()} of {h * w} pixels per frame")
    assert hit[0].any() and hit[1].any() and hit[2].any()
    # the colour of a covered pixel is the colour the PLY export writes for its source pixel
    records, _ = hip.cloud_compact(conf_pred["points"][0].float().contiguous(), conf_pred["images"][0].float().contiguous(), base)
    ply_rgb = records.cpu().numpy()[:, 12:15]
    rank = np.cumsum(keep.reshape(-1)) - 1                                                          # the record of a kept pixel
    assert np.array_equal(wide["color"].cpu().numpy()[hit], ply_rgb[rank[idx[hit]]])
    assert (wide["color"].cpu().numpy()[~hit] == [9, 8, 7]).all()
    # an explicit mask and explicit cameras give the same bytes; a new size and one K for every target
    again = render_point_cloud(conf_pred, camera_poses=conf_pred["camera_poses"], intrinsics=K, exclude_view=[0, 1], splat_radius=1, mask=base)
    assert all(torch.equal(again[k].view(torch.uint8), out[k].view(torch.uint8)) for k in out)
    small = render_point_cloud(conf_pred, camera_poses=conf_pred["camera_poses"][0], intrinsics=K[0, 0], size=(20, 33), splat_radius=2, mask=base)
    K1 = np.broadcast_to(K[0, 0].cpu().numpy(), (n, 3, 3))
    equal(small, rc.rule(points, images, keep, poses, K1, None, 20, 33, 2, 0))
    assert all(torch.equal(conf_pred[k].view(torch.uint8), v.view(torch.uint8)) for k, v in snap.items())


def test_orbit_frames_render_and_save(conf_pred, tmp_path):
    from PIL import Image
    base = point_cloud_mask(conf_pred)
    K = estimate_intrinsics(conf_pred, base)
    orbit = orbit_poses(conf_pred, frames=3, mask=base)
    assert tuple(orbit.shape) == (3, 4, 4) and orbit.dtype == torch.float32
    out = render_point_cloud(conf_pred, camera_poses=orbit, intrinsics=K[0, 0], size=(24, 31), splat_radius=1, mask=base)
    points, images, _ = host(conf_pred)
    equal(out, rc.rule(points, images, base.cpu().numpy(), orbit.numpy(), np.broadcast_to(K[0, 0].cpu().numpy(), (3, 3, 3)), None, 24, 31, 1, 0))
    paths = save_rendered_views(out, str(tmp_path / "frames"), prefix="orbit")
    assert [os.path.basename(p) for p in paths] == ["orbit_000.png", "orbit_001.png", "orbit_002.png"]
    for p, want in zip(paths, out["color"].cpu().numpy()):
        assert np.array_equal(np.asarray(Image.open(p).convert("RGB")), want)


def test_inference_recon_with_the_render_flags(tiny_checkpoint, golden_dir, tmp_path, monkeypatch):
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

    # without the flags: the file of before, and no directory of images
    pred = inference_recon.main(args + ["--save_path", str(tmp_path / "plain.ply")])
    save_ply_visualization(pred, str(tmp_path / "want.ply"), verbose=False)
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()

    # --render-dir: one PNG per view, re-rendered from the other view; the PLY is the same file
    out_dir = tmp_path / "renders"
    pred = inference_recon.main(args + ["--save_path", str(tmp_path / "r.ply"), "--render-dir", str(out_dir)])
    assert (tmp_path / "r.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()
    assert sorted(os.listdir(out_dir)) == ["view_000.png", "view_001.png"]
    want = render_point_cloud(pred, exclude_view="self", splat_radius=1)
    for k in range(2):
        assert np.array_equal(np.asarray(Image.open(out_dir / f"view_{k:03d}.png").convert("RGB")), want["color"][k].cpu().numpy())

    # --render-orbit 4 at another size and radius: four more PNGs of that size, the views at that size too
    orbit_dir = tmp_path / "renders_orbit"
    pred = inference_recon.main(args + ["--save_path", str(tmp_path / "o.ply"), "--render-dir", str(orbit_dir), "--render-orbit", "4",
                                        "--render-size", "30", "44", "--render-radius", "2"])
    assert sorted(os.listdir(orbit_dir)) == [f"orbit_{k:03d}.png" for k in range(4)] + ["view_000.png", "view_001.png"]
    base = point_cloud_mask(pred)
    K = estimate_intrinsics(pred, base)
    want = render_point_cloud(pred, camera_poses=orbit_poses(pred, 4, mask=base), intrinsics=K[0, 0], size=(30, 44), splat_radius=2, mask=base)
    for k in range(4):
        img = np.asarray(Image.open(orbit_dir / f"orbit_{k:03d}.png").convert("RGB"))
        assert img.shape == (30, 44, 3) and np.array_equal(img, want["color"][k].cpu().numpy())
    assert Image.open(orbit_dir / "view_000.png").size == (44, 30)
