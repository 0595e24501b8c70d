"""GPU, end to end: voxel downsampling of what `recon` returns, on the tiny synthetic model with a confidence head as
tests/test_cloud_e2e_gpu.py builds it (the fixture is restated here), through save_point_cloud, voxel_downsample and
inference_recon.main."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cloud_check  # noqa: E402
import voxel_check  # noqa: E402
from g2vlm_amd import host  # noqa: E402
from g2vlm_amd.g2vlm_utils import save_ply_visualization, save_point_cloud, voxel_downsample  # noqa: E402
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
    path = str(tmp_path_factory.mktemp("g2vlm_conf_ckpt_voxel"))
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


def snapshot(pred):
    return {k: v.clone() for k, v in pred.items() if torch.is_tensor(v)}


def unchanged(pred, snap):
    return all(torch.equal(pred[k].view(torch.uint8), v.view(torch.uint8)) for k, v in snap.items())   # bits: NaN == NaN


def host_arrays(pred):
    p = pred["points"][0].float().cpu().numpy()
    c = pred["images"][0].float().cpu().numpy()
    local = pred["local_points"][0].float().cpu().numpy()
    conf = None if pred.get("conf") is None else pred["conf"][0].float().cpu().numpy().reshape(p.shape[:3])
    return p, c, local, conf


def expected(path, pred, edge_rtol, min_points=1):
    """(file bytes, restatement, keep mask, voxel size) for the voxel size = the kept points' largest extent / 16 and the default
    origin: every cell index is then below 17, the grid range safe by construction"""
    p, c, local, conf = host_arrays(pred)
    m = cloud_check.keep_mask(p, local, conf, None, None, edge_rtol, True)
    kept = p[m].astype(np.float64)
    v = float((kept.max(0) - kept.min(0)).max() / 16)
    want = voxel_check.downsample(p, c, m, v, voxel_check.default_origin(p, m, v), min_points)
    host.write_ply_records(path, want["records"])
    return open(path, "rb").read(), want, m, v


def test_voxel_export_equals_the_restatement_byte_for_byte(conf_pred, tmp_path):
    snap = snapshot(conf_pred)
    rtol = 0.03
    want_bytes, want, m, v = expected(str(tmp_path / "want.ply"), conf_pred, rtol)
    kept, M = int(m.sum()), len(want["records"])
    print(f"edge_rtol {rtol}: kept {kept} of {m.size}; voxel_size {v}: {M} voxels, largest {int(want['counts'].max())}")
    assert 1 < M < kept
    info = save_point_cloud(conf_pred, str(tmp_path / "sub" / "got.ply"), edge_rtol=rtol, verbose=False, voxel_size=v)
    assert (tmp_path / "sub" / "got.ply").read_bytes() == want_bytes
    assert info == dict(num_points=M, counts=m.reshape(2, -1).sum(1).tolist(), num_input_points=kept)

    out = voxel_downsample(conf_pred, v, edge_rtol=rtol)
    assert set(out) == {"points", "colors", "counts", "origin", "num_input_points"} and out["num_input_points"] == kept
    body = np.frombuffer(want_bytes.split(b"end_header\n", 1)[1], dtype=np.uint8).reshape(-1, 15)
    assert out["points"].cpu().numpy().tobytes() == body[:, :12].tobytes() and np.array_equal(out["colors"].cpu().numpy(), body[:, 12:])
    assert np.array_equal(out["counts"].cpu().numpy(), want["counts"]) and int(out["counts"].sum()) == kept
    assert out["origin"] == tuple(voxel_check.default_origin(*host_arrays(conf_pred)[:1], m, v).tolist())

    # min_points, and an explicit origin shared with another call
    want2_bytes, want2, _, _ = expected(str(tmp_path / "want2.ply"), conf_pred, rtol, min_points=2)
    info2 = save_point_cloud(conf_pred, str(tmp_path / "got2.ply"), edge_rtol=rtol, verbose=False, voxel_size=v, min_points=2)
    assert (tmp_path / "got2.ply").read_bytes() == want2_bytes and info2["num_points"] == len(want2["records"]) <= M
    info3 = save_point_cloud(conf_pred, str(tmp_path / "got3.ply"), edge_rtol=rtol, verbose=False, voxel_size=v, voxel_origin=out["origin"])
    assert (tmp_path / "got3.ply").read_bytes() == want_bytes and info3 == info
    assert unchanged(conf_pred, snap)


def test_without_a_voxel_size_the_export_writes_the_bytes_it_wrote(conf_pred, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                              # save_ply_visualization writes results/input_images.png relative to cwd
    snap = snapshot(conf_pred)
    save_ply_visualization(conf_pred, str(tmp_path / "old.ply"), verbose=False)
    info = save_point_cloud(conf_pred, str(tmp_path / "new.ply"), edge_rtol=None, filter_nan=True, verbose=False, voxel_size=None)
    assert (tmp_path / "new.ply").read_bytes() == (tmp_path / "old.ply").read_bytes()
    assert set(info) == {"num_points", "counts"} and info["num_points"] == sum(info["counts"])
    assert unchanged(conf_pred, snap)


def test_inference_recon_with_a_voxel_size(tiny_checkpoint, golden_dir, tmp_path, monkeypatch):
    from PIL import Image
    from safetensors.torch import load_file
    from g2vlm_amd.g2vlm_utils import load_model_and_tokenizer
    path, _, _ = tiny_checkpoint
    monkeypatch.chdir(tmp_path)
    g = load_file(os.path.join(golden_dir, "recon_real2_dl3dv_2v.safetensors"))
    folder = tmp_path / "frames"
    folder.mkdir()
    for i, name in enumerate(("a_first.png", "b_second.png")):
        Image.fromarray(g["inp.images_u8"][i].permute(1, 2, 0).numpy()).save(folder / name)
    import inference_recon
    base = ["--image_folder", str(folder), "--model_path", path]
    model, tokenizer, new_token_ids, _, dino_tf = load_model_and_tokenizer(path)
    want = model.recon(tokenizer, new_token_ids, dino_tf, g["inp.images_u8"].float() / 255)

    # without the flags: the pred and the file of before
    save_ply_visualization(want, str(tmp_path / "want.ply"), verbose=False)
    pred = inference_recon.main(base + ["--save_path", str(tmp_path / "plain.ply")])
    assert set(pred) == set(want) and (tmp_path / "plain.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()

    # --voxel-size: no other filter than the finite test
    want_bytes, ref, m, v = expected(str(tmp_path / "vox_want.ply"), want, None)
    assert 1 < len(ref["records"]) < int(m.sum())
    pred2 = inference_recon.main(base + ["--save_path", str(tmp_path / "vox.ply"), "--voxel-size", repr(v)])
    assert (tmp_path / "vox.ply").read_bytes() == want_bytes
    assert set(pred2) == set(want)
    for k in ("points", "local_points", "global_points", "camera_poses", "images"):
        assert torch.equal(pred2[k], want[k]), k
    want3_bytes, ref3, _, _ = expected(str(tmp_path / "vox3_want.ply"), want, None, min_points=3)
    inference_recon.main(base + ["--save_path", str(tmp_path / "vox3.ply"), "--voxel-size", repr(v), "--voxel-min-points", "3"])
    assert (tmp_path / "vox3.ply").read_bytes() == want3_bytes and len(ref3["records"]) <= len(ref["records"])
