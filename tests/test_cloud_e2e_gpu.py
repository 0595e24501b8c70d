"""GPU, end to end: the filtered point-cloud export and the intrinsics on what `recon` returns, on the tiny synthetic model as
tests/test_boundary.py builds it (once with a confidence head), and through inference_recon.main with and without the new flags."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cloud_check  # noqa: E402
from g2vlm_amd import host  # noqa: E402
from g2vlm_amd.g2vlm_utils import estimate_intrinsics, point_cloud_mask, save_ply_visualization, save_point_cloud  # noqa: E402
from oracle import synth  # noqa: E402  checker-side helpers only (synthetic weights)

pytestmark = pytest.mark.gpu
POINT_HEAD_DAMP = 2.0 ** -8                                 # see conf_pred


@pytest.fixture(scope="module")
def conf_pred(tmp_path_factory):
    """recon of two 56 x 70 views by a train_conf_pi3 checkpoint (test_boundary.py::test_conf_checkpoint_through_the_config_flag).

    One thing differs from that checkpoint: the output layer of `point_head` (weight and bias) is scaled by POINT_HEAD_DAMP.
    The synthetic weights are random, and the head has separate rows for every pixel of a patch, so as they come the local
    depth exp(.) is independent noise from pixel to pixel (0.00016 .. 7282 over one view) and the depth-edge rule marks all 7 840
    pixels at every tolerance below 1: a filtered export of it is an empty file.  Damped by 2^-8 the depth is 1 +- 3.5 % and the
    rule at rtol 0.03 marks some pixels and leaves some (CPU oracle: 2 253 of 7 840 edges; 7 435 at 2^-7, none at 2^-9; on the MI355X 2 247 edges, 2 794 kept), which is
    what an end-to-end test of the filters needs.  Every other tensor, the config classes and the loading path are
    test_boundary.py's."""
    from conftest import write_tiny_checkpoint
    from safetensors.torch import save_file
    from g2vlm_amd.g2vlm_utils import LazySafetensors
    from g2vlm_amd.modeling.g2vlm import (G2VLM, G2VLMConfig, Dinov2WithRegistersConfig, Dinov2WithRegistersModel, Qwen2VLConfig,
                                          Qwen2VLForCausalLM, Qwen2VLVisionConfig, Qwen2VisionTransformerPretrainedModel)
    path = str(tmp_path_factory.mktemp("g2vlm_conf_ckpt"))
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


def expected_file(path, pred, conf_threshold=None, edge_rtol=None, edge_atol=None):
    """write_ply_binary(p[m], c[m]) for m from cloud_check; returns (bytes, m)"""
    p, c, local, conf = host_arrays(pred)
    logit = None if conf_threshold is None else host.conf_logit_threshold(conf_threshold)
    m = cloud_check.keep_mask(p, local, conf, logit, edge_atol, edge_rtol, True)
    host.write_ply_binary(path, p.reshape(-1, 3)[m.reshape(-1)], c.transpose(0, 2, 3, 1).reshape(-1, 3)[m.reshape(-1)])
    return open(path, "rb").read(), m


def test_unfiltered_export_is_the_existing_file_byte_for_byte(conf_pred, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                              # save_ply_visualization writes results/input_images.png relative to cwd
    snap = snapshot(conf_pred)
    save_ply_visualization(conf_pred, str(tmp_path / "old.ply"), verbose=False)
    info = save_point_cloud(conf_pred, str(tmp_path / "sub" / "new.ply"), edge_rtol=None, filter_nan=True, verbose=False)
    old = (tmp_path / "old.ply").read_bytes()
    assert (tmp_path / "sub" / "new.ply").read_bytes() == old
    assert info["num_points"] == sum(info["counts"]) == (len(old.split(b"end_header\n", 1)[1]) // 15) and len(info["counts"]) == 2
    p, c, _, _ = host_arrays(conf_pred)                      # no filter at all: every pixel, in order
    host.write_ply_binary(str(tmp_path / "all_want.ply"), p.reshape(-1, 3), c.transpose(0, 2, 3, 1).reshape(-1, 3))
    info = save_point_cloud(conf_pred, str(tmp_path / "all.ply"), edge_rtol=None, filter_nan=False, verbose=False)
    assert (tmp_path / "all.ply").read_bytes() == (tmp_path / "all_want.ply").read_bytes() and info["counts"] == [56 * 70] * 2
    assert unchanged(conf_pred, snap)


def _conf_threshold(conf):
    """0.5, or the median of the fixture's own confidence if 0.5 keeps everything or nothing"""
    kept = int((conf > host.conf_logit_threshold(0.5)).sum())
    return 0.5 if 0 < kept < conf.size else float(1.0 / (1.0 + np.exp(-np.float64(np.median(conf)))))


def test_filtered_export_equals_the_host_restatement(conf_pred, tmp_path):
    """edge_rtol = 0.03 with conf_threshold = 0.5: the file is write_ply_binary(p[m], c[m]) for m from cloud_check, byte for byte,
    and the filters keep some pixels and drop some."""
    snap = snapshot(conf_pred)
    p, c, local, conf = host_arrays(conf_pred)
    total = conf.size
    thr, rtol = _conf_threshold(conf), 0.03
    want, m = expected_file(str(tmp_path / "want.ply"), conf_pred, conf_threshold=thr, edge_rtol=rtol)
    print(f"conf_threshold {thr}: kept {int(m.sum())} of {total}; edges at rtol {rtol}: "
          f"{int(cloud_check.edge_mask(local[..., 2], None, rtol).sum())}; conf above: {int((conf > host.conf_logit_threshold(thr)).sum())}")
    info = save_point_cloud(conf_pred, str(tmp_path / "got.ply"), conf_threshold=thr, edge_rtol=rtol, verbose=False)
    assert (tmp_path / "got.ply").read_bytes() == want
    assert info["num_points"] == int(m.sum()) and info["counts"] == m.reshape(2, -1).sum(1).tolist()
    assert 0 < info["num_points"] < total
    dm = point_cloud_mask(conf_pred, conf_threshold=thr, edge_rtol=rtol)
    assert dm.dtype == torch.bool and dm.is_cuda and np.array_equal(dm.cpu().numpy(), m)
    # intrinsics of the same result, unmasked and restricted to the kept pixels: the kernel's own answer on these inputs
    # (tests/test_cloud_gpu.py holds the kernel to fp64 lstsq), NaN exactly where lstsq has nothing to fit
    from g2vlm_amd import hip
    for mask, mm in ((None, None), (dm, m)):
        K = estimate_intrinsics(conf_pred, mask)
        assert K.shape == (1, 2, 3, 3) and K.dtype == torch.float32 and K.is_cuda
        direct, used = hip.intrinsics_lsq(conf_pred["local_points"][0].contiguous(), None if mask is None else mask)
        assert torch.equal(K[0].view(torch.int32), direct.view(torch.int32))
        ref, ref_used = cloud_check.fit_intrinsics(local, mm)
        assert used.cpu().tolist() == ref_used.tolist()
        assert np.array_equal(np.isnan(K[0].cpu().numpy()), np.isnan(ref))
    assert unchanged(conf_pred, snap)


def test_conf_threshold_without_a_confidence_head_is_refused(conf_pred, tmp_path):
    plain = dict(conf_pred, conf=None)                       # what recon returns from a checkpoint without conf_decoder / conf_head
    with pytest.raises(ValueError, match="conf"):
        save_point_cloud(plain, str(tmp_path / "no.ply"), conf_threshold=0.5)
    with pytest.raises(ValueError, match="conf"):
        point_cloud_mask(plain, conf_threshold=0.5)
    assert not os.path.exists(tmp_path / "no.ply")


def test_inference_recon_with_and_without_the_new_flags(tiny_checkpoint, golden_dir, tmp_path, capsys, monkeypatch):
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

    # no new flag: the stage-method path of today - the same pred, the same PLY bytes
    model, tokenizer, new_token_ids, _, dino_tf = load_model_and_tokenizer(path)
    want = model.recon(tokenizer, new_token_ids, dino_tf, g["inp.images_u8"].float() / 255)
    assert want["conf"] is None
    save_ply_visualization(want, str(tmp_path / "want.ply"), verbose=False)
    pred = inference_recon.main(base + ["--save_path", str(tmp_path / "plain.ply")])
    assert set(pred) == set(want) and "intrinsics" not in pred
    for k in ("points", "local_points", "global_points", "camera_poses", "images"):
        assert torch.equal(pred[k], want[k]), k
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()

    # a checkpoint without a confidence head: what --conf-threshold hands to save_point_cloud is refused
    with pytest.raises(ValueError, match="conf"):
        save_point_cloud(want, str(tmp_path / "never.ply"), conf_threshold=0.5)
    assert not os.path.exists(tmp_path / "never.ply")

    # --edge-rtol 0.03 --intrinsics: the filtered file, K per view printed and returned
    capsys.readouterr()
    snap = snapshot(want)
    pred2 = inference_recon.main(base + ["--save_path", str(tmp_path / "edge.ply"), "--edge-rtol", "0.03", "--intrinsics"])
    out = capsys.readouterr().out
    expect, m = expected_file(str(tmp_path / "edge_want.ply"), want, edge_rtol=0.03)
    assert (tmp_path / "edge.ply").read_bytes() == expect
    print(f"--edge-rtol 0.03 kept {int(m.sum())} of {m.size}")
    K = pred2["intrinsics"]
    assert K.shape == (1, 2, 3, 3) and K.dtype == torch.float32 and bool(torch.isfinite(K).all())
    assert "view 0: K = " in out and "view 1: K = " in out
    for k in ("points", "local_points", "global_points", "camera_poses", "images"):
        assert torch.equal(pred2[k], want[k]), k
    assert unchanged(want, snap)
