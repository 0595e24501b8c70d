"""GPU, end to end: the triangle mesh of what `recon` returns, on the tiny synthetic model with a confidence head as
tests/test_cloud_e2e_gpu.py builds it (the fixture is restated here), through reconstruct_mesh and save_mesh; the exports that
existed before write the same bytes whether or not the mesh code has run."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import mesh_check as mc  # noqa: E402
from g2vlm_amd.g2vlm_utils import (point_cloud_mask, reconstruct_mesh, save_mesh, save_ply_visualization, save_point_cloud,  # noqa: E402
                                   save_point_cloud_masked)
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
    path = str(tmp_path_factory.mktemp("g2vlm_conf_ckpt_mesh"))
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
    return pred["points"][0].float().cpu().numpy(), pred["images"][0].float().cpu().numpy()


def equal(out, want, points, colors):
    rec = mc.vertex_records(points, colors, want["used"])
    assert set(out) == {"vertices", "colors", "faces", "vertex_pixel", "counts"} and all(v.is_cuda for v in out.values())
    assert (out["vertices"].dtype, out["colors"].dtype, out["faces"].dtype, out["vertex_pixel"].dtype, out["counts"].dtype) == \
        (torch.float32, torch.uint8, torch.int32, torch.int32, torch.int32)
    V, F = len(want["vertex_pixel"]), len(want["faces"])
    assert tuple(out["vertices"].shape) == (V, 3) and tuple(out["colors"].shape) == (V, 3) and tuple(out["faces"].shape) == (F, 3)
    assert np.array_equal(out["vertices"].cpu().numpy().view(np.uint8).reshape(-1, 12), rec[:, :12])
    assert np.array_equal(out["colors"].cpu().numpy(), rec[:, 12:])
    assert np.array_equal(out["faces"].cpu().numpy(), want["faces"])
    assert np.array_equal(out["vertex_pixel"].cpu().numpy(), want["vertex_pixel"])
    assert np.array_equal(out["counts"].cpu().numpy(), want["counts"])


def parse(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    nv, nf = int(lines[2].split()[-1]), int(lines[9].split()[-1])
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and lines[2].startswith("element vertex ") and \
        lines[9].startswith("element face ") and lines[10] == "property list uchar int vertex_indices" and len(body) == 15 * nv + 13 * nf
    return head, body[:15 * nv], np.frombuffer(body[:15 * nv], mc.VERTEX_DTYPE), np.frombuffer(body[15 * nv:], mc.FACE_DTYPE)


def test_reconstruct_mesh_equals_the_rule_on_point_cloud_masks_mask(conf_pred):
    snap = {k: v.clone() for k, v in conf_pred.items() if torch.is_tensor(v)}
    points, colors = host(conf_pred)
    keep = point_cloud_mask(conf_pred, edge_rtol=0.03).cpu().numpy()
    assert 0 < keep.sum() < keep.size
    want = mc.rule(points, keep)
    assert len(want["faces"]) > 0
    equal(reconstruct_mesh(conf_pred), want, points, colors)                                        # edge_rtol = 0.03 is the default
    lengths = np.sqrt(np.where(want["anti"], want["ea"], want["em"])[want["four"]])
    max_edge = float(np.median(lengths))
    limited = mc.rule(points, keep, max_edge)
    assert 0 < len(limited["faces"]) < len(want["faces"])
    equal(reconstruct_mesh(conf_pred, max_edge=max_edge), limited, points, colors)
    # other filters: the confidence threshold with the edge filter off; nothing but the finite test
    for kw in (dict(conf_threshold=0.5, edge_rtol=None), dict(edge_rtol=None), dict(edge_rtol=None, filter_nan=False)):
        m = point_cloud_mask(conf_pred, **kw).cpu().numpy()
        equal(reconstruct_mesh(conf_pred, **kw), mc.rule(points, m), points, colors)
    assert all(torch.equal(conf_pred[k], v) for k, v in snap.items())                               # the inputs are untouched


def test_an_explicit_mask_goes_through_and_equals_the_filters(conf_pred):
    points, colors = host(conf_pred)
    mv = point_cloud_mask(conf_pred, edge_rtol=0.03, min_views=1)
    want = mc.rule(points, mv.cpu().numpy())
    for mask in (mv, mv.view(torch.uint8), mv[None]):
        equal(reconstruct_mesh(conf_pred, mask=mask), want, points, colors)
    equal(reconstruct_mesh(conf_pred, min_views=1), want, points, colors)
    none = reconstruct_mesh(conf_pred, mask=torch.zeros_like(mv))
    assert tuple(none["faces"].shape) == (0, 3) and tuple(none["vertices"].shape) == (0, 3) and none["counts"].tolist() == [[0, 0], [0, 0]]


def test_save_mesh_writes_a_file_that_parses_back(conf_pred, tmp_path, capsys):
    points, colors = host(conf_pred)
    keep = point_cloud_mask(conf_pred, edge_rtol=0.03)
    want = mc.rule(points, keep.cpu().numpy())
    path = str(tmp_path / "sub" / "mesh.ply")
    info = save_mesh(conf_pred, path)
    V, F = len(want["vertex_pixel"]), len(want["faces"])
    assert info == dict(num_vertices=V, num_faces=F, counts=want["counts"].tolist())
    assert "mesh.ply" in capsys.readouterr().out
    head, vertex_block, vert, face = parse(path)
    assert np.array_equal(vert.view(np.uint8).reshape(-1, 15), mc.vertex_records(points, colors, want["used"]))
    assert (face["n"] == 3).all() and np.array_equal(face["v"], want["faces"])
    mesh = reconstruct_mesh(conf_pred)
    assert np.array_equal(vert["p"].view(np.int32), mesh["vertices"].cpu().numpy().view(np.int32)) and \
        np.array_equal(vert["c"], mesh["colors"].cpu().numpy()) and np.array_equal(face["v"], mesh["faces"].cpu().numpy())
    # the vertex block is the cloud export of the used pixels, header and bytes
    cloud = str(tmp_path / "used.ply")
    save_point_cloud_masked(conf_pred, cloud, torch.from_numpy(want["used"]).cuda(), verbose=False)
    chead, cbody = open(cloud, "rb").read().split(b"end_header\n", 1)
    assert cbody == vertex_block and head.startswith(chead)
    # with an explicit mask and a limit, quietly
    quiet = str(tmp_path / "quiet.ply")
    lim = mc.rule(points, keep.cpu().numpy(), 0.01)
    info = save_mesh(conf_pred, quiet, mask=keep, max_edge=0.01, verbose=False)
    assert capsys.readouterr().out == "" and info["num_faces"] == len(lim["faces"]) and info["num_vertices"] == len(lim["vertex_pixel"])
    assert np.array_equal(parse(quiet)[3]["v"], lim["faces"])


def test_the_exports_of_before_write_the_same_bytes(conf_pred, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                              # save_ply_visualization writes results/input_images.png relative to cwd

    def exports(tag):
        save_point_cloud(conf_pred, str(tmp_path / f"cloud_{tag}.ply"), verbose=False)
        save_point_cloud(conf_pred, str(tmp_path / f"conf_{tag}.ply"), conf_threshold=0.5, edge_rtol=None, verbose=False)
        save_ply_visualization(conf_pred, str(tmp_path / f"vis_{tag}.ply"), verbose=False)
        return [(tmp_path / f"{name}_{tag}.ply").read_bytes() for name in ("cloud", "conf", "vis")]

    before = exports("before")
    reconstruct_mesh(conf_pred)
    save_mesh(conf_pred, str(tmp_path / "mesh.ply"), max_edge=0.05, verbose=False)
    assert exports("after") == before


def test_inference_recon_with_the_mesh_flag(tiny_checkpoint, golden_dir, tmp_path, monkeypatch):
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

    # without the flag: the file of before and no mesh
    inference_recon.main(args + ["--save_path", str(tmp_path / "plain.ply")])
    assert sorted(p.name for p in tmp_path.glob("*.ply")) == ["plain.ply"]

    # --mesh alone: the PLY is the same file, the mesh is save_mesh's under its default edge filter
    pred = inference_recon.main(args + ["--save_path", str(tmp_path / "m.ply"), "--mesh", str(tmp_path / "mesh.ply")])
    assert (tmp_path / "m.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
    save_mesh(pred, str(tmp_path / "want.ply"), verbose=False)
    assert (tmp_path / "mesh.ply").read_bytes() == (tmp_path / "want.ply").read_bytes()

    # under filter flags the mesh takes point_cloud_mask's mask for them; an absolute edge tolerance nothing exceeds keeps every finite
    # pixel (this checkpoint's depth is noise from pixel to pixel: the relative rule would keep nothing)
    r = mc.rule(pred["points"][0].float().cpu().numpy())
    lim = repr(float(np.sqrt(np.median(np.where(r["anti"], r["ea"], r["em"])))))                   # about half of the triangles exceed it
    pred = inference_recon.main(args + ["--save_path", str(tmp_path / "f.ply"), "--edge-atol", "1e9", "--mesh", str(tmp_path / "fmesh.ply"),
                                        "--mesh-max-edge", lim])
    save_point_cloud(pred, str(tmp_path / "fwant.ply"), edge_rtol=None, edge_atol=1e9, verbose=False)
    assert (tmp_path / "f.ply").read_bytes() == (tmp_path / "fwant.ply").read_bytes()
    mask = point_cloud_mask(pred, edge_atol=1e9)
    want = reconstruct_mesh(pred, mask=mask, max_edge=float(lim))
    unlimited = reconstruct_mesh(pred, mask=mask)
    _, _, vert, face = parse(str(tmp_path / "fmesh.ply"))
    assert np.array_equal(face["v"], want["faces"].cpu().numpy()) and np.array_equal(vert["p"].view(np.int32), want["vertices"].cpu().numpy().view(np.int32))
    assert unlimited["faces"].shape[0] == 2 * mask.shape[0] * (mask.shape[1] - 1) * (mask.shape[2] - 1) > want["faces"].shape[0] > 0
