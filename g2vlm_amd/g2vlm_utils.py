"""Loader / glue with the reference's names and return conventions (reference g2vlm_utils.py:31-149).

    model, tokenizer, new_token_ids, vit_image_transform, dino_transform = load_model_and_tokenizer(model_path)

Differences from the reference, all inside the boundary contract of SURVEY.md §8b: accepts a path
string OR the argparse Namespace the reference scripts pass by mistake (H6); takes `device=`;
never reaches the hub (configs, tokenizer files and `model.safetensors` are read from the local
directory only); writes PLY without open3d.
"""
import os

import numpy as np
import torch

from . import host
from .host import QwenVL2ImageTransform, DinoImageNormalizeTransform
from .modeling.g2vlm import (G2VLM, G2VLMConfig, Qwen2VLConfig, Qwen2VLForCausalLM, Dinov2WithRegistersConfig,
                             Dinov2WithRegistersModel, Qwen2VLVisionConfig, Qwen2VisionTransformerPretrainedModel)


def add_special_tokens(tokenizer):
    """reference data/data_utils.py:278-313"""
    specials = []
    for v in tokenizer.special_tokens_map.values():
        specials += [v] if isinstance(v, str) else list(v)
    new = [t for t in ("<|im_start|>", "<|im_end|>", "<|vision_start|>", "<|vision_end|>") if t not in specials]
    n_new = tokenizer.add_tokens(new)
    ids = dict(bos_token_id=tokenizer.convert_tokens_to_ids("<|im_start|>"), eos_token_id=tokenizer.convert_tokens_to_ids("<|im_end|>"),
               start_of_image=tokenizer.convert_tokens_to_ids("<|vision_start|>"),
               end_of_image=tokenizer.convert_tokens_to_ids("<|vision_end|>"))
    return tokenizer, ids, n_new


def pil_img2rgb(image):
    """reference data/data_utils.py:254-263"""
    from PIL import Image
    if image.mode == "RGBA" or image.info.get("transparency", None) is not None:
        image = image.convert("RGBA")
        white = Image.new(mode="RGB", size=image.size, color=(255, 255, 255))
        white.paste(image, mask=image.split()[3])
        return white
    return image.convert("RGB")


def build_model(llm_config, vit_config, dino_config, state_dict, device="cuda", *, decode_weights="bf16",
                decode_kv="bf16"):
    """decode_weights: "bf16" or "fp8" (weight-only e4m3 decode, G2VLM.decode_weights).
    decode_kv: "bf16" or "fp8" (e4m3 KV cache of the decode step, G2VLM.decode_kv)."""
    llm_config.qk_norm = True
    llm_config.tie_word_embeddings = False
    llm_config.layer_module = "Qwen2VLMoTDecoderLayer"
    if vit_config is not None:
        vit_config.patch_size = 14
    from .modeling.dinov3 import DINOv3ViTConfig, DINOv3ViTModel
    v3 = isinstance(dino_config, DINOv3ViTConfig)          # the use_dinov3 variant (reference g2vlm.py:86, 134): config objects only,
    config = G2VLMConfig(visual_und=vit_config is not None, visual_recon=True, llm_config=llm_config, vit_config=vit_config,
                         dino_config=dino_config, vit_max_num_patch_per_side=36, use_dinov3=v3)   # the reference's loader never sets it
    model = G2VLM(Qwen2VLForCausalLM(llm_config), Qwen2VisionTransformerPretrainedModel(vit_config) if vit_config else None,
                  DINOv3ViTModel(dino_config) if v3 else Dinov2WithRegistersModel(dino_config), config)
    model.load_state_dict(state_dict, strict=False)
    model.decode_weights = decode_weights
    model.decode_kv = decode_kv
    return model.to(device).eval()


def configs_from_dims(dims):
    L, D, V = dims["llm"], dims["dino"], dims["vit"]
    llm = Qwen2VLConfig(vocab_size=L["vocab"], hidden_size=L["hidden"], intermediate_size=L["ffn"], num_hidden_layers=L["layers"],
                        num_attention_heads=L["heads"], num_key_value_heads=L["kv_heads"], rms_norm_eps=L["eps"],
                        rope_theta=L["theta"], rope_scaling={"type": "mrope", "mrope_section": [16, 24, 24]})
    vit = Qwen2VLVisionConfig(depth=V["depth"], embed_dim=V["embed"], hidden_size=V["out"], mlp_ratio=V["mlp_ratio"],
                              num_heads=V["heads"]) if V["depth"] > 0 else None
    if D.get("v3"):
        from .modeling.dinov3 import DINOv3ViTConfig
        dino = DINOv3ViTConfig(**D["v3"])
    else:
        dino = Dinov2WithRegistersConfig(hidden_size=D["hidden"], num_hidden_layers=D["layers"], num_attention_heads=D["heads"],
                                         patch_size=14, image_size=518)
    return llm, vit, dino


class LazySafetensors:
    """Mapping view of a .safetensors file that reads one tensor per access (fp32), so the 4.5 B-parameter checkpoint is
    never resident on the host as a whole: g2vlm_amd.weights.Weights pulls each tensor, rounds / lays it out and uploads it
    (the reference loads the full dict with safetensors.torch.load_file, g2vlm_utils.py:63-66)."""

    def __init__(self, path):
        from safetensors import safe_open
        self.f = safe_open(path, framework="pt", device="cpu")
        self._keys = set(self.f.keys())

    def __contains__(self, k):
        return k in self._keys

    def __getitem__(self, k):
        if k not in self._keys:
            raise KeyError(f"{k!r} is not in the checkpoint (state-dict key contract: g2vlm_amd/synthetic.py::param_shapes)")
        return self.f.get_tensor(k).float()

    def keys(self):
        return self._keys


def load_model_and_tokenizer(model_path, device=None, *, decode_weights=None, decode_kv=None):
    """decode_weights: None (a Namespace's .decode_weights if it has one, else "bf16"), "bf16" or "fp8"; decode_kv: the same
    for the decode step's KV cache (.decode_kv)."""
    if decode_weights is None:
        decode_weights = getattr(model_path, "decode_weights", None) or "bf16"
    if decode_kv is None:
        decode_kv = getattr(model_path, "decode_kv", None) or "bf16"
    if not isinstance(model_path, (str, os.PathLike)):                      # argparse Namespace (reference bug H6)
        model_path = getattr(model_path, "model_path", None) or getattr(model_path, "model-path", None)
        if model_path is None:
            raise TypeError("load_model_and_tokenizer takes a checkpoint directory or a Namespace with .model_path")
    if not os.path.isdir(model_path):
        raise FileNotFoundError(f"{model_path!r} is not a local directory; this loader never fetches from the hub. "
                                "Download InternRobotics/G2VLM-2B-MoT first and pass its path.")
    device = device or "cuda"
    llm_config = Qwen2VLConfig.from_json_file(os.path.join(model_path, "text_config.json"))
    vit_config = Qwen2VLVisionConfig.from_json_file(os.path.join(model_path, "vit_config.json"))
    dino_config = Dinov2WithRegistersConfig.from_json_file(os.path.join(model_path, "dino_config.json"))
    model = build_model(llm_config, vit_config, dino_config, LazySafetensors(os.path.join(model_path, "model.safetensors")), device,
                        decode_weights=decode_weights, decode_kv=decode_kv)
    from transformers import AutoTokenizer
    tokenizer = AutoTokenizer.from_pretrained(model_path, local_files_only=True)
    tokenizer, new_token_ids, _ = add_special_tokens(tokenizer)
    vit_image_transform = QwenVL2ImageTransform(768, 768, 14)
    dino_transform = DinoImageNormalizeTransform(target_size=518)
    return model, tokenizer, new_token_ids, vit_image_transform, dino_transform


def build_transform(pixel=224):
    return QwenVL2ImageTransform(pixel, pixel, 14)


def process_conversation(images, conversation):
    return [pil_img2rgb(image) for image in images], conversation


def save_ply_visualization(pred_dict, save_path, init_conf_threshold=20.0, filter_nan=True, verbose=True):
    """reference g2vlm_utils.py:84-149: PLY of points[0] coloured by images[0], NaN/inf filtered, plus
    results/input_images.png (8-per-row grid).  The reference's identity-sized bilinear resample of
    the points is skipped (H8: it is a no-op when sizes match)."""
    images = pred_dict["images"][0].detach().float().cpu()
    pts = pred_dict["points"][0].detach().float().cpu()
    n, _, h, w = images.shape
    if pts.shape[1:3] != (h, w):
        pts = torch.nn.functional.interpolate(pts.permute(0, 3, 1, 2), (h, w), mode="bilinear", align_corners=False,
                                              antialias=True).permute(0, 2, 3, 1)
    os.makedirs(os.path.dirname(save_path) or ".", exist_ok=True)
    try:
        from PIL import Image
        nrow, pad = 8, 2
        cols, rows = min(n, nrow), (n + nrow - 1) // nrow
        grid = torch.zeros((3, rows * (h + pad) + pad, cols * (w + pad) + pad))
        for i in range(n):
            r, c = divmod(i, nrow)
            grid[:, pad + r * (h + pad): pad + r * (h + pad) + h, pad + c * (w + pad): pad + c * (w + pad) + w] = images[i]
        os.makedirs("results", exist_ok=True)
        Image.fromarray((grid.clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0).numpy()).save("results/input_images.png")
    except Exception as e:                                                    # noqa: BLE001  (visual by-product only)
        if verbose:
            print("input_images.png not written:", e)
    p = pts.numpy().reshape(-1, 3)
    c = images.permute(0, 2, 3, 1).numpy().reshape(-1, 3)
    if filter_nan:
        ok = ~(np.isnan(p).any(1) | np.isinf(p).any(1))
        p, c = p[ok], c[ok]
    host.write_ply_binary(save_path, p, c)


# ---- filtered export and intrinsics on the device (csrc/cloud.hip) -----------------------------------------------------------
def _cloud_inputs(pred_dict, conf_threshold, edge_rtol, edge_atol, need_images):
    """Batch entry 0 of a recon result as the contiguous fp32 device tensors the kernels take, after every check that can
    refuse the call: (points [N,H,W,3], local [N,H,W,3], conf [N,H,W] or None, images [N,3,H,W] or None, logit threshold)."""
    logit = None
    if conf_threshold is not None:
        if pred_dict.get("conf") is None:
            raise ValueError("conf_threshold needs pred_dict['conf']: this checkpoint has no confidence head (train_conf_pi3)")
        logit = host.conf_logit_threshold(conf_threshold)
    for name, tol in (("edge_rtol", edge_rtol), ("edge_atol", edge_atol)):
        if tol is not None and not float(tol) >= 0.0:
            raise ValueError(f"{name} must be >= 0, got {tol}")
    points, local = pred_dict["points"], pred_dict["local_points"]
    if points.dim() != 5 or points.shape[0] != 1 or points.shape[-1] != 3 or local.shape != points.shape:
        raise ValueError(f"points / local_points [1,N,H,W,3] expected, got {tuple(points.shape)} / {tuple(local.shape)}")
    n, h, w = points.shape[1:4]
    images = pred_dict["images"] if need_images else pred_dict.get("images")
    if images is not None:
        if images.dim() != 5 or images.shape[0] != 1 or tuple(images.shape[1:3]) != (n, 3) or tuple(images.shape[3:]) != (h, w):
            raise ValueError(f"images {tuple(images.shape)} do not match points {tuple(points.shape)}: [1,N,3,H,W] with the points' "
                             "N, H, W expected (save_ply_visualization resamples; this export does not)")
        images = images[0].detach().float().contiguous() if need_images else None
    conf = None
    if logit is not None:
        conf = pred_dict["conf"]
        if conf.numel() != n * h * w:
            raise ValueError(f"conf {tuple(conf.shape)} does not match points {tuple(points.shape)}")
        conf = conf.detach().float().reshape(n, h, w).contiguous()
    return points[0].detach().float().contiguous(), local[0].detach().float().contiguous(), conf, images, logit


def point_cloud_mask(pred_dict, conf_threshold=None, edge_rtol=None, edge_atol=None, filter_nan=True, min_views=None,
                     max_in_front=None, depth_rtol=0.03, intrinsics=None):
    """Which pixels of a recon result belong in the cloud: bool [N,H,W] on the device (hip.cloud_mask).
    filter_nan: the world point is finite.  conf_threshold: a probability p in (0,1); keeps sigmoid(conf) > p, evaluated as
    conf > log(p/(1-p)).  edge_rtol / edge_atol: drops depth discontinuities ("flying pixels") by the reference's depth_edge
    rule on the local depth (modeling/pi3/utils/geometry.py:339, 3x3 window).
    min_views / max_in_front: the multi-view consistency filter on top of those (multiview_consistency has the rule; depth_rtol
    and intrinsics are its arguments): a pixel stays only if at least min_views other views confirm its point and at most
    max_in_front other views see it floating in front of their surface.  Both None: no such filter, no camera_poses needed."""
    from . import hip
    if min_views is not None or max_in_front is not None:
        min_views, max_in_front = _consistency_args(min_views, max_in_front, depth_rtol)
        points, local, conf, _, logit = _cloud_inputs(pred_dict, conf_threshold, edge_rtol, edge_atol, need_images=False)
        poses = _consistency_poses(pred_dict, points.shape[0])
        K = _consistency_K(intrinsics, points.shape[0])
        base = _cloud_mask_u8(points, local, conf, logit, edge_rtol, edge_atol, filter_nan)
        if K is None:
            K, _ = hip.intrinsics_lsq(local, base)
        return hip.cloud_consistency(points, local, base, poses, K.to(points.device), depth_rtol, min_views, max_in_front)[2].view(torch.bool)
    points, local, conf, _, logit = _cloud_inputs(pred_dict, conf_threshold, edge_rtol, edge_atol, need_images=False)
    if not (filter_nan or conf is not None or edge_rtol is not None or edge_atol is not None):
        return torch.ones(points.shape[:3], dtype=torch.bool, device=points.device)
    return hip.cloud_mask(points, local, conf, logit or 0.0, edge_atol, edge_rtol, finite=filter_nan).view(torch.bool)


def _consistency_args(min_views, max_in_front, depth_rtol):
    """(min_agree, max_in_front) as the kernel takes them, or ValueError: before any launch"""
    def integer(x):
        return not isinstance(x, bool) and isinstance(x, (int, np.integer))
    if min_views is not None and not (integer(min_views) and 1 <= min_views <= 255):
        raise ValueError(f"min_views must be an integer in [1, 255], got {min_views!r}")
    if max_in_front is not None and not (integer(max_in_front) and 0 <= max_in_front <= 255):
        raise ValueError(f"max_in_front must be an integer in [0, 255], got {max_in_front!r}")
    try:
        ok = float(depth_rtol) >= 0.0 and np.isfinite(float(depth_rtol))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"depth_rtol must be finite and >= 0, got {depth_rtol!r}")
    return (0 if min_views is None else int(min_views)), (-1 if max_in_front is None else int(max_in_front))


def _consistency_poses(pred_dict, n):
    poses = pred_dict.get("camera_poses")
    if not torch.is_tensor(poses) or tuple(poses.shape) != (1, n, 4, 4):
        raise ValueError(f"the multi-view filter needs pred_dict['camera_poses'] [1,N,4,4] with N = {n}, got "
                         f"{tuple(poses.shape) if torch.is_tensor(poses) else type(poses).__name__}")
    if n > 256:
        raise ValueError(f"the multi-view filter takes at most 256 views (its counts are bytes), got {n}")
    return poses[0].detach().float().contiguous()


def _consistency_K(intrinsics, n):
    if intrinsics is None:
        return None
    if not torch.is_tensor(intrinsics) or tuple(intrinsics.shape) not in ((1, n, 3, 3), (n, 3, 3)):
        raise ValueError(f"intrinsics: a tensor [1,N,3,3] or [N,3,3] with N = {n} expected, got "
                         f"{tuple(intrinsics.shape) if torch.is_tensor(intrinsics) else type(intrinsics).__name__}")
    return intrinsics.detach().float().reshape(n, 3, 3).contiguous()


def multiview_consistency(pred_dict, depth_rtol=0.03, intrinsics=None, conf_threshold=None, edge_rtol=None, edge_atol=None,
                          filter_nan=True, mask=None):
    """Does any other view see this point?  On the device (hip.cloud_consistency; include/g2vlm_hip.h and DESIGN.md 6k have the
    exact rule): the world point of every pixel of view i is projected into every other view j with j's pose and pinhole K and
    compared with the depth j predicts at the pixel it falls in (nearest neighbour).  It AGREES if the two depths differ by at
    most depth_rtol times j's depth, lies IN FRONT if it is nearer to camera j than that - in the free space before the surface j
    sees - and counts as neither where it is behind (occluded), outside j's image or on a pixel j's mask drops.
    The pixels that take part, as sources and as targets, are those point_cloud_mask keeps under the same filter arguments; an
    explicit mask (bool / uint8 [N,H,W]) replaces the filters.  intrinsics: [1,N,3,3] or [N,3,3]; None takes
    estimate_intrinsics(pred_dict, that mask) - a view whose K has a NaN entry then confirms nobody.
    Returns dict(agree uint8 [N,H,W], in_front uint8 [N,H,W] = the number of other views in each class, covisibility int32
    [N,N,2] = per (i, j) the pixels of i that agree / lie in front in j, intrinsics fp32 [1,N,3,3], mask bool [N,H,W] = the base
    mask), all on the device.  Needs pred_dict["camera_poses"] [1,N,4,4]; at most 256 views."""
    from . import hip
    _consistency_args(None, None, depth_rtol)
    if mask is not None:
        points, local, _, _, _ = _cloud_inputs(pred_dict, None, None, None, need_images=False)
    else:
        points, local, conf, _, logit = _cloud_inputs(pred_dict, conf_threshold, edge_rtol, edge_atol, need_images=False)
    n = points.shape[0]
    poses = _consistency_poses(pred_dict, n)
    K = _consistency_K(intrinsics, n)
    if mask is not None:
        base = _voxel_mask(mask, points.shape[:3], points.device)
    else:
        base = _cloud_mask_u8(points, local, conf, logit, edge_rtol, edge_atol, filter_nan)
    if K is None:
        K, _ = hip.intrinsics_lsq(local, base)
    K = K.to(points.device)
    agree, in_front, _, pairs = hip.cloud_consistency(points, local, base, poses, K, depth_rtol, pairs=True)
    return dict(agree=agree, in_front=in_front, covisibility=pairs, intrinsics=K.unsqueeze(0), mask=base.view(torch.bool))


def _voxel_args(voxel_size, origin, min_points):
    """(voxel_size as a float, origin as three floats or None, min_points), or ValueError: before any launch"""
    try:
        v = float(voxel_size)
    except (TypeError, ValueError):
        raise ValueError(f"voxel_size must be a number > 0, got {voxel_size!r}") from None
    if not (v > 0.0 and np.isfinite(v)):
        raise ValueError(f"voxel_size must be finite and > 0, got {voxel_size}")
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)) or min_points < 1:
        raise ValueError(f"min_points must be an integer >= 1, got {min_points}")
    if origin is not None:
        origin = [float(o) for o in (origin.tolist() if hasattr(origin, "tolist") else origin)]
        if len(origin) != 3 or not all(np.isfinite(o) for o in origin):
            raise ValueError(f"origin must be three finite numbers, got {origin}")
    return v, origin, int(min_points)


def _voxel_mask(mask, shape, device):
    """An explicit mask as uint8 [N,H,W] on the device, or ValueError"""
    if not torch.is_tensor(mask):
        raise ValueError(f"mask: a bool / uint8 tensor [N,H,W] = {tuple(shape)} expected, got {type(mask).__name__}")
    if mask.dim() == 4 and mask.shape[0] == 1:
        mask = mask[0]
    if tuple(mask.shape) != tuple(shape) or mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"mask: bool / uint8 [N,H,W] = {tuple(shape)} expected, got {mask.dtype} {tuple(mask.shape)}")
    mask = mask.to(device).contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _voxel_run(points, images, mask, v, origin, min_points):
    """assign + reduce on the device tensors: dict(records, points, colors, counts, origin, num_input_points).  ValueError, with
    nothing written, where a point falls outside the 2^21 cells per axis that the grid has."""
    from . import hip
    lo = hi = None
    if origin is None:
        # Open3D's convention for voxel_down_sample: the minimum bound of the cloud minus half a voxel, formed in fp64
        lo, hi, n = hip.voxel_bounds(points, mask)
        origin = [x - v * 0.5 for x in lo] if n else [0.0, 0.0, 0.0]
    voxel_of, (m, n_in, n_out, status) = hip.voxel_assign(points, mask, v, origin)
    if n_out or status:
        if lo is None:
            lo, hi, _ = hip.voxel_bounds(points, mask)
        raise ValueError(f"voxel_size {v} is too small for this cloud: {n_out} of its points lie outside the grid's 2^21 cells per "
                         f"axis around the origin {origin} (extent of the points: min {lo}, max {hi}; status {status})")
    records, counts, out_points, out_colors = hip.voxel_reduce(points, images, voxel_of, m, v, origin)
    if min_points > 1:                                      # on the [M]-sized outputs: M is small
        keep = counts >= min_points
        records, counts, out_points, out_colors = records[keep], counts[keep], out_points[keep], out_colors[keep]
    return dict(records=records, points=out_points, colors=out_colors, counts=counts, origin=tuple(origin), num_input_points=n_in)


def _cloud_mask_u8(points, local, conf, logit, edge_rtol, edge_atol, filter_nan):
    from . import hip
    if filter_nan or conf is not None or edge_rtol is not None or edge_atol is not None:
        return hip.cloud_mask(points, local, conf, logit or 0.0, edge_atol, edge_rtol, finite=filter_nan)
    return torch.ones(points.shape[:3], dtype=torch.uint8, device=points.device)


def voxel_downsample(pred_dict, voxel_size, origin=None, min_points=1, conf_threshold=None, edge_rtol=None, edge_atol=None,
                     filter_nan=True, mask=None):
    """The cloud of a recon result with one vertex per occupied cell of a regular grid, on the device (hip.voxel_assign /
    voxel_reduce; DESIGN.md 6j has the exact rule): the vertex is the mean of the cell's points, its colour the mean of their
    colour bytes, rounded half up; cells come in the order in which the pixels (view-major, row-major) first reach them.
    The pixels are those point_cloud_mask keeps under the same filter arguments; an explicit mask (bool / uint8 [N,H,W])
    replaces the filters.  Non-finite points never take part.  min_points drops cells with fewer points.
    origin: a corner of the grid (cells are [origin + k v, origin + (k + 1) v)); pass the same one to put two scenes on one grid.
    None takes the convention of Open3D's voxel_down_sample - the per-axis minimum of the participating points minus
    voxel_size / 2, in fp64.  Open3D itself is not a dependency and nothing here is tested against it: the convention is followed,
    equality with its output is not claimed.
    Returns dict(points fp32 [M,3], colors uint8 [M,3], counts int32 [M], origin (3 floats), num_input_points).  ValueError if
    the voxel size is so small that a point lies more than 2^20 cells from the origin."""
    v, origin, min_points = _voxel_args(voxel_size, origin, min_points)
    if mask is not None:
        points, _, _, images, _ = _cloud_inputs(pred_dict, None, None, None, need_images=True)
        mask = _voxel_mask(mask, points.shape[:3], points.device)
    else:
        points, local, conf, images, logit = _cloud_inputs(pred_dict, conf_threshold, edge_rtol, edge_atol, need_images=True)
        mask = _cloud_mask_u8(points, local, conf, logit, edge_rtol, edge_atol, filter_nan)
    out = _voxel_run(points, images, mask, v, origin, min_points)
    del out["records"]
    return out


def save_point_cloud(pred_dict, save_path, conf_threshold=None, edge_rtol=0.03, edge_atol=None, filter_nan=True, verbose=True,
                     voxel_size=None, voxel_origin=None, min_points=1):
    """save_ply_visualization's PLY with the filters of point_cloud_mask, packed on the device: mask, stable compaction into
    15-byte records, ONE device-to-host copy of the kept records, one write.  With every filter but filter_nan off the file is
    byte-identical to save_ply_visualization's.  Returns dict(num_points, counts = kept pixels per view).
    voxel_size: the kept pixels are voxel-downsampled first (voxel_downsample; voxel_origin and min_points are its origin and
    min_points) and only the cells' records are copied and written; the dict then also has num_input_points, and num_points is
    the number of records written."""
    if voxel_size is not None:
        voxel_size, voxel_origin, min_points = _voxel_args(voxel_size, voxel_origin, min_points)
    points, local, conf, images, logit = _cloud_inputs(pred_dict, conf_threshold, edge_rtol, edge_atol, need_images=True)
    mask = _cloud_mask_u8(points, local, conf, logit, edge_rtol, edge_atol, filter_nan)
    return _save_masked(points, images, mask, save_path, verbose, voxel_size, voxel_origin, min_points)


def save_point_cloud_masked(pred_dict, save_path, mask, verbose=True, voxel_size=None, voxel_origin=None, min_points=1):
    """save_point_cloud for an explicit mask (bool / uint8 [N,H,W], e.g. point_cloud_mask(min_views=...)'s) in place of the
    filter arguments: the same compaction, the same optional voxel downsampling, the same file and the same returned dict."""
    if voxel_size is not None:
        voxel_size, voxel_origin, min_points = _voxel_args(voxel_size, voxel_origin, min_points)
    points, _, _, images, _ = _cloud_inputs(pred_dict, None, None, None, need_images=True)
    mask = _voxel_mask(mask, points.shape[:3], points.device)
    return _save_masked(points, images, mask, save_path, verbose, voxel_size, voxel_origin, min_points)


def _save_masked(points, images, mask, save_path, verbose, voxel_size, voxel_origin, min_points):
    """the export of checked inputs: compaction (or voxel downsampling) of the pixels mask keeps, one copy, one write"""
    from . import hip
    if voxel_size is not None:
        vox = _voxel_run(points, images, mask, voxel_size, voxel_origin, min_points)
        records = vox["records"]
        counts = hip.cloud_counts(points, images, mask)
    else:
        records, counts = hip.cloud_compact(points, images, mask)
    os.makedirs(os.path.dirname(save_path) or ".", exist_ok=True)
    host.write_ply_records(save_path, records.cpu())
    counts = counts.cpu().tolist()
    if voxel_size is not None:
        if verbose:
            print(f"{save_path}: {records.shape[0]} voxels of {voxel_size} from {vox['num_input_points']} of {mask.numel()} points, "
                  f"per view {counts}")
        return dict(num_points=int(records.shape[0]), counts=counts, num_input_points=vox["num_input_points"])
    if verbose:
        print(f"{save_path}: {records.shape[0]} of {mask.numel()} points kept, per view {counts}")
    return dict(num_points=int(records.shape[0]), counts=counts)


def estimate_intrinsics(pred_dict, mask=None):
    """Pinhole intrinsics of every view from its local points (x z, y z, z) (reference g2vlm.py:1203-1205): the least-squares
    fit u = fx X/Z + cx, v = fy Y/Z + cy over pixel centres, on the device (hip.intrinsics_lsq).  mask: bool / uint8 [N,H,W]
    (point_cloud_mask's) restricts the fit.  Returns fp32 [1,N,3,3]; NaN where a view does not determine an entry."""
    from . import hip
    _, local, _, _, _ = _cloud_inputs(pred_dict, None, None, None, need_images=False)
    if mask is not None:
        mask = mask.to(local.device)
        if mask.dim() == 4 and mask.shape[0] == 1:
            mask = mask[0]
        if tuple(mask.shape) != tuple(local.shape[:3]) or mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"mask: bool [N,H,W] = {tuple(local.shape[:3])} expected, got {mask.dtype} {tuple(mask.shape)}")
        mask = mask.contiguous()
    K, _ = hip.intrinsics_lsq(local, mask)
    return K.unsqueeze(0)


# ---- triangle-mesh export (csrc/mesh.hip) ------------------------------------------------------------------------------------
def _max_edge_arg(max_edge):
    """max_edge as a float or None, or ValueError"""
    if max_edge is None:
        return None
    try:
        ok = not isinstance(max_edge, bool) and float(max_edge) >= 0.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"max_edge must be a number >= 0 (or None: no limit), got {max_edge!r}")
    return float(max_edge)


def _mask_replaces_filters(filters):
    """ValueError if one of the filter arguments - (name, value, default) each - is given beside an explicit mask"""
    given = [k for k, v, d in filters if not (v is d or v == d)]
    if given:
        raise ValueError(f"an explicit mask replaces the filters: {', '.join(given)} may not be given with it")


def _mesh_inputs(pred_dict, conf_threshold, edge_rtol, edge_atol, filter_nan, min_views, max_in_front, depth_rtol, intrinsics, mask,
                 max_edge):
    """(points [N,H,W,3], images [N,3,H,W], mask uint8 [N,H,W], max_edge as a float or None) on the device, or ValueError: every
    check comes before any launch"""
    max_edge = _max_edge_arg(max_edge)
    if mask is not None:
        _mask_replaces_filters((("conf_threshold", conf_threshold, None), ("edge_rtol", edge_rtol, 0.03), ("edge_atol", edge_atol, None),
                                ("filter_nan", filter_nan, True), ("min_views", min_views, None), ("max_in_front", max_in_front, None),
                                ("depth_rtol", depth_rtol, 0.03), ("intrinsics", intrinsics, None)))
    points, _, _, images, _ = _cloud_inputs(pred_dict, None, None, None, need_images=True)
    n, h, w = points.shape[:3]
    if n > 65535 or 2 * n * (h - 1) * (w - 1) > 2 ** 31 - 1:
        raise ValueError(f"{n} views of {h} x {w} are more than a mesh holds (65535 views, 2^31 - 1 candidate triangles)")
    if mask is not None:
        return points, images, _voxel_mask(mask, points.shape[:3], points.device), max_edge
    keep = point_cloud_mask(pred_dict, conf_threshold, edge_rtol, edge_atol, filter_nan, min_views, max_in_front, depth_rtol, intrinsics)
    return points, images, keep.view(torch.uint8), max_edge


def reconstruct_mesh(pred_dict, conf_threshold=None, edge_rtol=0.03, edge_atol=None, filter_nan=True, min_views=None,
                     max_in_front=None, depth_rtol=0.03, intrinsics=None, mask=None, max_edge=None):
    """The reconstruction as a triangle mesh, on the device (hip.cloud_mesh; include/g2vlm_hip.h and DESIGN.md 6n have the exact
    rule): every view's pixel grid is triangulated - a quad whose four corners are kept is cut along its shorter diagonal, a quad
    with three kept corners gives one triangle - and the triangles face the camera that saw them.  The views stay separate sheets.
    The kept pixels are those of point_cloud_mask under the same filter arguments (edge_rtol = 0.03 by default: no triangle spans a
    depth discontinuity); an explicit mask (bool / uint8 [N,H,W], e.g. point_cloud_mask(...)'s) replaces the filters and may not be
    combined with them.  max_edge: triangles with an edge longer than this (in the units of the points) are dropped as well.
    Returns dict(vertices fp32 [V,3], colors uint8 [V,3] - the bytes the PLY export writes -, faces int32 [F,3] of vertex ids,
    vertex_pixel int32 [V] = the flat pixel (i H + y) W + x of every vertex, increasing, counts int32 [N,2] = vertices and faces
    per view).  Only pixels that a face references are vertices.  ValueError for every bad argument, before any launch."""
    from . import hip
    points, images, keep, max_edge = _mesh_inputs(pred_dict, conf_threshold, edge_rtol, edge_atol, filter_nan, min_views, max_in_front,
                                                  depth_rtol, intrinsics, mask, max_edge)
    m = hip.cloud_mesh(points, images, keep, max_edge, face_records=False)
    rec = m["vertex_records"]
    return dict(vertices=rec[:, :12].reshape(-1).view(torch.float32).view(-1, 3), colors=rec[:, 12:].contiguous(), faces=m["faces"],
                vertex_pixel=torch.nonzero(m["used"].reshape(-1)).reshape(-1).to(torch.int32), counts=m["counts"])


def save_mesh(pred_dict, save_path, conf_threshold=None, edge_rtol=0.03, edge_atol=None, filter_nan=True, min_views=None,
              max_in_front=None, depth_rtol=0.03, intrinsics=None, mask=None, max_edge=None, verbose=True):
    """reconstruct_mesh's mesh as a binary little-endian PLY that mesh viewers open: the vertex block of save_point_cloud_masked
    for the used pixels, then `element face F` / `property list uchar int vertex_indices`.  Both blocks are packed on the device:
    one device-to-host copy each, one write.  Returns dict(num_vertices, num_faces, counts = [vertices, faces] per view)."""
    from . import hip
    points, images, keep, max_edge = _mesh_inputs(pred_dict, conf_threshold, edge_rtol, edge_atol, filter_nan, min_views, max_in_front,
                                                  depth_rtol, intrinsics, mask, max_edge)
    m = hip.cloud_mesh(points, images, keep, max_edge, faces=False)
    os.makedirs(os.path.dirname(save_path) or ".", exist_ok=True)
    host.write_ply_mesh(save_path, m["vertex_records"].cpu(), m["face_records"].cpu())
    counts = m["counts"].cpu().tolist()
    nv, nf = int(m["vertex_records"].shape[0]), int(m["face_records"].shape[0])
    if verbose:
        print(f"{save_path}: {nv} vertices of {keep.numel()} pixels, {nf} triangles, per view {counts}")
    return dict(num_vertices=nv, num_faces=nf, counts=counts)


# ---- surface normals (csrc/normals.hip) --------------------------------------------------------------------------------------
def _view_angle_cos(max_view_angle):
    """cos(max_view_angle) as the fp32 number the device compares with (fp64 cosine, rounded once), or ValueError"""
    ok = isinstance(max_view_angle, (int, float, np.integer, np.floating)) and not isinstance(max_view_angle, bool)
    a = float(max_view_angle) if ok else 0.0
    if not (ok and 0.0 < a <= 90.0):
        raise ValueError(f"max_view_angle must be an angle in degrees in (0, 90], got {max_view_angle!r}")
    return float(np.float32(np.cos(np.radians(a))))


def _normals_inputs(pred_dict, step, max_edge, frame, conf_threshold, edge_rtol, edge_atol, filter_nan, mask, need_images):
    """(the points the normals are taken of [N,H,W,3], poses [N,4,4] or None, keep mask uint8 [N,H,W], images [N,3,H,W] or None, step,
    max_edge as a float or None) on the device, or ValueError: every check comes before any launch"""
    if isinstance(step, bool) or not isinstance(step, (int, np.integer)) or not 1 <= step <= 8:
        raise ValueError(f"step must be an integer in [1, 8], got {step!r}")
    max_edge = _max_edge_arg(max_edge)
    if frame not in ("world", "camera"):
        raise ValueError(f"frame must be 'world' or 'camera', got {frame!r}")
    if mask is not None:
        _mask_replaces_filters((("conf_threshold", conf_threshold, None), ("edge_rtol", edge_rtol, 0.03), ("edge_atol", edge_atol, None),
                                ("filter_nan", filter_nan, True)))
        points, local, conf, images, logit = _cloud_inputs(pred_dict, None, None, None, need_images=need_images)
    else:
        points, local, conf, images, logit = _cloud_inputs(pred_dict, conf_threshold, edge_rtol, edge_atol, need_images=need_images)
    n = points.shape[0]
    if n > 65535:
        raise ValueError(f"at most 65535 views per call, got {n}")
    poses = None
    if frame == "world":
        poses = pred_dict.get("camera_poses")
        if not torch.is_tensor(poses) or tuple(poses.shape) != (1, n, 4, 4):
            raise ValueError(f"frame='world' needs pred_dict['camera_poses'] [1,N,4,4] with N = {n} (the normals look at each view's camera "
                             f"centre), got {tuple(poses.shape) if torch.is_tensor(poses) else type(poses).__name__}")
        poses = poses[0].detach().float().to(points.device).contiguous()
    if mask is not None:
        keep = _voxel_mask(mask, points.shape[:3], points.device)
    else:
        keep = _cloud_mask_u8(points, local, conf, logit, edge_rtol, edge_atol, filter_nan)
    return (points if frame == "world" else local), poses, keep, images, int(step), max_edge


def estimate_normals(pred_dict, step=1, max_edge=None, frame="world", conf_threshold=None, edge_rtol=0.03, edge_atol=None,
                     filter_nan=True, mask=None, colors=False):
    """A surface normal for every pixel of a recon result, on the device (hip.cloud_normals; include/g2vlm_hip.h and DESIGN.md 6u have
    the exact rule): the cross products of the edges from a pixel's point to its four axis neighbours at distance `step`, summed over
    the neighbour pairs that are there, normalised and turned towards the camera that saw the pixel - an image-space normal, no
    plane fit over a larger window.  frame="world": normals of `points`, towards each view's centre in `camera_poses`;
    frame="camera": normals of `local_points`, towards the origin.  The pixels that take part, as centres and as neighbours, are
    those point_cloud_mask keeps under the same filter arguments (edge_rtol = 0.03 by default: no normal is taken across a depth
    discontinuity); an explicit mask (bool / uint8 [N,H,W]) replaces the filters and may not be combined with them.  max_edge:
    neighbours farther away than this (in the units of the points) do not count.
    Returns, on the device, dict(normals fp32 [N,H,W,3] unit vectors, valid bool [N,H,W], cos_view fp32 [N,H,W] = the cosine of the
    angle between the normal and the ray back to the camera, in [0, 1]); a pixel that takes no part, has no pair of neighbours or
    whose neighbours are collinear is not valid and has zeros.  colors=True adds images fp32 [1,N,3,H,W] = n / 2 + 1 / 2, shaped like
    pred_dict["images"]: dict(pred_dict, images=r["images"]) shows the normals through render_point_cloud and save_point_cloud_masked.
    ValueError for every bad argument, before any launch."""
    from . import hip
    if not isinstance(colors, (bool, np.bool_)):
        raise ValueError(f"colors must be a bool, got {colors!r}")
    src, poses, keep, _, step, max_edge = _normals_inputs(pred_dict, step, max_edge, frame, conf_threshold, edge_rtol, edge_atol, filter_nan,
                                                           mask, need_images=False)
    r = hip.cloud_normals(src, keep, poses, step, max_edge, colors=bool(colors))
    out = dict(normals=r["normals"], valid=r["valid"].view(torch.bool), cos_view=r["cos_view"])
    if colors:
        out["images"] = r["colors"].unsqueeze(0)
    return out


def view_angle_mask(pred_dict, max_view_angle, step=1, max_edge=None, frame="world", conf_threshold=None, edge_rtol=0.03, edge_atol=None,
                    filter_nan=True, mask=None):
    """Which pixels are seen at no more than max_view_angle degrees (in (0, 90]) from their surface normal: bool [N,H,W] on the
    device.  A pixel is kept iff the filters (or the explicit mask) keep it, its normal is valid (estimate_normals, same arguments)
    and cos_view >= float32(cos(max_view_angle)), the cosine taken in fp64 and rounded once.  Points seen at a grazing angle - where
    a small error in the ray becomes a large error in depth - are what this drops."""
    from . import hip
    threshold = _view_angle_cos(max_view_angle)
    src, poses, keep, _, step, max_edge = _normals_inputs(pred_dict, step, max_edge, frame, conf_threshold, edge_rtol, edge_atol, filter_nan,
                                                           mask, need_images=False)
    r = hip.cloud_normals(src, keep, poses, step, max_edge)
    return (r["valid"] != 0) & (r["cos_view"] >= threshold)


def save_point_cloud_normals(pred_dict, save_path, step=1, max_edge=None, max_view_angle=None, conf_threshold=None, edge_rtol=0.03,
                             edge_atol=None, filter_nan=True, mask=None, verbose=True):
    """save_point_cloud's PLY with `nx ny nz` beside every vertex (world frame; estimate_normals has the rule and the arguments), packed
    on the device: mask, normals, stable compaction into 27-byte records <f4 x, y, z; <f4 nx, ny, nz; u1 r, g, b, ONE device-to-host
    copy of the kept records, one write.  The vertices, their order and their colours are those of save_point_cloud_masked under the
    same mask.  A kept pixel without a valid normal is written with a zero normal; max_view_angle (degrees, view_angle_mask) drops
    such pixels along with those seen at a larger angle.  Returns dict(num_points, counts = kept pixels per view, num_normals = the
    written vertices whose normal is valid)."""
    from . import hip
    threshold = None if max_view_angle is None else _view_angle_cos(max_view_angle)
    points, poses, keep, images, step, max_edge = _normals_inputs(pred_dict, step, max_edge, "world", conf_threshold, edge_rtol, edge_atol,
                                                                  filter_nan, mask, need_images=True)
    r = hip.cloud_normals(points, keep, poses, step, max_edge)
    if threshold is not None:
        keep = ((r["valid"] != 0) & (r["cos_view"] >= threshold)).view(torch.uint8)
    records, counts = hip.cloud_compact_normals(points, r["normals"], images, keep)
    num_normals = int(((keep != 0) & (r["valid"] != 0)).sum().item())
    os.makedirs(os.path.dirname(save_path) or ".", exist_ok=True)
    host.write_ply_normal_records(save_path, records.cpu())
    counts = counts.cpu().tolist()
    if verbose:
        print(f"{save_path}: {records.shape[0]} of {keep.numel()} points kept, {num_normals} with a normal, per view {counts}")
    return dict(num_points=int(records.shape[0]), counts=counts, num_normals=num_normals)


def save_normal_maps(pred_dict, directory, prefix="normal", frame="camera", step=1, max_edge=None, conf_threshold=None, edge_rtol=0.03,
                     edge_atol=None, filter_nan=True, mask=None):
    """estimate_normals' colours as PNGs directory/prefix_000.png ... (Pillow), one per view: the bytes the PLY export would write for
    n / 2 + 1 / 2 - (uint8)(clip(c, 0, 1) * 255) -, black where no normal is valid.  frame="camera" by default: the usual normal map
    beside a depth map (x right, y down, z forward; a wall that faces the camera has the normal (0, 0, -1) and the bytes
    (127, 127, 0)).  Returns the paths."""
    from PIL import Image
    from . import hip
    src, poses, keep, _, step, max_edge = _normals_inputs(pred_dict, step, max_edge, frame, conf_threshold, edge_rtol, edge_atol, filter_nan,
                                                           mask, need_images=False)
    colors = hip.cloud_normals(src, keep, poses, step, max_edge, colors=True)["colors"]
    img = (colors.double().clamp(0.0, 1.0) * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu().numpy()
    os.makedirs(directory, exist_ok=True)
    paths = []
    for k, view in enumerate(img):
        paths.append(os.path.join(directory, f"{prefix}_{k:03d}.png"))
        Image.fromarray(view).save(paths[-1])
    return paths


# ---- evaluation against ground truth (csrc/nn.hip) ---------------------------------------------------------------------------
def _points3(t, what):
    if not torch.is_tensor(t) or not t.is_floating_point() or t.dim() < 1 or t.shape[-1] != 3:
        raise ValueError(f"{what}: a floating-point tensor [...,3] expected, got "
                         f"{(t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__}")
    return t


def _flat_mask(mask, shape, what):
    """an optional mask over points of `shape` (without the 3) as a flat uint8 tensor, or ValueError"""
    if mask is None:
        return None
    if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != tuple(shape):
        raise ValueError(f"{what}: a bool / uint8 tensor {tuple(shape)} expected, got "
                         f"{(mask.dtype, tuple(mask.shape)) if torch.is_tensor(mask) else type(mask).__name__}")
    mask = mask.reshape(-1).contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _max_distance(max_distance):
    if max_distance is None:
        return None
    try:
        ok = not isinstance(max_distance, bool) and float(max_distance) >= 0.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"max_distance must be a number >= 0 (or None: no limit), got {max_distance!r}")
    return float(max_distance)


def nearest_points(query, target, max_distance=None, query_mask=None, target_mask=None):
    """For every query point the nearest target point, on the device (hip.cloud_nn; include/g2vlm_hip.h and DESIGN.md 6p have the
    exact rule): query and target are tensors [...,3] on the device, flattened to [Nq,3] and [Nt,3]; the masks (bool / uint8, the
    shape of the points without the 3) drop points on either side, non-finite points never take part; max_distance is the largest
    distance that counts.  Exact: the smallest fp32 squared distance, ties to the lowest index - no approximate search.
    Returns dict(index int32 [Nq] = the flat target index or -1, sq_distance fp32 [Nq] (+inf without a neighbour), distance fp32
    [Nq] = sqrt(sq_distance)).  ValueError for every bad argument, before any launch."""
    from . import hip
    query, target = _points3(query, "query"), _points3(target, "target")
    max_distance = _max_distance(max_distance)
    query_mask = _flat_mask(query_mask, query.shape[:-1], "query_mask")
    target_mask = _flat_mask(target_mask, target.shape[:-1], "target_mask")
    if not (query.is_cuda and target.is_cuda and query.device == target.device):
        raise ValueError(f"query and target must be on one GPU, got {query.device} and {target.device}")
    if query.numel() // 3 > 2 ** 31 - 1 or target.numel() // 3 > 2 ** 31 - 1:
        raise ValueError("at most 2^31 - 1 points per side")
    q, t = query.detach().float().reshape(-1, 3).contiguous(), target.detach().float().reshape(-1, 3).contiguous()
    qm = None if query_mask is None else query_mask.to(q.device)
    tm = None if target_mask is None else target_mask.to(q.device)
    index, sq, _ = hip.cloud_nn(q, t, max_distance, qm, tm)
    return dict(index=index, sq_distance=sq, distance=torch.sqrt(sq))


def align_points(src, dst, mask=None, with_scale=True):
    """Umeyama's closed-form similarity dst ~ s R src + t over corresponding points (the alignment family of the reference's
    modeling/pi3/utils/alignment.py, here in closed form): src, dst tensors [...,3] of one shape, mask bool / uint8 [...] or None.
    The rows that take part are those the mask keeps whose six coordinates are finite.  Means, covariance and variance are fp64
    reductions on the tensors' device; the 3 x 3 SVD runs in fp64 on the host; det(U) det(V) < 0 (the best orthogonal fit is a
    reflection) flips the last singular vector, so R is always a rotation.  with_scale=False fixes s = 1.
    Returns dict(scale float, rotation fp64 [3,3], translation fp64 [3], transform fp64 [4,4] = [[s R, t], [0, 1]], num_points),
    tensors on the host.  ValueError for bad arguments, and where fewer than 3 rows take part or src has no spread."""
    src, dst = _points3(src, "src"), _points3(dst, "dst")
    if src.shape != dst.shape:
        raise ValueError(f"src and dst must have one shape, got {tuple(src.shape)} and {tuple(dst.shape)}")
    if not isinstance(with_scale, (bool, np.bool_)):
        raise ValueError(f"with_scale must be a bool, got {with_scale!r}")
    mask = _flat_mask(mask, src.shape[:-1], "mask")
    s64, d64 = src.detach().reshape(-1, 3).double(), dst.detach().reshape(-1, 3).to(src.device).double()
    valid = torch.isfinite(s64).all(1) & torch.isfinite(d64).all(1)
    if mask is not None:
        valid &= mask.to(src.device) != 0
    col = valid.unsqueeze(1)
    zero = torch.zeros((), dtype=torch.float64, device=s64.device)
    n = valid.sum().double()
    mu_s, mu_d = torch.where(col, s64, zero).sum(0) / n, torch.where(col, d64, zero).sum(0) / n
    xs, xd = torch.where(col, s64 - mu_s, zero), torch.where(col, d64 - mu_d, zero)
    cov = (xd.t() @ xs) / n
    var = (xs * xs).sum() / n
    host_ = torch.cat([cov.reshape(-1), var.reshape(1), mu_s, mu_d, n.reshape(1)]).cpu().numpy()      # one copy of 17 numbers
    cov, var, mu_s, mu_d, count = host_[:9].reshape(3, 3), host_[9], host_[10:13], host_[13:16], int(host_[16])
    if count < 3 or not var > 0.0:
        raise ValueError(f"align_points needs at least 3 finite corresponding points with some spread, got {count} (variance {var})")
    U, D, Vt = np.linalg.svd(cov)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    s = float((D * S).sum() / var) if with_scale else 1.0
    t = mu_d - s * (R @ mu_s)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s * R, t
    return dict(scale=s, rotation=torch.from_numpy(R), translation=torch.from_numpy(t), transform=torch.from_numpy(M), num_points=count)


def _apply_transform(M, points):
    """rows of a 4 x 4 (numpy fp64) applied to points fp32 [n,3], op by op in fp64 - ((a0 x + a1 y) + a2 z) + t - and rounded to
    fp32 once: the same numbers wherever it runs"""
    p = points.double()
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return torch.stack([((float(M[k, 0]) * x + float(M[k, 1]) * y) + float(M[k, 2]) * z) + float(M[k, 3]) for k in range(3)], 1).float().contiguous()


def _eval_thresholds(thresholds):
    try:
        out = tuple(float(t) for t in thresholds)
        ok = all(not isinstance(t, bool) for t in thresholds) and all(t > 0.0 and np.isfinite(t) for t in out)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"thresholds must be a sequence of finite numbers > 0, got {thresholds!r}")
    return out


def _metrics_from_distances(acc_sq, acc_found, comp_sq, comp_found, thresholds, max_distance):
    """The metrics of evaluate_reconstruction from the two nearest-neighbour results: *_sq fp32 squared distances of the points that
    take part on each side (+inf without a neighbour), *_found bool.  fp64 throughout."""
    out = dict(n_pred=int(acc_sq.numel()), n_gt=int(comp_sq.numel()), thresholds=tuple(thresholds))
    nan = float("nan")
    dist = {}
    for name, sq in (("accuracy", acc_sq), ("completeness", comp_sq)):
        d = torch.sqrt(sq.double())
        if max_distance is not None:
            d = torch.clamp(d, max=float(max_distance))
        dist[name] = d
        if d.numel():
            s = torch.sort(d).values
            out[name], out[name + "_median"] = float(d.mean()), float(0.5 * (s[(d.numel() - 1) // 2] + s[d.numel() // 2]))
        else:
            out[name] = out[name + "_median"] = nan
    out["chamfer"] = 0.5 * (out["accuracy"] + out["completeness"])
    out["precision"], out["recall"], out["fscore"], out["precision_hits"], out["recall_hits"] = [], [], [], [], []
    for T in thresholds:
        ha = int((acc_found & (acc_sq.double() <= T * T)).sum())
        hc = int((comp_found & (comp_sq.double() <= T * T)).sum())
        p = ha / out["n_pred"] if out["n_pred"] else nan
        r = hc / out["n_gt"] if out["n_gt"] else nan
        f = nan if (p != p or r != r) else (2 * p * r / (p + r) if p + r > 0 else 0.0)
        for key, v in (("precision", p), ("recall", r), ("fscore", f), ("precision_hits", ha), ("recall_hits", hc)):
            out[key].append(v)
    return out, dist


def evaluate_reconstruction(pred_dict, gt_points, gt_mask=None, align="sim3", thresholds=(0.05,), max_distance=None, mask=None,
                            conf_threshold=None, edge_rtol=None, edge_atol=None, filter_nan=True, return_distances=False):
    """A recon result measured against a ground-truth cloud, on the device (two exact nearest-neighbour searches, hip.cloud_nn;
    DESIGN.md 6p).  The predicted cloud is the pixels point_cloud_mask keeps under the same filter arguments; an explicit mask (bool
    / uint8 [N,H,W]) replaces the filters and may not be combined with them.  Non-finite points take no part on either side.
    gt_points: [N,H,W,3] (or [1,N,H,W,3]), pixel-aligned with the prediction - then align="sim3" fits Umeyama's similarity
    (align_points) on the pixels valid on both sides and applies it to the prediction -, or an unordered cloud [M,3], for which
    align must be "none" or a 4 x 4 similarity to apply (no correspondences: nothing to fit; ICP is not provided).  gt_mask: bool /
    uint8 of the ground truth's shape without the 3.
    Returns dict(accuracy = the mean distance from a predicted point to its nearest ground-truth point, completeness = the other
    direction, chamfer = their mean, accuracy_median, completeness_median, thresholds, precision / recall / fscore = a list with
    one entry per threshold (the share of predicted / ground-truth points with a neighbour within it; 2 p r / (p + r)),
    precision_hits / recall_hits = the counts, n_pred, n_gt, transform fp64 [4,4]); with return_distances=True also
    accuracy_distances / completeness_distances fp64 and pred_points fp32 [n_pred,3] = the aligned prediction, on the device.
    Distances are fp64 square roots of the kernel's fp32 squared distances and means are fp64.  With max_distance a neighbour
    farther away does not count: such a point is a miss at every threshold and enters the means and medians with max_distance
    itself (clipping).  An empty side gives NaN for its mean, median and rate (and for chamfer and fscore); without max_distance a
    point of the other side then has distance +inf.  ValueError for every bad argument, before any launch."""
    from . import hip
    thresholds = _eval_thresholds(thresholds)
    max_distance = _max_distance(max_distance)
    if not isinstance(return_distances, (bool, np.bool_)):
        raise ValueError(f"return_distances must be a bool, got {return_distances!r}")
    if mask is not None:
        given = [k for k, v, d in (("conf_threshold", conf_threshold, None), ("edge_rtol", edge_rtol, None), ("edge_atol", edge_atol, None),
                                   ("filter_nan", filter_nan, True)) if not (v is d or v == d)]
        if given:
            raise ValueError(f"an explicit mask replaces the filters: {', '.join(given)} may not be given with it")
    points, local, conf, _, logit = _cloud_inputs(pred_dict, conf_threshold, edge_rtol, edge_atol, need_images=False)
    n, h, w = points.shape[:3]
    gt = _points3(gt_points, "gt_points")
    if gt.dim() == 5 and gt.shape[0] == 1:
        gt = gt[0]
        if torch.is_tensor(gt_mask) and gt_mask.dim() == 4 and gt_mask.shape[0] == 1:
            gt_mask = gt_mask[0]
    if gt.dim() == 4:
        if tuple(gt.shape[:3]) != (n, h, w):
            raise ValueError(f"gt_points {tuple(gt.shape)} is not pixel-aligned with the prediction [{n},{h},{w},3]")
    elif gt.dim() != 2:
        raise ValueError(f"gt_points: [N,H,W,3] pixel-aligned with the prediction or an unordered cloud [M,3] expected, got {tuple(gt.shape)}")
    gm = _flat_mask(gt_mask, gt.shape[:-1], "gt_mask")
    M = None
    if isinstance(align, str):
        if align not in ("sim3", "none"):
            raise ValueError(f"align must be 'sim3', 'none' or a 4 x 4 similarity, got {align!r}")
        if align == "sim3" and gt.dim() != 4:
            raise ValueError("align='sim3' needs pixel-aligned gt_points [N,H,W,3]: an unordered cloud has no correspondences to fit "
                             "(pass align='none' or a 4 x 4 similarity)")
    else:
        try:
            M = np.array(align.detach().cpu().numpy() if torch.is_tensor(align) else align, dtype=np.float64)
        except (TypeError, ValueError):
            M = None
        if M is None or M.shape != (4, 4) or not np.isfinite(M).all() or M[3].tolist() != [0.0, 0.0, 0.0, 1.0]:
            raise ValueError("align: 'sim3', 'none' or a finite 4 x 4 matrix with the last row (0, 0, 0, 1) expected")
    if mask is not None:
        keep = _voxel_mask(mask, points.shape[:3], points.device)
    else:
        keep = _cloud_mask_u8(points, local, conf, logit, edge_rtol, edge_atol, filter_nan)
    dev = points.device
    P, pm = points.reshape(-1, 3), keep.reshape(-1)
    G = gt.detach().to(dev).float().reshape(-1, 3).contiguous()
    gm = None if gm is None else gm.to(dev)
    if isinstance(align, str) and align == "sim3":
        both = pm != 0 if gm is None else (pm != 0) & (gm != 0)
        M = align_points(P, G, mask=both)["transform"].numpy()
    Pa = P if M is None else _apply_transform(M, P)
    idx_a, sq_a, _ = hip.cloud_nn(Pa, G, max_distance, pm, gm)
    idx_c, sq_c, _ = hip.cloud_nn(G, Pa, max_distance, gm, pm)
    part_a = (pm != 0) & torch.isfinite(Pa).all(1)
    part_c = torch.isfinite(G).all(1) if gm is None else (gm != 0) & torch.isfinite(G).all(1)
    out, dist = _metrics_from_distances(sq_a[part_a], idx_a[part_a] >= 0, sq_c[part_c], idx_c[part_c] >= 0, thresholds, max_distance)
    out["transform"] = torch.from_numpy(np.eye(4) if M is None else M.copy())
    if return_distances:
        out.update(accuracy_distances=dist["accuracy"], completeness_distances=dist["completeness"], pred_points=Pa[part_a])
    return out


def format_evaluation(result):
    """evaluate_reconstruction's result as the lines of a small table"""
    lines = [f"{'points':<22}{result['n_pred']:>12} predicted {result['n_gt']:>12} ground truth",
             f"{'accuracy (mean)':<22}{result['accuracy']:>12.6f}   median {result['accuracy_median']:.6f}",
             f"{'completeness (mean)':<22}{result['completeness']:>12.6f}   median {result['completeness_median']:.6f}",
             f"{'chamfer':<22}{result['chamfer']:>12.6f}"]
    for T, p, r, f in zip(result["thresholds"], result["precision"], result["recall"], result["fscore"]):
        lines.append(f"{'at ' + format(T, 'g'):<22}precision {p:.4f}   recall {r:.4f}   fscore {f:.4f}")
    return lines


# ---- rendering the cloud from any camera (csrc/render.hip) -------------------------------------------------------------------
def _is_int(x):
    return not isinstance(x, bool) and isinstance(x, (int, np.integer))


def _render_args(splat_radius, background, size, default_size):
    """(radius, 0xRRGGBB, (OH, OW)), or ValueError: before any launch"""
    if not (_is_int(splat_radius) and 0 <= splat_radius <= 8):
        raise ValueError(f"splat_radius must be an integer in [0, 8], got {splat_radius!r}")
    try:
        bg = list(background)
    except TypeError:
        bg = None
    if bg is None or len(bg) != 3 or not all(_is_int(b) and 0 <= b <= 255 for b in bg):
        raise ValueError(f"background must be three integers in [0, 255], got {background!r}")
    if size is None:
        size = default_size
    try:
        size = list(size)
    except TypeError:
        size = []
    if len(size) != 2 or not all(_is_int(s) and s > 0 for s in size):
        raise ValueError(f"size must be two positive integers (OH, OW), got {size!r}")
    return int(splat_radius), (int(bg[0]) << 16) | (int(bg[1]) << 8) | int(bg[2]), (int(size[0]), int(size[1]))


def _render_cameras(pred_dict, camera_poses, intrinsics, n):
    """(poses fp32 [M,4,4] on the host's or the device's side as given, K fp32 [M,3,3] or None = estimate), or ValueError"""
    if camera_poses is None:
        poses = pred_dict.get("camera_poses")
        if not torch.is_tensor(poses) or tuple(poses.shape) != (1, n, 4, 4):
            raise ValueError(f"camera_poses=None takes pred_dict['camera_poses'] [1,N,4,4] with N = {n}, got "
                             f"{tuple(poses.shape) if torch.is_tensor(poses) else type(poses).__name__}")
    else:
        poses = camera_poses
        if intrinsics is None:
            raise ValueError("explicit camera_poses need intrinsics ([3,3] or [M,3,3]): for the scene's own cameras pass "
                             "estimate_intrinsics(pred)[0, i]")
    ok = torch.is_tensor(poses) and poses.is_floating_point() and poses.dim() in (3, 4) and tuple(poses.shape[-2:]) == (4, 4) and \
        (poses.dim() == 3 or poses.shape[0] == 1) and poses.shape[-3] >= 1
    if not ok:
        raise ValueError(f"camera_poses: a floating-point tensor [M,4,4] or [1,M,4,4] expected, got "
                         f"{(poses.dtype, tuple(poses.shape)) if torch.is_tensor(poses) else type(poses).__name__}")
    poses = poses.detach().reshape(-1, 4, 4)
    m = poses.shape[0]
    if m > 65535:
        raise ValueError(f"at most 65535 target cameras per call, got {m}")
    if intrinsics is None:
        return poses, None
    K = intrinsics
    if not (torch.is_tensor(K) and K.is_floating_point() and tuple(K.shape) in ((3, 3), (m, 3, 3), (1, m, 3, 3))):
        raise ValueError(f"intrinsics: a floating-point tensor [3,3], [M,3,3] or [1,M,3,3] with M = {m} expected, got "
                         f"{(K.dtype, tuple(K.shape)) if torch.is_tensor(K) else type(K).__name__}")
    K = K.detach().float()
    return poses, (K.expand(m, 3, 3) if K.dim() == 2 else K.reshape(m, 3, 3))


def _render_skip(exclude_view, m, n):
    """the source view left out of every target as m ints, or None"""
    if exclude_view is None:
        return None
    if isinstance(exclude_view, str):
        if exclude_view != "self":
            raise ValueError(f"exclude_view: None, 'self' or {m} integers expected, got {exclude_view!r}")
        if m != n:
            raise ValueError(f"exclude_view='self' needs as many target cameras as source views, got {m} and {n}")
        return list(range(n))
    try:
        skip = exclude_view.tolist() if hasattr(exclude_view, "tolist") else list(exclude_view)
    except TypeError:
        skip = None
    if skip is None or len(skip) != m or not all(_is_int(s) and -2 ** 31 <= s < 2 ** 31 for s in skip):
        raise ValueError(f"exclude_view: None, 'self' or {m} integers expected, got {exclude_view!r}")
    return [int(s) for s in skip]


def render_point_cloud(pred_dict, camera_poses=None, intrinsics=None, size=None, splat_radius=0, exclude_view=None,
                       background=(0, 0, 0), mask=None, conf_threshold=None, edge_rtol=None, edge_atol=None, filter_nan=True):
    """The cloud of a recon result seen from any camera, on the device (hip.cloud_render; include/g2vlm_hip.h and DESIGN.md 6l
    have the exact rule): every kept pixel's world point is projected into every target camera, drawn as a square of
    2 splat_radius + 1 pixels, and every target pixel keeps the nearest point that covers it (a z-buffer; equal depths go to the
    lower source pixel).  One source pixel per target pixel, no blending: `index` says which.
    The source pixels are those point_cloud_mask keeps under the same filter arguments; an explicit mask (bool / uint8 [N,H,W],
    e.g. point_cloud_mask(min_views=...)'s) replaces the filters.
    camera_poses: [M,4,4] or [1,M,4,4] camera-to-world; None takes the scene's own pred_dict["camera_poses"] (M = N).
    intrinsics: [3,3] (one K for every target), [M,3,3] or [1,M,3,3], used as given (never rescaled to `size`); None is allowed
    only with camera_poses=None and takes estimate_intrinsics over the same mask.  size = (OH, OW), default (H, W).
    exclude_view: None, "self" (target m leaves out source view m: leave-one-out re-rendering, needs M == N) or M integers (the
    source view each target leaves out; -1 for none).  background: (r, g, b) bytes for the pixels nothing covers.
    Returns, on the device, dict(color uint8 [M,OH,OW,3] - the bytes the PLY export writes for the source pixel -, depth fp32
    [M,OH,OW] (0 where nothing lands), index int32 [M,OH,OW] = the flat source pixel (i H + y) W + x or -1, intrinsics fp32
    [M,3,3]).  ValueError for every bad argument, before any launch."""
    from . import hip
    if mask is not None:
        points, local, _, images, _ = _cloud_inputs(pred_dict, None, None, None, need_images=True)
        conf = logit = None
    else:
        points, local, conf, images, logit = _cloud_inputs(pred_dict, conf_threshold, edge_rtol, edge_atol, need_images=True)
    n, h, w = points.shape[:3]
    radius, bg, (oh, ow) = _render_args(splat_radius, background, size, (h, w))
    poses, K = _render_cameras(pred_dict, camera_poses, intrinsics, n)
    m = poses.shape[0]
    if m * oh * ow > 2 ** 31 - 1:
        raise ValueError(f"{m} targets of {oh} x {ow} are more than 2^31 - 1 pixels: render fewer cameras per call")
    skip = _render_skip(exclude_view, m, n)
    if mask is not None:
        base = _voxel_mask(mask, points.shape[:3], points.device)
    else:
        base = _cloud_mask_u8(points, local, conf, logit, edge_rtol, edge_atol, filter_nan)
    if K is None:
        K, _ = hip.intrinsics_lsq(local, base)
    dev = points.device
    K = K.to(dev).contiguous()
    poses = poses.to(dev).float().contiguous()
    if skip is not None:
        skip = torch.tensor(skip, dtype=torch.int32).to(dev)
    color, depth, index = hip.cloud_render(points, images, base, poses, K, (oh, ow), radius, bg, skip)
    return dict(color=color, depth=depth, index=index, intrinsics=K)


def orbit_poses(pred_dict, frames=36, mask=None):
    """A turntable through the scene's own cameras: fp32 [frames,4,4] camera-to-world (a host tensor; fp64 arithmetic on the
    host, rounded once).  Centre c = the per-axis median of the kept finite world points (mask: bool / uint8 [N,H,W], None = all);
    up = the normalised mean of the cameras' negated y axes (column 1 of a pose points down); height h = the mean of
    (centre_i - c) . up and radius rho = the mean norm of the part of (centre_i - c) perpendicular to up.  Frame k stands at
    c + h up + rho (cos a e1 + sin a e2), a = 2 pi k / frames, e1 = the normalised perpendicular part of camera 0's offset - frame 0
    has camera 0's azimuth -, e2 = up x e1, and looks at c: the rotation's columns are right = forward x up (normalised), down =
    forward x right, forward.  ValueError if no point is kept or up or the orbit is degenerate."""
    if not (_is_int(frames) and frames >= 1):
        raise ValueError(f"frames must be an integer >= 1, got {frames!r}")
    points = pred_dict["points"]
    if points.dim() != 5 or points.shape[0] != 1 or points.shape[-1] != 3:
        raise ValueError(f"points [1,N,H,W,3] expected, got {tuple(points.shape)}")
    n = points.shape[1]
    poses = pred_dict.get("camera_poses")
    if not torch.is_tensor(poses) or tuple(poses.shape) != (1, n, 4, 4):
        raise ValueError(f"orbit_poses needs pred_dict['camera_poses'] [1,N,4,4] with N = {n}, got "
                         f"{tuple(poses.shape) if torch.is_tensor(poses) else type(poses).__name__}")
    p = points[0].detach().double().cpu().numpy()
    keep = np.isfinite(p).all(-1)
    if mask is not None:
        keep &= _voxel_mask(mask, points.shape[1:4], "cpu").numpy() != 0
    if not keep.any():
        raise ValueError("orbit_poses: no finite point is kept")
    c = np.median(p[keep], axis=0)
    cam = poses[0].detach().double().cpu().numpy()
    up = -cam[:, :3, 1].mean(0)
    norm = np.linalg.norm(up)
    if not (np.isfinite(norm) and norm > 1e-9):
        raise ValueError("orbit_poses: the cameras' up directions cancel (or are not finite): no turntable axis")
    up = up / norm
    off = cam[:, :3, 3] - c
    along = off @ up
    perp = off - along[:, None] * up
    h, rho = along.mean(), np.linalg.norm(perp, axis=1).mean()
    e1n = np.linalg.norm(perp[0])
    if not (np.isfinite(e1n) and e1n > 1e-9 and np.isfinite(h) and rho > 1e-9):
        raise ValueError("orbit_poses: camera 0 stands on the turntable's axis (or a pose is not finite): no azimuth to start from")
    e1 = perp[0] / e1n
    e2 = np.cross(up, e1)
    out = np.zeros((frames, 4, 4))
    for k in range(frames):
        a = 2.0 * np.pi * k / frames
        pos = c + h * up + rho * (np.cos(a) * e1 + np.sin(a) * e2)
        fwd = (c - pos) / np.linalg.norm(c - pos)
        right = np.cross(fwd, up)
        right /= np.linalg.norm(right)                       # rho > 0: forward is never parallel to up
        out[k, :3, 0], out[k, :3, 1], out[k, :3, 2], out[k, :3, 3], out[k, 3, 3] = right, np.cross(fwd, right), fwd, pos, 1.0
    return torch.from_numpy(out.astype(np.float32))


def save_rendered_views(render, directory, prefix="view"):
    """render_point_cloud's colour images as PNGs directory/prefix_000.png ... (Pillow); returns the paths"""
    from PIL import Image
    color = render["color"]
    if not torch.is_tensor(color) or color.dtype != torch.uint8 or color.dim() != 4 or color.shape[-1] != 3:
        raise ValueError("render['color']: uint8 [M,OH,OW,3] expected (render_point_cloud's result)")
    os.makedirs(directory, exist_ok=True)
    paths = []
    for k, img in enumerate(color.cpu().numpy()):
        paths.append(os.path.join(directory, f"{prefix}_{k:03d}.png"))
        Image.fromarray(img).save(paths[-1])
    return paths
