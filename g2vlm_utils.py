"""Top-level `g2vlm_utils` - the module name the reference's scripts import (reference inference_recon.py:15,
inference_chat.py:8, the notebook): `from g2vlm_utils import load_model_and_tokenizer, ...` works with this repository's
root on `sys.path` in place of the reference's.  The implementation lives in g2vlm_amd/g2vlm_utils.py; this file only
re-exports it under the reference's name (reference g2vlm_utils.py:31-149), with the filtered export that this project adds."""
from g2vlm_amd.g2vlm_utils import (LazySafetensors, add_special_tokens, align_points, build_model, build_transform,  # noqa: F401
                                   configs_from_dims, estimate_intrinsics, estimate_normals, evaluate_reconstruction,
                                   load_model_and_tokenizer, multiview_consistency, nearest_points, orbit_poses, pil_img2rgb,
                                   point_cloud_mask, process_conversation, reconstruct_mesh, render_point_cloud, save_mesh,
                                   save_normal_maps, save_ply_visualization, save_point_cloud, save_point_cloud_masked,
                                   save_point_cloud_normals, save_rendered_views, view_angle_mask, voxel_downsample)

__all__ = ["load_model_and_tokenizer", "build_transform", "process_conversation", "save_ply_visualization",
           "save_point_cloud", "point_cloud_mask", "estimate_intrinsics", "voxel_downsample", "multiview_consistency",
           "save_point_cloud_masked", "render_point_cloud", "orbit_poses", "save_rendered_views", "reconstruct_mesh", "save_mesh",
           "nearest_points", "align_points", "evaluate_reconstruction", "estimate_normals", "view_angle_mask",
           "save_point_cloud_normals", "save_normal_maps"]
