"""Drop-in counterpart of the reference's inference_recon.py (same flags), running on g2vlm_amd.
Fixes the reference's Namespace-as-path bug and sorts the folder listing.

Flags of this project's own, all off by default (without them main() does what the reference's does): --conf-threshold,
--edge-rtol, --edge-atol write the PLY through save_point_cloud's device filters; --intrinsics fits and prints a pinhole
matrix per view; --voxel-size (with --voxel-min-points) voxel-downsamples the cloud on the device before it is written;
--min-views, --max-in-front (with --consistency-rtol) add the multi-view consistency filter (point_cloud_mask);
--render-dir writes one PNG per input view, re-rendered from the OTHER views' points (render_point_cloud, under the filters given),
--render-orbit F adds F turntable frames there, --render-radius and --render-size set the splat half-width and the image size;
--mesh PATH also writes the reconstruction as a triangle mesh (save_mesh, under the filters given; --mesh-max-edge L drops triangles
with an edge longer than L); --evaluate GT.npy measures the reconstruction against a ground-truth cloud (evaluate_reconstruction, under
the filters given: a [N,H,W,3] array pixel-aligned with the views, or an unordered [M,3] cloud with --eval-align none) and prints
accuracy, completeness, Chamfer distance and precision / recall / F-score at every --eval-threshold T; --eval-max-distance D clips
the search, --eval-align sim3|none picks the alignment; --normals-ply PATH also writes the cloud with a surface normal per vertex
(save_point_cloud_normals, under the filters given) and --normal-maps DIR one normal-map PNG per view (save_normal_maps), with
--normal-step S the distance to the neighbours a normal is taken from (1..8), --normal-max-edge L the longest edge to a neighbour that
counts and --max-view-angle DEG (--normals-ply only) dropping the points seen at more than DEG degrees from their normal."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from g2vlm_utils import load_model_and_tokenizer, save_ply_visualization  # noqa: E402  (the reference's import line, inference_recon.py:15)

parser = argparse.ArgumentParser(description="Demo for 3D visualization")
parser.add_argument("--image_folder", type=str, default="examples/dl3dv/", help="Path to folder containing images")
parser.add_argument("--model_path", type=str, default="InternRobotics/G2VLM-2B-MoT")
parser.add_argument("--save_path", type=str, default="results/arkitscenes_results.ply")
parser.add_argument("--conf-threshold", type=float, default=None, metavar="P",
                    help="keep points whose confidence sigmoid(conf) exceeds P in (0,1); needs a checkpoint with a confidence head")
parser.add_argument("--edge-rtol", type=float, default=None, metavar="R",
                    help="drop depth discontinuities: 3x3 depth range / depth above R (0.03 is the usual choice)")
parser.add_argument("--edge-atol", type=float, default=None, metavar="A", help="drop depth discontinuities: 3x3 depth range above A")
parser.add_argument("--intrinsics", action="store_true", help="fit, print and return a pinhole matrix per view (pred['intrinsics'])")
parser.add_argument("--voxel-size", type=float, default=None, metavar="V",
                    help="voxel-downsample the cloud on the device: one vertex per occupied cell of a grid of spacing V")
parser.add_argument("--voxel-min-points", type=int, default=1, metavar="K", help="with --voxel-size: drop cells with fewer than K points")
parser.add_argument("--min-views", type=int, default=None, metavar="K",
                    help="keep a point only if at least K other views confirm it (its depth there agrees within --consistency-rtol)")
parser.add_argument("--max-in-front", type=int, default=None, metavar="M",
                    help="keep a point only if at most M other views see it floating in front of their surface")
parser.add_argument("--consistency-rtol", type=float, default=0.03, metavar="R", help="with --min-views / --max-in-front: the relative depth tolerance")
parser.add_argument("--render-dir", type=str, default=None, metavar="DIR",
                    help="write view_000.png ...: every input view re-rendered from the other views' points (leave-one-out)")
parser.add_argument("--render-orbit", type=int, default=None, metavar="F",
                    help="with --render-dir: also write orbit_000.png ..., F turntable frames through the scene's own cameras")
parser.add_argument("--render-radius", type=int, default=1, metavar="R", help="with --render-dir: a point is drawn as a square of 2R+1 pixels (0..8)")
parser.add_argument("--render-size", type=int, nargs=2, default=None, metavar=("H", "W"), help="with --render-dir: the size of the rendered images")
parser.add_argument("--mesh", type=str, default=None, metavar="PATH",
                    help="also write the reconstruction as a triangle mesh (binary PLY with faces): every view's pixel grid triangulated")
parser.add_argument("--mesh-max-edge", type=float, default=None, metavar="L", help="with --mesh: drop triangles with an edge longer than L")
parser.add_argument("--evaluate", type=str, default=None, metavar="GT.npy",
                    help="measure the reconstruction against ground-truth points: a .npy of shape [N,H,W,3] (pixel-aligned) or [M,3]")
parser.add_argument("--eval-threshold", type=float, action="append", default=None, metavar="T",
                    help="with --evaluate: a distance at which precision / recall / F-score are reported (repeatable; default 0.05)")
parser.add_argument("--eval-max-distance", type=float, default=None, metavar="D",
                    help="with --evaluate: neighbours farther than D do not count (such points are misses, and enter the means with D)")
parser.add_argument("--eval-align", type=str, default=None, choices=("sim3", "none"),
                    help="with --evaluate: fit a similarity on the pixels valid on both sides (default for [N,H,W,3]) or compare as is")


parser.add_argument("--normals-ply", type=str, default=None, metavar="PATH",
                    help="also write the cloud with a surface normal per vertex (binary PLY with nx ny nz)")
parser.add_argument("--normal-maps", type=str, default=None, metavar="DIR", help="write normal_000.png ...: a camera-frame normal map per input view")
parser.add_argument("--normal-step", type=int, default=None, metavar="S",
                    help="with --normals-ply / --normal-maps: the distance in pixels to the neighbours a normal is taken from (1..8, default 1)")
parser.add_argument("--normal-max-edge", type=float, default=None, metavar="L",
                    help="with --normals-ply / --normal-maps: neighbours farther than L from the pixel's point do not count")
parser.add_argument("--max-view-angle", type=float, default=None, metavar="DEG",
                    help="with --normals-ply: drop points seen at more than DEG degrees from their normal, in (0, 90]")


def check_normal_flags(args):
    """refuses --normal-step / --normal-max-edge / --max-view-angle without an output that uses them, and values out of range"""
    if args.normals_ply is None and args.normal_maps is None:
        if args.normal_step is not None or args.normal_max_edge is not None or args.max_view_angle is not None:
            parser.error("--normal-step, --normal-max-edge and --max-view-angle need --normals-ply PATH or --normal-maps DIR")
    if args.normal_step is not None and not 1 <= args.normal_step <= 8:
        parser.error("--normal-step S must be in 1..8")
    if args.normal_max_edge is not None and not args.normal_max_edge >= 0:
        parser.error("--normal-max-edge L must be >= 0")
    if args.max_view_angle is not None and (args.normals_ply is None or not 0 < args.max_view_angle <= 90):
        parser.error("--max-view-angle DEG needs --normals-ply and DEG in (0, 90]")


def write_normals(pred, args):
    """--normals-ply / --normal-maps: under the filters given on the command line; with no filter flag at all, the functions' defaults
    (edge_rtol = 0.03)"""
    from g2vlm_utils import point_cloud_mask, save_normal_maps, save_point_cloud_normals
    kw = dict(step=args.normal_step or 1, max_edge=args.normal_max_edge)
    if args.min_views is not None or args.max_in_front is not None or args.edge_rtol is not None or args.edge_atol is not None \
            or args.conf_threshold is not None:
        consistency = {}
        if args.min_views is not None or args.max_in_front is not None:
            consistency = dict(min_views=args.min_views, max_in_front=args.max_in_front, depth_rtol=args.consistency_rtol)
        kw["mask"] = point_cloud_mask(pred, conf_threshold=args.conf_threshold, edge_rtol=args.edge_rtol, edge_atol=args.edge_atol, **consistency)
    if args.normals_ply is not None:
        save_point_cloud_normals(pred, args.normals_ply, max_view_angle=args.max_view_angle, **kw)
    if args.normal_maps is not None:
        paths = save_normal_maps(pred, args.normal_maps, **kw)
        print(f"{args.normal_maps}: {len(paths)} normal maps")


def check_evaluation_flags(args):
    """refuses malformed --evaluate / --eval-* values (parser.error) and returns the ground truth array or None"""
    import numpy as np
    if args.evaluate is None:
        if args.eval_threshold is not None or args.eval_max_distance is not None or args.eval_align is not None:
            parser.error("--eval-threshold, --eval-max-distance and --eval-align need --evaluate GT.npy")
        return None
    for t in args.eval_threshold or ():
        if not (t > 0 and np.isfinite(t)):
            parser.error("--eval-threshold T must be finite and > 0")
    if args.eval_max_distance is not None and not args.eval_max_distance >= 0:
        parser.error("--eval-max-distance D must be >= 0")
    try:
        gt = np.load(args.evaluate, allow_pickle=False)
    except (OSError, ValueError) as e:
        parser.error(f"--evaluate {args.evaluate}: {e}")
    if gt.dtype.kind != "f" or gt.ndim not in (2, 4) or gt.shape[-1] != 3:
        parser.error(f"--evaluate {args.evaluate}: a float array [N,H,W,3] or [M,3] expected, got {gt.dtype} {gt.shape}")
    if gt.ndim == 2 and args.eval_align == "sim3":
        parser.error("--eval-align sim3 needs pixel-aligned ground truth [N,H,W,3]")
    return gt


def evaluate(pred, args, gt):
    """--evaluate: the table, under the filters given on the command line"""
    import torch
    from g2vlm_utils import evaluate_reconstruction, point_cloud_mask
    from g2vlm_amd.g2vlm_utils import format_evaluation
    consistency = {}
    if args.min_views is not None or args.max_in_front is not None:
        consistency = dict(min_views=args.min_views, max_in_front=args.max_in_front, depth_rtol=args.consistency_rtol)
    mask = point_cloud_mask(pred, conf_threshold=args.conf_threshold, edge_rtol=args.edge_rtol, edge_atol=args.edge_atol, **consistency)
    align = args.eval_align or ("sim3" if gt.ndim == 4 else "none")
    result = evaluate_reconstruction(pred, torch.from_numpy(gt).float(), align=align, thresholds=tuple(args.eval_threshold or (0.05,)),
                                     max_distance=args.eval_max_distance, mask=mask)
    print(f"{args.evaluate}: align {align}")
    for line in format_evaluation(result):
        print(line)
    return result


def write_mesh(pred, args):
    """--mesh: the mesh under the filters given on the command line; with no filter flag at all, save_mesh's defaults (edge_rtol = 0.03)"""
    from g2vlm_utils import point_cloud_mask, save_mesh
    if args.min_views is not None or args.max_in_front is not None or args.edge_rtol is not None or args.edge_atol is not None \
            or args.conf_threshold is not None:
        consistency = {}
        if args.min_views is not None or args.max_in_front is not None:
            consistency = dict(min_views=args.min_views, max_in_front=args.max_in_front, depth_rtol=args.consistency_rtol)
        mask = point_cloud_mask(pred, conf_threshold=args.conf_threshold, edge_rtol=args.edge_rtol, edge_atol=args.edge_atol, **consistency)
        return save_mesh(pred, args.mesh, mask=mask, max_edge=args.mesh_max_edge)
    return save_mesh(pred, args.mesh, max_edge=args.mesh_max_edge)


def render_views(pred, args):
    """--render-dir / --render-orbit: the PNGs, under the filters given on the command line"""
    from g2vlm_utils import estimate_intrinsics, orbit_poses, point_cloud_mask, render_point_cloud, save_rendered_views
    consistency = {}
    if args.min_views is not None or args.max_in_front is not None:
        consistency = dict(min_views=args.min_views, max_in_front=args.max_in_front, depth_rtol=args.consistency_rtol)
    mask = point_cloud_mask(pred, conf_threshold=args.conf_threshold, edge_rtol=args.edge_rtol, edge_atol=args.edge_atol, **consistency)
    size = None if args.render_size is None else tuple(args.render_size)
    views = render_point_cloud(pred, size=size, splat_radius=args.render_radius, exclude_view="self", mask=mask)
    paths = save_rendered_views(views, args.render_dir, prefix="view")
    if args.render_orbit is not None:
        K = estimate_intrinsics(pred, mask)[0, 0]
        orbit = render_point_cloud(pred, camera_poses=orbit_poses(pred, args.render_orbit, mask=mask), intrinsics=K, size=size,
                                   splat_radius=args.render_radius, mask=mask)
        paths += save_rendered_views(orbit, args.render_dir, prefix="orbit")
    print(f"{args.render_dir}: {len(paths)} rendered images")


def main(argv=None):
    args = parser.parse_args(argv)
    if args.render_orbit is not None and (args.render_dir is None or args.render_orbit < 1):
        parser.error("--render-orbit F needs --render-dir and F >= 1")
    if not 0 <= args.render_radius <= 8:
        parser.error("--render-radius must be in 0..8")
    if args.mesh_max_edge is not None and (args.mesh is None or not args.mesh_max_edge >= 0):
        parser.error("--mesh-max-edge L needs --mesh and L >= 0")
    check_normal_flags(args)
    gt = check_evaluation_flags(args)
    names =sorted(n for n in os.listdir(args.image_folder) if n.lower().endswith((".png", ".jpg", ".jpeg")))
    image_names = [os.path.join(args.image_folder, n) for n in names]
    print(image_names)
    model, tokenizer, new_token_ids, vit_image_transform, dino_transform = load_model_and_tokenizer(args.model_path)
    pred = model.recon(tokenizer, new_token_ids, dino_transform, image_names)
    filtered = args.conf_threshold is not None or args.edge_rtol is not None or args.edge_atol is not None
    if args.min_views is not None or args.max_in_front is not None:
        from g2vlm_utils import point_cloud_mask, save_point_cloud_masked
        mask = point_cloud_mask(pred, conf_threshold=args.conf_threshold, edge_rtol=args.edge_rtol, edge_atol=args.edge_atol,
                                min_views=args.min_views, max_in_front=args.max_in_front, depth_rtol=args.consistency_rtol)
        save_point_cloud_masked(pred, args.save_path, mask, voxel_size=args.voxel_size, min_points=args.voxel_min_points)
    elif filtered or args.voxel_size is not None:
        from g2vlm_utils import save_point_cloud
        save_point_cloud(pred, args.save_path, conf_threshold=args.conf_threshold, edge_rtol=args.edge_rtol, edge_atol=args.edge_atol,
                         voxel_size=args.voxel_size, min_points=args.voxel_min_points)
    else:
        save_ply_visualization(pred, args.save_path)
    if args.render_dir is not None:
        render_views(pred, args)
    if args.mesh is not None:
        write_mesh(pred, args)
    if args.normals_ply is not None or args.normal_maps is not None:
        write_normals(pred, args)
    if gt is not None:
        pred["evaluation"] = evaluate(pred, args, gt)
    if args.intrinsics:
        from g2vlm_utils import estimate_intrinsics
        # over every valid pixel: X/Z and Y/Z of a local point (xy z, z) do not depend on its depth, so the depth filters have
        # nothing to remove from this fit
        pred["intrinsics"] = estimate_intrinsics(pred)
        for i, k in enumerate(pred["intrinsics"][0].cpu().tolist()):
            print(f"view {i}: K = {k}")
    return pred


if __name__ == "__main__":
    main()
