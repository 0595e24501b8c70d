"""Time the multi-view consistency filter (g2v_cloud_consistency: csrc/consistency.hip) on the synthetic floor-and-sphere scene of
tests/consistency_check.py at N views of 518 x 518.  Needs the GPU; bench.py is a different measurement and is not touched.

    python tools/bench_consistency.py [--views 8 32] [--out profiles/consistency_bench.json]

  kernel         device events around single calls of the entry point g2v_cloud_consistency (prepass + main kernel, every output on,
                 outputs and workspace allocated once), warmed up: median, p10 and p90 of 30 calls; and back to back, 20 calls
                 between two events, which leaves no idle queue inside the interval: the rates (projections and gathered bytes per
                 second, 4 bytes per projection that lands inside a view) are taken from that one
  wrapper        the same events around hip.cloud_consistency, which allocates the outputs and queries the workspace on every call
  torch          the same rule written in torch on the same device (one pass per target view over [N,H,W] temporaries), the same
                 events and number of calls; it is compared with the kernel before anything is timed and the tool stops if they differ
  export         save_point_cloud_masked(point_cloud_mask(min_views=1, max_in_front=0)) against save_point_cloud(edge_rtol=None), the
                 export without the filter: tools/bench_cloud_export.py's alternating rounds

A second build with another tile shape (-DG2V_CONSISTENCY_TILE_W=16 -DG2V_CONSISTENCY_TILE_H=16 through build.build(extra_flags,
out)) is measured by running this tool with G2V_LIB_PATH pointing at it and --out elsewhere."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_cloud_export as base  # noqa: E402
import consistency_check as cc  # noqa: E402
from g2vlm_amd import hip  # noqa: E402
from g2vlm_amd.g2vlm_utils import point_cloud_mask, save_point_cloud, save_point_cloud_masked  # noqa: E402

H, W, LAUNCHES, WARM = base.H, base.W, 30, 5


def torch_rule(points, local, mask, poses, K, rtol):
    """the rule in torch: separate elementwise kernels, so nothing fuses; -> (agree uint8, in_front uint8, inside projections)"""
    N, H, W = points.shape[:3]
    keep = mask != 0
    eligible = keep & torch.isfinite(points).all(-1)
    z = local[..., 2]
    plane = torch.where(keep & torch.isfinite(z) & (z > 0), z, torch.full_like(z, float("nan")))
    agree = torch.zeros(points.shape[:3], dtype=torch.int32, device=points.device)
    front = torch.zeros_like(agree)
    views = torch.arange(N, device=points.device).view(N, 1, 1)
    rt = torch.tensor(rtol, dtype=torch.float32, device=points.device)
    inside_total = 0
    for j in range(N):
        R, t, k = poses[j, :3, :3], poses[j, :3, 3], K[j]
        d0, d1, d2 = points[..., 0] - t[0], points[..., 1] - t[1], points[..., 2] - t[2]
        q = [(R[0, c] * d0 + R[1, c] * d1) + R[2, c] * d2 for c in range(3)]
        u = k[0, 0] * (q[0] / q[2]) + k[0, 2]
        v = k[1, 1] * (q[1] / q[2]) + k[1, 2]
        inside = (q[2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H) & eligible & (views != j)
        x = torch.where(inside, u, torch.zeros_like(u)).long()
        y = torch.where(inside, v, torch.zeros_like(v)).long()
        zt = plane[j][y, x]
        tol, diff = rt * zt, q[2] - zt
        agree += (inside & (diff.abs() <= tol)).int()
        front += (inside & (diff < -tol)).int()
        inside_total += inside.sum()
    return agree.to(torch.uint8), front.to(torch.uint8), int(inside_total)


def percentiles(ms):
    ms = sorted(ms)
    return dict(median_ms=round(statistics.median(ms), 4), p10_ms=round(ms[len(ms) // 10], 4), p90_ms=round(ms[(len(ms) * 9) // 10], 4), runs=len(ms))


def event_times(fn):
    out = []
    for r in range(WARM + LAUNCHES):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r >= WARM:
            out.append(a.elapsed_time(b))
    return percentiles(out)


def bench_size(n, tmp):
    s = cc.scene(n, H, W)
    t = {k: torch.from_numpy(s[k]).cuda() for k in ("points", "local", "poses", "K")}
    mask = hip.cloud_mask(t["points"], finite=True)
    args = (t["points"], t["local"], mask, t["poses"], t["K"], 0.03)
    agree, in_front, _, pairs = hip.cloud_consistency(*args, 1, 0, pairs=True)
    ta, tf, inside = torch_rule(*args)
    if not (torch.equal(agree, ta) and torch.equal(in_front, tf)):
        raise SystemExit(f"{n} views: the kernel and the torch form differ on {int(((agree != ta) | (in_front != tf)).sum())} pixels")
    assert int(pairs[..., 0].sum()) == int(agree.sum(dtype=torch.int64)) and int(pairs[..., 1].sum()) == int(in_front.sum(dtype=torch.int64))
    # the entry point itself, outputs and workspace allocated once: nothing but the two launches lies between the events
    out = [torch.empty((n, H, W), dtype=torch.uint8, device="cuda") for _ in range(3)]
    pair_out = torch.empty((n, n, 2), dtype=torch.int32, device="cuda")
    ws = torch.empty(hip.cloud_consistency_workspace(n, H, W), dtype=torch.uint8, device="cuda")
    fn, stream = hip.lib().g2v_cloud_consistency, hip._stream()
    ptrs = [hip._p(x) for x in (t["points"], t["local"], mask, t["poses"], t["K"])]
    outs = [hip._p(out[0]), hip._p(out[1]), hip._p(pair_out), hip._p(out[2]), hip._p(ws), ws.numel(), stream]

    def launch():
        assert fn(*ptrs, n, H, W, 0.03, 1, 0, *outs) == 0

    launch()
    assert torch.equal(out[0], agree) and torch.equal(out[1], in_front) and torch.equal(pair_out, pairs)
    kernel = event_times(launch)
    kernel["back_to_back_ms"] = round(base.kernel_time(launch), 4)           # 20 calls between two events: no idle queue between them
    wrapper = event_times(lambda: hip.cloud_consistency(*args, 1, 0, pairs=True))
    torch_form = event_times(lambda: torch_rule(*args))
    rng = np.random.default_rng(0)
    pred = dict(points=t["points"][None], local_points=t["local"][None], camera_poses=t["poses"][None], conf=None,
                images=torch.from_numpy(rng.random((1, n, 3, H, W), np.float32)).cuda())
    f = {k: os.path.join(tmp, k + ".ply") for k in ("filtered", "plain")}

    def filtered():
        return save_point_cloud_masked(pred, f["filtered"], point_cloud_mask(pred, min_views=1, max_in_front=0, intrinsics=t["K"]), verbose=False)

    kept, plain = filtered()["num_points"], save_point_cloud(pred, f["plain"], edge_rtol=None, verbose=False)["num_points"]
    calls = base.rounds({"export_with_filter": filtered, "export_without_filter": lambda: save_point_cloud(pred, f["plain"], edge_rtol=None, verbose=False)})
    proj = n * (n - 1) * H * W
    sec = kernel["back_to_back_ms"] * 1e-3
    return dict(views=n, height=H, width=W, projections=proj, projections_inside=inside, kernel=kernel, wrapper=wrapper, torch_form=torch_form,
                torch_over_kernel=round(torch_form["median_ms"] / kernel["median_ms"], 1),
                torch_over_wrapper=round(torch_form["median_ms"] / wrapper["median_ms"], 1), kernel_equals_torch_form=True,
                projections_per_s=round(proj / sec), gathered_bytes_per_s=round(4 * inside / sec), depth_plane_bytes_per_view=4 * H * W,
                points_kept_with_filter=kept, points_kept_without=plain, calls=calls)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_consistency.py measures on the GPU; there is none here")
    ram = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=ram) as tmp:
        sizes = []
        for n in a.views:
            sizes.append(bench_size(n, tmp))
            print(f"{n} views: {sizes[-1]}", file=sys.stderr, flush=True)
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]
    res = dict(what="multi-view consistency filter: g2v_cloud_consistency vs the same rule in torch, and the filtered export vs the unfiltered one",
               measured_on="1x MI355X (gfx950)" if arch == "gfx950" else "1x " + torch.cuda.get_device_name(0), arch=arch,
               library=os.path.basename(hip.LIB_PATH), ram_backed_dir=ram is not None,
               method=f"kernel / wrapper / torch: device events around one call, {LAUNCHES} calls after {WARM} warm-ups; back to back: "
                      f"{base.KERNEL_LAUNCHES} calls between two events, median of {base.ROUNDS} such rounds, per call; export: median of {base.ROUNDS} "
                      f"rounds after {base.WARMUP} warm-ups, variants alternated, host clock around work ending in a synchronise", sizes=sizes)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
