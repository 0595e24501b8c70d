"""Time the z-buffer rendering of the cloud (g2v_cloud_render: csrc/render.hip) on the synthetic floor-and-sphere scene of
tests/consistency_check.py: N source views of 518 x 518 into M target cameras of 518 x 518.  Needs the GPU; bench.py is a different
measurement and is not touched.

    python tools/bench_render.py [--views 8 32] [--targets 1 8] [--radii 0 1 2] [--out profiles/render_bench.json]
                                 [--stage-libs FILL.so FILL_SPLAT.so] [--kernel-only]

  kernel         device events around single calls of the entry point g2v_cloud_render (fill + splat + resolve, every output on,
                 outputs and workspace allocated once), warmed up: median, p10 and p90 of 30 calls
  launches       with --stage-libs: the same events around the entry point of two timing builds that stop after the first and after
                 the second launch (-DG2V_RENDER_STAGES=1 and =3 through build.build(extra_flags, out)), each measured in a child
                 process of its own; fill = the first, splat = second - first, resolve = kernel - second (differences of medians)
  wrapper        the same events around hip.cloud_render, which allocates the outputs and queries the workspace on every call
  torch          the same rule written in torch on the same device: elementwise projection, int64 keys, one
                 scatter_reduce_(..., "amin") over the expanded footprints per target, then the gathers; the same events and number
                 of calls; it is compared with the kernel before anything is timed and the tool stops if they differ
  self_check     render_point_cloud(pred, exclude_view="self", splat_radius=1) as a user calls it (mask, intrinsics fit, render,
                 allocation), host clock around work ending in a synchronise: tools/bench_cloud_export.py's rounds

--kernel-only measures `kernel` alone, without comparing outputs (a timing build writes none).  The A/B build without the plain
load before the atomic (-DG2V_RENDER_TEST_FIRST=0) is measured by running this tool with G2V_LIB_PATH pointing at it and --out
elsewhere."""
import argparse
import json
import os
import statistics
import subprocess
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
import render_check as rc  # noqa: E402
from g2vlm_amd import hip  # noqa: E402
from g2vlm_amd.g2vlm_utils import render_point_cloud  # noqa: E402

H, W, LAUNCHES, WARM, BG = base.H, base.W, 30, 5, 0x102030


def torch_rule(points, colors, mask, poses, K, OH, OW, radius, bg):
    """the rule in torch: separate elementwise kernels, so nothing fuses; -> (color uint8, depth fp32, index int32, landed)"""
    N, H, W = points.shape[:3]
    M = poses.shape[0]
    dev = points.device
    P = points.reshape(-1, 3)
    eligible = (mask.reshape(-1) != 0) & torch.isfinite(P).all(-1)
    p = torch.arange(N * H * W, device=dev, dtype=torch.int64)
    empty = torch.iinfo(torch.int64).max
    keys = torch.full((M, OH * OW), empty, dtype=torch.int64, device=dev)
    offs = [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]
    dy = torch.tensor([o[0] for o in offs], device=dev).view(-1, 1)
    dx = torch.tensor([o[1] for o in offs], device=dev).view(-1, 1)
    landed = 0
    for m in range(M):
        R, t, k = poses[m, :3, :3], poses[m, :3, 3], K[m]
        d0, d1, d2 = P[:, 0] - t[0], P[:, 1] - t[1], P[:, 2] - t[2]
        q = [(R[0, c] * d0 + R[1, c] * d1) + R[2, c] * d2 for c in range(3)]
        u = k[0, 0] * (q[0] / q[2]) + k[0, 2]
        v = k[1, 1] * (q[1] / q[2]) + k[1, 2]
        lands = eligible & (q[2] > 0) & torch.isfinite(q[2]) & (u >= 0) & (u < OW) & (v >= 0) & (v < OH)
        sel = lands.nonzero().squeeze(1)
        landed += sel.numel()
        x0, y0 = u[sel].long(), v[sel].long()
        key = (q[2][sel].view(torch.int32).long() << 32) | p[sel]
        tx, ty = x0.unsqueeze(0) + dx, y0.unsqueeze(0) + dy                     # the expanded footprints [(2r+1)^2, landed]
        ok = (tx >= 0) & (tx < OW) & (ty >= 0) & (ty < OH)
        keys[m].scatter_reduce_(0, (ty * OW + tx)[ok], key.unsqueeze(0).expand_as(ok)[ok], "amin")
    hit = keys != empty
    index = torch.where(hit, keys & 0xFFFFFFFF, torch.full_like(keys, -1))
    depth = torch.where(hit, (keys >> 32).int().view(torch.float32), torch.zeros((), device=dev))
    src = index.clamp(min=0)
    i, rem = src // (H * W), src % (H * W)
    chan = torch.stack([colors.reshape(N, 3, H * W)[i, c, rem] for c in range(3)], -1)
    color = (chan.double().clamp(0, 1) * 255).to(torch.uint8)
    back = torch.tensor([(bg >> 16) & 255, (bg >> 8) & 255, bg & 255], dtype=torch.uint8, device=dev)
    color = torch.where(hit.unsqueeze(-1), color, back)
    return color.view(M, OH, OW, 3), depth.view(M, OH, OW), index.int().view(M, OH, OW), landed


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


def tag(n, m, r):
    return f"{n}v_{m}t_r{r}"


def bench_views(n, targets, radii, kernel_only):
    s = cc.scene(n, H, W)
    points, colors = torch.from_numpy(s["points"]).cuda(), torch.from_numpy(rc.scene_colors(n, H, W)).cuda()
    mask = hip.cloud_mask(points, finite=True)
    out = []
    for m in targets:
        poses, K = (torch.from_numpy(a).cuda() for a in rc.targets(s, m, H, W))
        outs = (torch.empty((m, H, W, 3), dtype=torch.uint8, device="cuda"), torch.empty((m, H, W), dtype=torch.float32, device="cuda"),
                torch.empty((m, H, W), dtype=torch.int32, device="cuda"))
        ws = torch.empty(hip.cloud_render_workspace(m, H, W) // 8, dtype=torch.int64, device="cuda")
        fn, stream = hip.lib().g2v_cloud_render, hip._stream()
        for r in radii:
            def launch():
                assert fn(hip._p(points), hip._p(colors), hip._p(mask), n, H, W, hip._p(poses), hip._p(K), None, m, H, W, r, BG,
                          hip._p(outs[0]), hip._p(outs[1]), hip._p(outs[2]), hip._p(ws), ws.numel() * 8, stream) == 0

            res = dict(config=tag(n, m, r), views=n, targets=m, radius=r, height=H, width=W, key_bytes_per_target=8 * H * W)
            if not kernel_only:
                want = torch_rule(points, colors, mask, poses, K, H, W, r, BG)
                launch()
                torch.cuda.synchronize()
                if not all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs, want[:3])):
                    raise SystemExit(f"{res['config']}: the kernel and the torch form differ on {int((outs[2] != want[2]).sum())} indices")
                res.update(kernel_equals_torch_form=True, points_landed=want[3], splat_writes=want[3] * (2 * r + 1) ** 2,
                           covered=round(float((want[2] >= 0).float().mean()), 4))
                del want
            res["kernel"] = event_times(launch)
            if not kernel_only:
                res["wrapper"] = event_times(lambda: hip.cloud_render(points, colors, mask, poses, K, (H, W), r, BG))
                res["torch_form"] = event_times(lambda: torch_rule(points, colors, mask, poses, K, H, W, r, BG))
                res["torch_over_kernel"] = round(res["torch_form"]["median_ms"] / res["kernel"]["median_ms"], 1)
            out.append(res)
            print(res, file=sys.stderr, flush=True)
    self_check = None
    if not kernel_only and n == 8:
        pred = dict(points=points[None], local_points=torch.from_numpy(s["local"]).cuda()[None], camera_poses=torch.from_numpy(s["poses"]).cuda()[None],
                    images=colors[None], conf=None)
        self_check = base.rounds({"render_point_cloud_exclude_self_radius1": lambda: render_point_cloud(pred, exclude_view="self", splat_radius=1)})
    return out, self_check


def stage_times(libs, argv, tmp):
    """the entry point's medians under the two timing builds, each in a child process of its own: {config: median_ms} per build"""
    out = []
    for k, lib in enumerate(libs):
        path = os.path.join(tmp, f"stage{k}.json")
        subprocess.run([sys.executable, os.path.abspath(__file__), *argv, "--kernel-only", "--out", path], check=True,
                       env=dict(os.environ, G2V_LIB_PATH=os.path.abspath(lib)), stdout=subprocess.DEVNULL, timeout=600)
        out.append({c["config"]: c["kernel"]["median_ms"] for c in json.load(open(path))["configs"]})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--targets", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--radii", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    ap.add_argument("--stage-libs", nargs=2, default=None, metavar=("FILL", "FILL_SPLAT"))
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py measures on the GPU; there is none here")
    configs, self_check = [], None
    for n in a.views:
        res, sc = bench_views(n, a.targets, a.radii, a.kernel_only)
        configs += res
        self_check = self_check or sc
    if a.stage_libs:
        shapes = ["--views", *map(str, a.views), "--targets", *map(str, a.targets), "--radii", *map(str, a.radii)]
        with tempfile.TemporaryDirectory() as tmp:
            fill, fill_splat = stage_times(a.stage_libs, shapes, tmp)
        for c in configs:
            k = c["config"]
            c["launches"] = dict(fill_ms=round(fill[k], 4), splat_ms=round(fill_splat[k] - fill[k], 4),
                                 resolve_ms=round(c["kernel"]["median_ms"] - fill_splat[k], 4))
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]
    res = dict(what="z-buffer rendering of the cloud: g2v_cloud_render vs the same rule in torch",
               measured_on="1x MI355X (gfx950)" if arch == "gfx950" else "1x " + torch.cuda.get_device_name(0), arch=arch,
               library=os.path.basename(hip.LIB_PATH), kernel_only=a.kernel_only,
               method=f"kernel / wrapper / torch: device events around one call, {LAUNCHES} calls after {WARM} warm-ups; launches: differences of "
                      f"the medians of timing builds that stop after the first / second launch; self_check: median of {base.ROUNDS} rounds after "
                      f"{base.WARMUP} warm-ups, host clock around work ending in a synchronise", configs=configs)
    if self_check:
        res["self_check_8_views"] = self_check
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
