"""Time the point-cloud export: the device path (g2vlm_utils.save_point_cloud: csrc/cloud.hip mask + compaction, one copy of the
kept records, one write) against the host path (save_ply_visualization's: two full copies to the host, numpy mask and packing),
and the three kernels of csrc/cloud.hip alone.  Needs the GPU; bench.py is a different measurement and is not touched.

    python tools/bench_cloud_export.py [--views 8 32] [--out profiles/cloud_export_bench.json]

Synthetic pred_dicts of N views of 518 x 518: a pinhole camera over smooth depth with steps (so that the edge filter has edges to
find), a sprinkle of NaN points.  Files go to a RAM-backed directory, so that no disk is timed.  Per size, 3 warm-ups and then 10
timed rounds; a round runs every variant once, in turn, so that drift on a shared host hits all alike; the median is reported with
the extremes.  Call times are host clocks around work that ends in a device synchronise; kernel times are device events around
20 launches.  Before anything is timed the files of the two paths are compared byte for byte.

  (a) filter_nan only:   save_point_cloud(edge_rtol=None) | the host PLY path (save_ply_visualization without its PNG by-product)
                         | save_ply_visualization as it is (PNG grid included), for the record
  (b) edge_rtol = 0.03:  save_point_cloud | the same filter on the host (torch max_pool2d on the CPU, as the reference's depth_edge)
  (c) kernels alone:     g2v_cloud_mask (FINITE + EDGE_RTOL), g2v_cloud_compact, g2v_intrinsics_lsq, with the bytes each has to move
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from g2vlm_amd import hip, host  # noqa: E402
from g2vlm_amd.g2vlm_utils import save_ply_visualization, save_point_cloud  # noqa: E402

H = W = 518
WARMUP, ROUNDS, KERNEL_LAUNCHES = 3, 10, 20


def synthetic_pred(n, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    local = torch.empty((n, H, W, 3))
    for i in range(n):
        z = 2.0 + 0.002 * xx + 0.001 * yy + 0.2 * torch.sin(xx / 40 + i) * torch.cos(yy / 55)
        for _ in range(6):                                   # boxes in front of the surface: depth steps
            x0, y0 = int(torch.randint(0, W - 80, (1,), generator=g)), int(torch.randint(0, H - 80, (1,), generator=g))
            z[y0:y0 + 80, x0:x0 + 80] -= 0.5
        a, b = (xx + 0.5 - 0.52 * W) / (0.9 * W), (yy + 0.5 - 0.47 * H) / (0.85 * W)
        local[i] = torch.stack([a * z, b * z, z], -1)
    points = local + torch.arange(n, dtype=torch.float32).view(n, 1, 1, 1) * 0.1
    points[torch.rand((n, H, W), generator=g) < 0.001] = float("nan")
    images = torch.rand((n, 3, H, W), generator=g)
    return dict(points=points.unsqueeze(0).to(device), local_points=local.unsqueeze(0).to(device), conf=None,
                images=images.unsqueeze(0).to(device))


def host_ply(pred, path, edge_rtol=None):
    """save_ply_visualization's PLY path without the PNG grid: copy points and images to the host, mask and pack in numpy.
    edge_rtol: the reference's depth_edge on the host (torch CPU max_pool2d) on top."""
    images = pred["images"][0].detach().float().cpu()
    pts = pred["points"][0].detach().float().cpu()
    p = pts.numpy().reshape(-1, 3)
    c = images.permute(0, 2, 3, 1).numpy().reshape(-1, 3)
    ok = ~(np.isnan(p).any(1) | np.isinf(p).any(1))
    if edge_rtol is not None:
        d = pred["local_points"][0, ..., 2].detach().float().cpu().unsqueeze(1)
        mp = torch.nn.functional.max_pool2d
        diff = mp(d, 3, stride=1, padding=1) + mp(-d, 3, stride=1, padding=1)
        ok &= ~((diff / d).nan_to_num_() > edge_rtol).numpy().reshape(-1)
    host.write_ply_binary(path, p[ok], c[ok])


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def rounds(variants):
    """{name: fn} -> {name: {median_ms, min_ms, max_ms}}; every round runs every variant once, in turn"""
    times = {k: [] for k in variants}
    for r in range(WARMUP + ROUNDS):
        for k, fn in variants.items():
            t = timed(fn)
            if r >= WARMUP:
                times[k].append(t)
    return {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for k, v in times.items()}


def kernel_time(launch):
    """median over ROUNDS of (device-event time of KERNEL_LAUNCHES launches) / KERNEL_LAUNCHES, in ms"""
    out = []
    for r in range(WARMUP + ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(KERNEL_LAUNCHES):
            launch()
        b.record()
        b.synchronize()
        if r >= WARMUP:
            out.append(a.elapsed_time(b) / KERNEL_LAUNCHES)
    return statistics.median(out)


def bench_size(n, tmp):
    dev = torch.device("cuda")
    pred = synthetic_pred(n, dev)
    pixels = n * H * W
    f = {k: os.path.join(tmp, k + ".ply") for k in ("dev", "host", "full", "dev_edge", "host_edge")}
    cwd = os.getcwd()
    os.chdir(tmp)                                            # save_ply_visualization writes results/input_images.png relative to cwd
    try:
        info = save_point_cloud(pred, f["dev"], edge_rtol=None, verbose=False)
        host_ply(pred, f["host"])
        save_ply_visualization(pred, f["full"], verbose=False)
        info_edge = save_point_cloud(pred, f["dev_edge"], edge_rtol=0.03, verbose=False)
        host_ply(pred, f["host_edge"], edge_rtol=0.03)
        same = {k: open(f[a], "rb").read() == open(f[b], "rb").read() for k, (a, b) in
                dict(a_device_vs_host=("dev", "host"), a_device_vs_save_ply_visualization=("dev", "full"), b_device_vs_host=("dev_edge", "host_edge")).items()}
        if not all(same.values()):
            raise SystemExit(f"the two paths wrote different files: {same}")
        a = rounds({"device": lambda: save_point_cloud(pred, f["dev"], edge_rtol=None, verbose=False),
                    "host_ply_only": lambda: host_ply(pred, f["host"]),
                    "host_save_ply_visualization": lambda: save_ply_visualization(pred, f["full"], verbose=False)})
        b = rounds({"device": lambda: save_point_cloud(pred, f["dev_edge"], edge_rtol=0.03, verbose=False),
                    "host": lambda: host_ply(pred, f["host_edge"], edge_rtol=0.03)})
    finally:
        os.chdir(cwd)

    # (c) the kernels alone, buffers allocated once; bytes = what the algorithm has to move, from the shapes
    points, local, images = pred["points"][0].contiguous(), pred["local_points"][0].contiguous(), pred["images"][0].contiguous()
    mask = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    rec = torch.empty((pixels, 15), dtype=torch.uint8, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    K, used = torch.empty((n, 3, 3), device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    ws_c = torch.empty(hip.cloud_compact_workspace(n, H, W), dtype=torch.uint8, device=dev)
    ws_i = torch.empty(hip.intrinsics_lsq_workspace(n, H, W), dtype=torch.uint8, device=dev)
    L, p, st = hip.lib(), hip._p, hip._stream

    def k_mask():
        hip._ck(L.g2v_cloud_mask(p(points), p(local), None, n, H, W, hip.CLOUD_FINITE | hip.CLOUD_EDGE_RTOL, 0.0, 0.0, 0.03, p(mask), st()), "mask")

    def k_compact():
        hip._ck(L.g2v_cloud_compact(p(points), p(images), p(mask), n, H, W, p(rec), pixels, p(counts), p(ws_c), ws_c.numel(), st()), "compact")

    def k_lsq():
        hip._ck(L.g2v_intrinsics_lsq(p(local), p(mask), n, H, W, p(K), p(used), p(ws_i), ws_i.numel(), st()), "lsq")

    kernels = {}
    k_mask()
    kept = int(mask.sum())
    for name, fn, nbytes in (("g2v_cloud_mask", k_mask, pixels * 25),
                             ("g2v_cloud_compact", k_compact, pixels * 2 + kept * (24 + 15)),      # mask read twice; kept points + colours in, records out
                             ("g2v_intrinsics_lsq", k_lsq, pixels * 1 + kept * 12)):
        ms = kernel_time(fn)
        kernels[name] = dict(ms=round(ms, 4), bytes=int(nbytes), GB_per_s=round(nbytes / ms / 1e6, 1))
    return dict(views=n, height=H, width=W, pixels=pixels, kept_filter_nan=info["num_points"], kept_edge_rtol_0p03=info_edge["num_points"],
                files_identical=same, a_filter_nan_only=a, b_edge_rtol_0p03=b, c_kernels=kernels,
                bytes_device_to_host=dict(device_path=info["num_points"] * 15, host_path=pixels * 24))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_export_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud_export.py measures on the GPU; there is none here")
    ram = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=ram) as tmp:
        sizes = []
        for n in args.views:
            sizes.append(bench_size(n, tmp))
            print(f"{n} views done: (a) {sizes[-1]['a_filter_nan_only']}", file=sys.stderr, flush=True)
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]
    res = dict(what="point-cloud export: device path vs host path, and the kernels of csrc/cloud.hip alone",
               measured_on="1x MI355X (gfx950)" if arch == "gfx950" else "1x " + torch.cuda.get_device_name(0),
               device_name=torch.cuda.get_device_name(0), arch=arch, ram_backed_dir=ram is not None,
               method=f"median of {ROUNDS} rounds after {WARMUP} warm-ups, variants alternated inside a round; call times: host clock around "
                      f"work ending in a device synchronise; kernel times: device events around {KERNEL_LAUNCHES} launches",
               sizes=sizes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
