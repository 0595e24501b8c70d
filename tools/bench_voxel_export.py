"""Time the voxel-downsampled export (g2vlm_utils.save_point_cloud(voxel_size=v): csrc/voxel.hip) against the unfiltered export
and against the same downsampling done on the host.  Needs the GPU; bench.py is a different measurement and is not touched.

    python tools/bench_voxel_export.py [--views 8 32] [--out profiles/voxel_export_bench.json]

The scenes, the RAM-backed directory, the alternation and the medians are tools/bench_cloud_export.py's: synthetic pred_dicts of N
views of 518 x 518, 3 warm-ups and then 10 timed rounds, a round running every variant once, in turn.  Per size two voxel sizes,
found by bisection on the device so that the file has roughly 10x and 100x fewer vertices than the unfiltered one.  Before
anything is timed the device file is compared byte for byte with the host restatement's.

  device_voxel   save_point_cloud(edge_rtol=None, voxel_size=v)
  device_full    save_point_cloud(edge_rtol=None): every finite point, what the export wrote before
  host_voxel     copy points and images to the host, tests/voxel_check.py's numpy restatement (np.unique on the keys), write
  kernels        device events around 20 launches of g2v_voxel_assign, and of g2v_voxel_reduce with and without the in-wave
                 summing of runs of equal ids (G2V_VOXEL_NO_RUNS)
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_cloud_export as base  # noqa: E402
import voxel_check  # noqa: E402
from g2vlm_amd import hip, host  # noqa: E402
from g2vlm_amd.g2vlm_utils import save_point_cloud, voxel_downsample  # noqa: E402

H, W = base.H, base.W


def host_voxel(pred, path, v):
    """the full copy, then the numpy restatement with the default origin, then the write"""
    pts = pred["points"][0].detach().float().cpu().numpy()
    col = pred["images"][0].detach().float().cpu().numpy()
    mask = np.isfinite(pts).all(-1)
    out = voxel_check.downsample(pts, col, mask, v, voxel_check.default_origin(pts, mask, v))
    host.write_ply_records(path, out["records"])


def voxel_size_for(pred, kept, ratio):
    """bisection on log v for len(voxel_downsample) ~ kept / ratio"""
    lo, hi = 1e-4, 10.0
    for _ in range(24):
        v = (lo * hi) ** 0.5
        m = len(voxel_downsample(pred, v)["counts"])
        lo, hi = (v, hi) if m * ratio > kept else (lo, v)
    return float(f"{(lo * hi) ** 0.5:.3g}")


def bench_voxel(pred, n, v, tmp, kept):
    dev = torch.device("cuda")
    f = {k: os.path.join(tmp, k + ".ply") for k in ("dev_voxel", "dev_full", "host_voxel")}
    info = save_point_cloud(pred, f["dev_voxel"], edge_rtol=None, verbose=False, voxel_size=v)
    host_voxel(pred, f["host_voxel"], v)
    if open(f["dev_voxel"], "rb").read() != open(f["host_voxel"], "rb").read():
        raise SystemExit(f"{n} views, voxel size {v}: the device and the host wrote different files")
    calls = base.rounds({"device_voxel": lambda: save_point_cloud(pred, f["dev_voxel"], edge_rtol=None, verbose=False, voxel_size=v),
                         "device_full": lambda: save_point_cloud(pred, f["dev_full"], edge_rtol=None, verbose=False),
                         "host_voxel": lambda: host_voxel(pred, f["host_voxel"], v)})

    points, images = pred["points"][0].contiguous(), pred["images"][0].contiguous()
    mask = hip.cloud_mask(points, finite=True)
    lo, _, _ = hip.voxel_bounds(points, mask)
    origin = [x - v * 0.5 for x in lo]
    voxel_of, stats = hip.voxel_assign(points, mask, v, origin)
    m = stats[0]
    ws_a = torch.empty(hip.voxel_assign_workspace(n, H, W) // 8 + 1, dtype=torch.int64, device=dev)
    ws_r = torch.empty(hip.voxel_reduce_workspace(m) // 8 + 1, dtype=torch.int64, device=dev)
    st_dev = torch.empty(4, dtype=torch.int32, device=dev)
    rec, cnt = torch.empty((m, 15), dtype=torch.uint8, device=dev), torch.empty(m, dtype=torch.int32, device=dev)
    L, p, st = hip.lib(), hip._p, hip._stream

    def k_assign():
        hip._ck(L.g2v_voxel_assign(p(points), p(mask), n, H, W, v, *origin, p(voxel_of), p(st_dev), p(ws_a), ws_a.numel() * 8, st()), "assign")

    def k_reduce(flags):
        hip._ck(L.g2v_voxel_reduce(p(points), p(images), p(voxel_of), n, H, W, v, *origin, m, p(rec), p(cnt), None, None, p(ws_r),
                                   ws_r.numel() * 8, flags, st()), "reduce")

    kernels = {name: round(base.kernel_time(fn), 4) for name, fn in (("g2v_voxel_assign_ms", k_assign),
                                                                     ("g2v_voxel_reduce_ms", lambda: k_reduce(0)),
                                                                     ("g2v_voxel_reduce_no_runs_ms", lambda: k_reduce(hip.VOXEL_NO_RUNS)))}
    return dict(voxel_size=v, voxels=info["num_points"], input_points=info["num_input_points"], fewer_vertices=round(kept / max(info["num_points"], 1), 1),
                files_identical=True, calls=calls, kernels=kernels, table_bytes=hip.voxel_assign_workspace(n, H, W),
                bytes_device_to_host=dict(device_voxel=info["num_points"] * 15 + 16 + 28 + 4 * n, device_full=kept * 15 + 4 * n,
                                          host_voxel=n * H * W * 24))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--ratios", type=float, nargs="+", default=[10.0, 100.0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_export_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_voxel_export.py measures on the GPU; there is none here")
    ram = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    sizes = []
    with tempfile.TemporaryDirectory(dir=ram) as tmp:
        for n in args.views:
            pred = base.synthetic_pred(n, torch.device("cuda"))
            kept = save_point_cloud(pred, os.path.join(tmp, "full.ply"), edge_rtol=None, verbose=False)["num_points"]
            runs = []
            for ratio in args.ratios:
                runs.append(bench_voxel(pred, n, voxel_size_for(pred, kept, ratio), tmp, kept))
                print(f"{n} views, 1/{ratio:g}: {runs[-1]}", file=sys.stderr, flush=True)
            sizes.append(dict(views=n, height=H, width=W, pixels=n * H * W, kept_filter_nan=kept, voxel_sizes=runs))
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]
    res = dict(what="voxel-downsampled export: save_point_cloud(voxel_size=v) vs the unfiltered export vs the same downsampling on the host",
               measured_on="1x MI355X (gfx950)" if arch == "gfx950" else "1x " + torch.cuda.get_device_name(0),
               device_name=torch.cuda.get_device_name(0), arch=arch, ram_backed_dir=ram is not None,
               method=f"median of {base.ROUNDS} rounds after {base.WARMUP} warm-ups, variants alternated inside a round; call times: host clock "
                      f"around work ending in a device synchronise; kernel times: device events around {base.KERNEL_LAUNCHES} launches",
               sizes=sizes)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
