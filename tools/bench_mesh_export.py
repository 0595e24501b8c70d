"""Time the triangle-mesh export (g2v_cloud_mesh: csrc/mesh.hip) on the synthetic floor-and-sphere scene of
tests/consistency_check.py: N views of 518 x 518, under the finite test alone and with edge_rtol = 0.03 on top.  Needs the GPU;
bench.py is a different measurement and is not touched.

    python tools/bench_mesh_export.py [--views 8 32] [--out profiles/mesh_export_bench.json]

  kernel         device events around single calls of the entry point g2v_cloud_mesh (classify, count, scan, vertex ids, faces;
                 every output on, outputs for the worst case and workspace allocated once), warmed up: median, p10 and p90 of 30 calls
  count_only     the same around the call that hip.cloud_mesh makes first: no face output, no vertex ids (classify, count, scan)
  wrapper        the same around hip.cloud_mesh as reconstruct_mesh / save_mesh call it: count, read the counts back, allocate at
                 the exact size, fill, g2v_cloud_compact of the used pixels
  torch          the same rule written in torch on the same device - elementwise edge lengths, boolean indexing, a cumulative sum -
                 under the same events and number of calls; it is compared with the kernel before anything is timed and the tool
                 stops if they differ
  save           save_mesh into a RAM-backed directory against the host path - copy points, images and depth to the host, the mask
                 with torch's CPU max_pool2d, tests/mesh_check.py's rule in numpy, host.write_ply_mesh -, the two files compared
                 first; host clock around work ending in a synchronise, the variants alternated inside a round"""
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
import mesh_check as mc  # noqa: E402
from g2vlm_amd import hip, host  # noqa: E402
from g2vlm_amd.g2vlm_utils import save_mesh  # noqa: E402

H, W, LAUNCHES, WARM = base.H, base.W, 30, 5
SAVE_WARM, SAVE_ROUNDS = 1, 5


def torch_rule(points, mask, max_edge=None):
    """the rule in torch: separate elementwise kernels, so nothing fuses; -> (used uint8, vertex_of int32, faces int32, counts int32)"""
    N, Hh, Ww = points.shape[:3]
    dev = points.device
    keep = mask != 0
    p00, p01, p10, p11 = points[:, :-1, :-1], points[:, :-1, 1:], points[:, 1:, :-1], points[:, 1:, 1:]
    k00, k01, k10, k11 = keep[:, :-1, :-1], keep[:, :-1, 1:], keep[:, 1:, :-1], keep[:, 1:, 1:]

    def e2(a, b):
        d = a - b
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]

    n = k00.int() + k01.int() + k10.int() + k11.int()
    ea, em = e2(p01, p10), e2(p00, p11)
    anti = ea < em
    four, three = n == 4, n == 3
    t = [(four & anti) | (three & ~k11), (four & anti) | (three & ~k00), (four & ~anti) | (three & ~k01), (four & ~anti) | (three & ~k10)]
    if max_edge is not None:
        lim = torch.tensor(max_edge, dtype=torch.float32, device=dev)
        lim = lim * lim
        top, left, right, bottom, da, dm = e2(p00, p01) <= lim, e2(p00, p10) <= lim, e2(p01, p11) <= lim, e2(p10, p11) <= lim, ea <= lim, em <= lim
        t = [t[0] & left & da & top, t[1] & da & bottom & right, t[2] & left & bottom & dm, t[3] & dm & right & top]
    bits = torch.stack(t, -1)                                                                       # [N,H-1,W-1,4]
    pix = torch.arange(N * Hh * Ww, device=dev, dtype=torch.int64).view(N, Hh, Ww)[:, :-1, :-1]
    off = torch.tensor([[dy * Ww + dx for dy, dx in tri] for tri in mc.TRIANGLES], device=dev, dtype=torch.int64)
    face_pixels = (pix[..., None, None] + off)[bits]                                                # C order: view, row, column, triangle
    used = torch.zeros(N * Hh * Ww, dtype=torch.uint8, device=dev)
    used[face_pixels.reshape(-1)] = 1
    rank = torch.cumsum(used, 0, dtype=torch.int64) - 1
    vertex_of = torch.where(used != 0, rank, torch.full_like(rank, -1)).int()
    faces = vertex_of[face_pixels]
    counts = torch.stack([used.view(N, -1).sum(1, dtype=torch.int64), bits.reshape(N, -1).sum(1, dtype=torch.int64)], 1).int()
    return used.view(N, Hh, Ww), vertex_of.view(N, Hh, Ww), faces, counts


def host_mesh(pred, path, edge_rtol=None):
    """the export on the host: copy points, images (and the depth) over, mask as tools/bench_cloud_export.py's host_ply has it, the
    rule and the records in numpy, one write"""
    images = pred["images"][0].detach().float().cpu().numpy()
    pts = pred["points"][0].detach().float().cpu().numpy()
    ok = np.isfinite(pts).all(-1)
    if edge_rtol is not None:
        d = pred["local_points"][0, ..., 2].detach().float().cpu().unsqueeze(1)
        mp = torch.nn.functional.max_pool2d
        diff = mp(d, 3, stride=1, padding=1) + mp(-d, 3, stride=1, padding=1)
        ok &= ~((diff / d).nan_to_num_() > edge_rtol).numpy()[:, 0]
    r = mc.rule(pts, ok)
    host.write_ply_mesh(path, mc.vertex_records(pts, images, r["used"]), r["face_records"])


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


def save_rounds(variants):
    """{name: fn} -> {name: {median_ms, min_ms, max_ms}}; every round runs every variant once, in turn"""
    times = {k: [] for k in variants}
    for r in range(SAVE_WARM + SAVE_ROUNDS):
        for k, fn in variants.items():
            t = base.timed(fn)
            if r >= SAVE_WARM:
                times[k].append(t)
    return {k: dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3)) for k, v in times.items()}


def bench_views(n, tmp):
    s = mc.scene(n, H, W)
    points, local = torch.from_numpy(s["points"]).cuda(), torch.from_numpy(s["local"]).cuda()
    colors = torch.from_numpy(mc.scene_colors(n, H, W)).cuda()
    pred = dict(points=points[None], local_points=local[None], camera_poses=torch.from_numpy(s["poses"]).cuda()[None], images=colors[None], conf=None)
    del s
    cap = 2 * n * (H - 1) * (W - 1)
    used, vertex_of = torch.empty((n, H, W), dtype=torch.uint8, device="cuda"), torch.empty((n, H, W), dtype=torch.int32, device="cuda")
    faces, records = torch.empty((cap, 3), dtype=torch.int32, device="cuda"), torch.empty((cap, 13), dtype=torch.uint8, device="cuda")
    counts = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    ws = torch.empty((hip.cloud_mesh_workspace(n, H, W) + 7) // 8, dtype=torch.int64, device="cuda")
    out = []
    for edge_rtol in (None, 0.03):
        mask = hip.cloud_mask(points, local, edge_rtol=edge_rtol, finite=True)
        res = dict(config=f"{n}v_" + ("finite" if edge_rtol is None else "edge_rtol_0p03"), views=n, height=H, width=W, edge_rtol=edge_rtol,
                   pixels=n * H * W, kept=int(mask.sum()), candidates_at_most=cap)

        def full():
            hip.cloud_mesh_raw(points, mask, None, counts, used, vertex_of, faces, records, workspace=ws)

        def count_only():
            hip.cloud_mesh_raw(points, mask, None, counts, workspace=ws)

        want = torch_rule(points, mask)
        full()
        torch.cuda.synchronize()
        F = int(counts[:, 1].sum())
        same = torch.equal(used, want[0]) and torch.equal(vertex_of, want[1]) and torch.equal(faces[:F], want[2]) and torch.equal(counts, want[3]) \
            and F == want[2].shape[0]
        if not same:
            raise SystemExit(f"{res['config']}: the kernel and the torch form differ")
        res.update(kernel_equals_torch_form=True, vertices=int(counts[:, 0].sum()), faces=F)
        del want
        # bytes the algorithm has to move, from the shapes: points and mask in; used, vertex ids, faces and records out
        nbytes = n * H * W * (12 + 1 + 1 + 4) + F * (12 + 13)
        res["kernel"] = event_times(full)
        res["kernel"]["algorithm_bytes"] = nbytes
        res["kernel"]["GB_per_s"] = round(nbytes / res["kernel"]["median_ms"] / 1e6, 1)
        res["count_only"] = event_times(count_only)
        res["wrapper"] = event_times(lambda: hip.cloud_mesh(points, colors, mask))
        res["torch_form"] = event_times(lambda: torch_rule(points, mask))
        res["torch_over_kernel"] = round(res["torch_form"]["median_ms"] / res["kernel"]["median_ms"], 1)
        f_dev, f_host = os.path.join(tmp, "dev.ply"), os.path.join(tmp, "host.ply")
        info = save_mesh(pred, f_dev, edge_rtol=edge_rtol, verbose=False)
        host_mesh(pred, f_host, edge_rtol)
        if open(f_dev, "rb").read() != open(f_host, "rb").read():
            raise SystemExit(f"{res['config']}: save_mesh and the host path wrote different files")
        res["save"] = save_rounds({"device": lambda: save_mesh(pred, f_dev, edge_rtol=edge_rtol, verbose=False),
                                   "host": lambda: host_mesh(pred, f_host, edge_rtol)})
        res["save"].update(files_identical=True, file_bytes=os.path.getsize(f_dev),
                           bytes_device_to_host=dict(device_path=info["num_vertices"] * 15 + info["num_faces"] * 13, host_path=n * H * W * 28),
                           host_over_device=round(res["save"]["host"]["median_ms"] / res["save"]["device"]["median_ms"], 1))
        out.append(res)
        print(res, file=sys.stderr, flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_export_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_export.py measures on the GPU; there is none here")
    ram = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    configs = []
    with tempfile.TemporaryDirectory(dir=ram) as tmp:
        for n in a.views:
            configs += bench_views(n, tmp)
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]
    res = dict(what="triangle-mesh export: g2v_cloud_mesh vs the same rule in torch, save_mesh vs the host path",
               measured_on="1x MI355X (gfx950)" if arch == "gfx950" else "1x " + torch.cuda.get_device_name(0), arch=arch,
               library=os.path.basename(hip.LIB_PATH), ram_backed_dir=ram is not None,
               method=f"kernel / count_only / wrapper / torch: device events around one call, {LAUNCHES} calls after {WARM} warm-ups; save: median "
                      f"of {SAVE_ROUNDS} rounds after {SAVE_WARM} warm-up, variants alternated inside a round, host clock around work ending in a "
                      "device synchronise", configs=configs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
