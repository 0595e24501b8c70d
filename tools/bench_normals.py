"""Time the surface normals (g2v_cloud_normals, g2v_cloud_compact_normals: csrc/normals.hip) on the synthetic floor-and-sphere scene of
tests/consistency_check.py: N views of 518 x 518 under edge_rtol = 0.03.  Needs the GPU; bench.py is a different measurement and is
not touched.

    python tools/bench_normals.py [--views 8 32] [--out profiles/normals_bench.json]

  kernel         device events around single calls of g2v_cloud_normals into preallocated outputs, warmed up: median, p10 and p90 of
                 30 calls, at steps 1 and 4, with all four outputs and with `normals` alone; achieved bytes/s over the bytes the
                 algorithm has to move (13 B read and 29 B - or 12 B - written per pixel), beside the 6.3 TB/s that a streaming copy
                 reaches on this part
  forms          the plain-load form against the LDS-halo form at step 1, alternated call by call under the same events
  torch          the same rule written in torch on the same device - elementwise kernels, nothing fuses - under the same events; it is
                 compared with the kernel before anything is timed (valid must be equal; whether the floats are bit-equal is reported)
  save           save_point_cloud_normals into a RAM-backed directory against the host path - copy points, images and depth to the
                 host, the mask with torch's CPU max_pool2d, tests/normals_check.py's rule in numpy, host.write_ply_normal_records -,
                 the two files compared first; host clock around work ending in a synchronise, the variants alternated inside a round
                 (the host shares its CPUs with other work: the spread is reported, and only the ratio's order of magnitude means much)"""
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
import normals_check as nc  # noqa: E402
from bench_mesh_export import event_times, percentiles, save_rounds  # noqa: E402
from g2vlm_amd import hip, host  # noqa: E402
from g2vlm_amd.g2vlm_utils import save_point_cloud_normals  # noqa: E402

H, W, LAUNCHES, WARM = base.H, base.W, 30, 5
READ_BYTES, WRITE_ALL, WRITE_NORMALS = 13, 29, 12
HBM_ACHIEVABLE_TB_S = 6.3                                    # a float4 streaming copy on an MI355X (8.0 TB/s on the data sheet)


def shifted(a, dy, dx):
    """out[:, y, x] = a[:, y + dy, x + dx] inside the view, 0 / False elsewhere"""
    out = torch.zeros_like(a)
    Hh, Ww = a.shape[1:3]
    y0, y1, x0, x1 = max(0, -dy), min(Hh, Hh - dy), max(0, -dx), min(Ww, Ww - dx)
    if y1 > y0 and x1 > x0:
        out[:, y0:y1, x0:x1] = a[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def torch_rule(points, mask, poses, step):
    """the rule in torch: separate elementwise kernels; -> (normals, valid uint8, cos_view, colors [N,3,H,W])"""
    part = (mask != 0) & torch.isfinite(points).all(-1)
    e, av = [], []
    for dy, dx in nc.NEIGHBOURS:
        e.append(shifted(points, dy * step, dx * step) - points)
        av.append(shifted(part, dy * step, dx * step))
    m = torch.zeros_like(points)
    have = torch.zeros_like(part)
    for a, b in nc.PAIRS:
        present = av[a] & av[b] & part
        x, y = e[a], e[b]
        c = torch.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                         x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], -1)
        m = torch.where((present & have)[..., None], m + c, torch.where(present[..., None], c, m))
        have = have | present
    s2 = (m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]
    valid = part & have & torch.isfinite(s2) & (s2 > 0)
    n = m / torch.sqrt(s2)[..., None]
    d = points - poses[:, None, None, :3, 3]
    t = (n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]
    n = torch.where((t > 0)[..., None], -n, n)
    q = t.abs() / torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    q = torch.where(torch.isnan(q), torch.zeros_like(q), q)
    zero = torch.zeros((), dtype=points.dtype, device=points.device)
    cos_view = torch.where(valid, torch.clamp(q, max=1.0), zero)
    colors = torch.where(valid[..., None], n * 0.5 + 0.5, zero).permute(0, 3, 1, 2).contiguous()
    return torch.where(valid[..., None], n, zero), valid.to(torch.uint8), cos_view, colors


def host_normals_ply(pred, path, edge_rtol):
    """the export on the host: copy points, images, poses (and the depth) over, the mask as tools/bench_cloud_export.py's host_ply has
    it, the rule and the records in numpy, one write"""
    images = pred["images"][0].detach().float().cpu().numpy()
    pts = pred["points"][0].detach().float().cpu().numpy()
    poses = pred["camera_poses"][0].detach().float().cpu().numpy()
    ok = np.isfinite(pts).all(-1)
    d = pred["local_points"][0, ..., 2].detach().float().cpu().unsqueeze(1)
    mp = torch.nn.functional.max_pool2d
    diff = mp(d, 3, stride=1, padding=1) + mp(-d, 3, stride=1, padding=1)
    ok &= ~((diff / d).nan_to_num_() > edge_rtol).numpy()[:, 0]
    r = nc.rule(pts, ok, poses)
    host.write_ply_normal_records(path, nc.records(pts, r["normals"], images, ok))


def alternated(fns):
    """{name: fn} -> {name: percentiles}: every round times every form once, in turn, under device events"""
    times = {k: [] for k in fns}
    for r in range(WARM + LAUNCHES):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= WARM:
                times[k].append(a.elapsed_time(b))
    return {k: percentiles(v) for k, v in times.items()}


def with_rate(t, nbytes):
    t = dict(t, algorithm_bytes=nbytes)
    t["GB_per_s"] = round(nbytes / t["median_ms"] / 1e6, 1)
    t["share_of_achievable_hbm"] = round(t["GB_per_s"] / (HBM_ACHIEVABLE_TB_S * 1e3), 3)
    return t


def bench_views(n, tmp):
    s = nc.scene(n, H, W)
    points, local, poses = torch.from_numpy(s["points"]).cuda(), torch.from_numpy(s["local"]).cuda(), torch.from_numpy(s["poses"]).cuda()
    colors = torch.from_numpy(nc.scene_colors(n, H, W)).cuda()
    pred = dict(points=points[None], local_points=local[None], camera_poses=poses[None], images=colors[None], conf=None)
    del s
    edge_rtol = 0.03
    mask = hip.cloud_mask(points, local, edge_rtol=edge_rtol, finite=True)
    pixels = n * H * W
    out = dict(normals=torch.empty((n, H, W, 3), device="cuda"), valid=torch.empty((n, H, W), dtype=torch.uint8, device="cuda"),
               cos_view=torch.empty((n, H, W), device="cuda"), colors=torch.empty((n, 3, H, W), device="cuda"))
    res = dict(config=f"{n}v_edge_rtol_0p03", views=n, height=H, width=W, edge_rtol=edge_rtol, pixels=pixels, kept=int(mask.sum()))

    # the kernel (both forms) against the torch form, before anything is timed
    want = torch_rule(points, mask, poses, 1)
    for flags in (hip.NORMALS_PLAIN, hip.NORMALS_HALO):
        hip.cloud_normals_raw(points, mask, poses, 1, None, flags=flags, **out)
        torch.cuda.synchronize()
        if not torch.equal(out["valid"], want[1]) or float((out["normals"] - want[0]).abs().max()) > 1e-5:
            raise SystemExit(f"{res['config']}: the kernel (flags {flags}) and the torch form differ")
    res.update(valid=int(want[1].sum()), kernel_valid_equals_torch_form=True,
               kernel_bits_equal_torch_form=bool(torch.equal(out["normals"].view(torch.int32), want[0].view(torch.int32)) and
                                                 torch.equal(out["cos_view"].view(torch.int32), want[2].view(torch.int32)) and
                                                 torch.equal(out["colors"].view(torch.int32), want[3].view(torch.int32))))
    del want

    res["kernel"] = {}
    for step in (1, 4):
        res["kernel"][f"step{step}_all_outputs"] = with_rate(event_times(lambda: hip.cloud_normals_raw(points, mask, poses, step, None, **out)),
                                                             pixels * (READ_BYTES + WRITE_ALL))
        res["kernel"][f"step{step}_normals_only"] = with_rate(
            event_times(lambda: hip.cloud_normals_raw(points, mask, poses, step, None, normals=out["normals"])), pixels * (READ_BYTES + WRITE_NORMALS))
        res["kernel"][f"step{step}_torch_form"] = event_times(lambda: torch_rule(points, mask, poses, step))
        res["kernel"][f"step{step}_torch_over_kernel"] = round(res["kernel"][f"step{step}_torch_form"]["median_ms"] /
                                                               res["kernel"][f"step{step}_all_outputs"]["median_ms"], 1)
    forms = alternated({"plain_all_outputs": lambda: hip.cloud_normals_raw(points, mask, poses, 1, None, flags=hip.NORMALS_PLAIN, **out),
                        "halo_all_outputs": lambda: hip.cloud_normals_raw(points, mask, poses, 1, None, flags=hip.NORMALS_HALO, **out),
                        "plain_normals_only": lambda: hip.cloud_normals_raw(points, mask, poses, 1, None, flags=hip.NORMALS_PLAIN, normals=out["normals"]),
                        "halo_normals_only": lambda: hip.cloud_normals_raw(points, mask, poses, 1, None, flags=hip.NORMALS_HALO, normals=out["normals"])})
    res["forms_step1"] = dict(forms, halo_over_plain_all_outputs=round(forms["halo_all_outputs"]["median_ms"] / forms["plain_all_outputs"]["median_ms"], 3),
                              halo_over_plain_normals_only=round(forms["halo_normals_only"]["median_ms"] / forms["plain_normals_only"]["median_ms"], 3))
    res["compact_normals_wrapper"] = event_times(lambda: hip.cloud_compact_normals(points, out["normals"], colors, mask))

    f_dev, f_host = os.path.join(tmp, "dev.ply"), os.path.join(tmp, "host.ply")
    info = save_point_cloud_normals(pred, f_dev, edge_rtol=edge_rtol, verbose=False)
    host_normals_ply(pred, f_host, edge_rtol)
    if open(f_dev, "rb").read() != open(f_host, "rb").read():
        raise SystemExit(f"{res['config']}: save_point_cloud_normals and the host path wrote different files")
    res["save"] = save_rounds({"device": lambda: save_point_cloud_normals(pred, f_dev, edge_rtol=edge_rtol, verbose=False),
                               "host": lambda: host_normals_ply(pred, f_host, edge_rtol)})
    res["save"].update(files_identical=True, file_bytes=os.path.getsize(f_dev),
                       bytes_device_to_host=dict(device_path=info["num_points"] * 27, host_path=pixels * 28 + n * 64),
                       host_over_device=round(res["save"]["host"]["median_ms"] / res["save"]["device"]["median_ms"], 1))
    print(res, file=sys.stderr, flush=True)
    return [res]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_normals.py measures on the GPU; there is none here")
    ram = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    configs = []
    with tempfile.TemporaryDirectory(dir=ram) as tmp:
        for n in a.views:
            configs += bench_views(n, tmp)
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]
    res = dict(what="surface normals: g2v_cloud_normals (plain-load and LDS-halo forms) vs the same rule in torch, save_point_cloud_normals vs the "
                    "host path",
               measured_on="1x MI355X (gfx950)" if arch == "gfx950" else "1x " + torch.cuda.get_device_name(0), arch=arch,
               library=os.path.basename(hip.LIB_PATH), ram_backed_dir=ram is not None, hbm_achievable_TB_per_s=HBM_ACHIEVABLE_TB_S,
               method=f"kernel / torch / forms: device events around one call, {LAUNCHES} calls after {WARM} warm-ups (forms: alternated call by "
                      "call); save: median of 5 rounds after 1 warm-up, variants alternated inside a round, host clock around work ending in a "
                      "device synchronise; GB_per_s = algorithm_bytes (13 B read + 29 B or 12 B written per pixel) over the median", configs=configs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
