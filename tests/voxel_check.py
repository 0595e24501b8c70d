"""Helper (no tests): the voxel-downsampling rule of DESIGN.md 6j restated in numpy, written from the rule and not from the kernels
(csrc/voxel.hip follows this file, not the other way round).

  participating  which pixels take part: mask != 0 and three finite coordinates
  cells          per participating point the cell g (fp64 floor), the 24-bit fraction q and the packed 63-bit key
  downsample     the whole rule: records uint8 [M,15], counts, labels voxel_of, stats - integer sums, first-appearance order
  brute_means    an independent check: per cell the fp64 mean of the member points and of their colour bytes, found by a
                 dictionary over the cells and not through the keys, the fractions or np.unique
  default_origin Open3D's convention: the minimum of the participating points minus voxel_size / 2, in fp64
"""
import numpy as np

Q = 16777216.0                                               # 2^24 fraction steps per cell
G = 1048576.0                                                # cells [-2^20, 2^20) per axis


def participating(points, mask):
    points = np.asarray(points, dtype=np.float32)
    return (np.asarray(mask).reshape(points.shape[:-1]) != 0) & np.isfinite(points).all(-1)


def default_origin(points, mask, voxel_size):
    part = participating(points, mask)
    if not part.any():
        return np.zeros(3)
    return np.asarray(points, dtype=np.float32)[part].astype(np.float64).min(0) - np.float64(voxel_size) * 0.5


def cells(p, voxel_size, origin):
    """p fp32 [K,3], finite -> (g fp64 [K,3], q int64 [K,3], key uint64 [K], in_range bool [K]); q and key are 0 out of range"""
    v, o = np.float64(voxel_size), np.asarray(origin, dtype=np.float64)
    with np.errstate(over="ignore"):
        t = (p.astype(np.float64) - o) / v
    g = np.floor(t)
    ok = ((g >= -G) & (g < G)).all(1)
    g_ok = np.where(ok[:, None], g, 0.0)
    f = np.where(ok[:, None], t, 0.0) - g_ok
    q = np.floor(f * Q + 0.5).astype(np.int64)
    cell = (g_ok.astype(np.int64) + (1 << 20)).astype(np.uint64)
    key = cell[:, 0] | (cell[:, 1] << np.uint64(21)) | (cell[:, 2] << np.uint64(42))
    q[~ok] = 0
    key[~ok] = 0
    return g, q, key, ok


def colour_bytes(colors):
    """host.write_ply_binary's byte of colours fp32 [..., 3]"""
    return (np.clip(np.asarray(colors, dtype=np.float32).astype(np.float64), 0, 1) * 255).astype(np.uint8)


def downsample(points, colors, mask, voxel_size, origin, min_points=1):
    """points fp32 [N,H,W,3], colors fp32 [N,3,H,W], mask [N,H,W] -> dict(records uint8 [M,15], points fp32 [M,3], colors uint8
    [M,3], counts int32 [M], voxel_of int32 [N,H,W] (ids BEFORE min_points drops cells; -1: dropped pixel), stats = [cells before
    min_points, participating pixels, out-of-range pixels, 0], kept bool [cells] = n >= min_points)."""
    points = np.ascontiguousarray(points, dtype=np.float32)
    colors = np.asarray(colors, dtype=np.float32)
    n_views, h, w, _ = points.shape
    v, o = np.float64(voxel_size), np.asarray(origin, dtype=np.float64)
    part = participating(points, mask).reshape(-1)
    flat = np.flatnonzero(part)                              # flat pixel index: view-major, row-major
    p = points.reshape(-1, 3)[flat]
    _, q, key, ok = cells(p, v, o)
    n_out = int((~ok).sum())
    flat, p, q, key = flat[ok], p[ok], q[ok], key[ok]
    byte = colour_bytes(colors.transpose(0, 2, 3, 1).reshape(-1, 3)[flat]).astype(np.int64)

    uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                 # cells by first appearance (first holds positions in pixel order)
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    label = rank[inv.reshape(-1)]
    m = len(uniq)
    n = np.bincount(label, minlength=m).astype(np.int64)
    S = np.zeros((m, 3), dtype=np.int64)
    C = np.zeros((m, 3), dtype=np.int64)
    if m:                                                    # int64 sums over the members of every cell (each cell has one at least)
        by_cell = np.argsort(label, kind="stable")
        starts = np.searchsorted(label[by_cell], np.arange(m))
        S = np.add.reduceat(q[by_cell], starts, axis=0)
        C = np.add.reduceat(byte[by_cell], starts, axis=0)
    k = uniq[order]
    g = np.stack([((k >> np.uint64(21 * a)) & np.uint64(0x1fffff)).astype(np.int64) - (1 << 20) for a in range(3)], 1)
    mean = S.astype(np.float64) / (n.astype(np.float64)[:, None] * Q)
    xyz = (o + (g.astype(np.float64) + mean) * v).astype(np.float32)
    rgb = ((2 * C + n[:, None]) // (2 * n[:, None])).astype(np.uint8)

    voxel_of = np.full(n_views * h * w, -1, dtype=np.int32)
    voxel_of[flat] = label
    kept = n >= min_points
    xyz_k, rgb_k = xyz[kept], rgb[kept]
    rec = np.zeros((int(kept.sum()), 15), dtype=np.uint8)
    rec[:, :12] = np.ascontiguousarray(xyz_k, dtype="<f4").view(np.uint8).reshape(-1, 12)
    rec[:, 12:] = rgb_k
    return dict(records=rec, points=xyz_k, colors=rgb_k, counts=n[kept].astype(np.int32), voxel_of=voxel_of.reshape(n_views, h, w),
                stats=[m, int(len(flat)), n_out, 0], kept=kept)


def brute_means(points, colors, mask, voxel_size, origin):
    """{(gx, gy, gz): (mean fp64 [3] of the member points, mean fp64 [3] of their colour bytes, n)} in first-appearance order
    (dicts keep insertion order).  A python loop: small inputs only."""
    points = np.asarray(points, dtype=np.float32)
    colors = np.asarray(colors, dtype=np.float32)
    v, o = float(voxel_size), [float(x) for x in origin]
    part = participating(points, mask).reshape(-1)
    pts = points.reshape(-1, 3)
    cols = colour_bytes(colors.transpose(0, 2, 3, 1).reshape(-1, 3))
    members = {}
    for i in np.flatnonzero(part):
        cell = [np.floor((float(pts[i, a]) - o[a]) / v) for a in range(3)]
        if all(-G <= c < G for c in cell):
            members.setdefault(tuple(int(c) for c in cell), []).append(i)
    return {cell: (pts[idx].astype(np.float64).mean(0), cols[idx].astype(np.float64).mean(0), len(idx)) for cell, idx in members.items()}
