"""The z-buffer rendering rule that csrc/render.hip is held to (include/g2vlm_hip.h states it), restated in numpy.  Checker side
only: nothing here is imported by the product.  The scene, the poses and the masks are those of tests/consistency_check.py.

rule(...) evaluates the rule in the dtype it is given.  In float32 every ufunc call is one fp32 operation rounded once - separate
calls cannot fuse - which is what the kernel does with contraction switched off, so the two agree byte for byte.  In float64 the
same code is the yardstick for how much of the answer hangs on rounding: `near` marks the target pixels where a decision that
contributes to them sits within 1e-4 of a threshold, and outside that set both dtypes must pick the same source pixel."""
import numpy as np

from consistency_check import look_at_origin, random_mask, rotate, scene  # noqa: F401  (re-exported for the tests)


def colour_bytes(c):
    """cc_colour: the byte the PLY export writes for a colour channel"""
    return (np.clip(np.asarray(c, np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)


def _footprint(x0, y0, sel, r, OH, OW):
    """for the points `sel` (indices into x0 / y0) every covered target pixel: (point, flat target pixel), clipped to the image"""
    pts, tgt = [], []
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            tx, ty = x0[sel] + dx, y0[sel] + dy
            ok = (tx >= 0) & (tx < OW) & (ty >= 0) & (ty < OH)
            pts.append(sel[ok])
            tgt.append(ty[ok] * OW + tx[ok])
    return np.concatenate(pts), np.concatenate(tgt)


def rule(points, colors, mask, poses, K, skip, OH, OW, radius, background, dtype=np.float32, fused_uv=False, fused_q=None):
    """points fp32 [N,H,W,3], colors fp32 [N,3,H,W] or None, mask bool / uint8 [N,H,W] or None, poses fp32 [M,4,4] camera-to-world
    and K fp32 [M,3,3] of the targets, skip M ints or None, background 0xRRGGBB.
    Returns dict(color uint8 [M,OH,OW,3] (None without colors), depth `dtype` [M,OH,OW], index int32 [M,OH,OW], near bool
    [M,OH,OW], landed int [M] = the points that land per target).
    fused_uv: u and v as a fused multiply-add would give them - NOT the rule; the GPU test uses it to show that its scene tells
    the two apart.  fused_q (one of consistency_check.FUSED_Q, fp32 only): the same for the sums of R^T d."""
    f = dtype
    assert fused_q is None or f is np.float32
    N, H, W = points.shape[:3]
    M = poses.shape[0]
    P = points.reshape(-1, 3).astype(f)
    R, t = poses[:, :3, :3].astype(f), poses[:, :3, 3].astype(f)
    Kf = K.astype(f)
    keep = np.ones(N * H * W, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    finite = keep & np.isfinite(points.reshape(-1, 3)).all(-1)
    view = np.arange(N * H * W) // (H * W)
    depth = np.zeros((M, OH * OW), f)
    index = np.full((M, OH * OW), -1, np.int64)
    near = np.zeros((M, OH * OW), bool)
    landed = np.zeros(M, np.int64)
    with np.errstate(all="ignore"):
        for m in range(M):
            eligible = finite if skip is None else finite & (view != int(skip[m]))
            d0, d1, d2 = P[:, 0] - t[m, 0], P[:, 1] - t[m, 1], P[:, 2] - t[m, 2]
            q = [rotate(R[m], d0, d1, d2, k, fused_q) for k in range(3)]
            r0, r1 = q[0] / q[2], q[1] / q[2]
            if fused_uv:
                u = (Kf[m, 0, 0].astype(np.float64) * r0.astype(np.float64) + Kf[m, 0, 2].astype(np.float64)).astype(f)
                v = (Kf[m, 1, 1].astype(np.float64) * r1.astype(np.float64) + Kf[m, 1, 2].astype(np.float64)).astype(f)
            else:
                u = Kf[m, 0, 0] * r0 + Kf[m, 0, 2]
                v = Kf[m, 1, 1] * r1 + Kf[m, 1, 2]
            lands = eligible & (q[2] > 0) & np.isfinite(q[2]) & (u >= 0) & (u < f(OW)) & (v >= 0) & (v < f(OH))
            x0 = np.where(lands, u, 0).astype(np.int64)       # converted only where the point lands; truncation = floor there
            y0 = np.where(lands, v, 0).astype(np.int64)
            sel = np.flatnonzero(lands)
            landed[m] = sel.size
            pts, tgt = _footprint(x0, y0, sel, radius, OH, OW)
            if f is np.float32:
                # the rule as written: the minimum of the 64-bit keys, bits of q2 above the source index
                key = (q[2][pts].view(np.uint32).astype(np.uint64) << np.uint64(32)) | pts.astype(np.uint64)
                best = np.full(OH * OW, np.iinfo(np.uint64).max, np.uint64)
                np.minimum.at(best, tgt, key)
                hit = best != np.iinfo(np.uint64).max
                depth[m][hit] = (best[hit] >> np.uint64(32)).astype(np.uint32).view(np.float32)
                index[m][hit] = (best[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
            else:
                # the same order without the bit trick: the smallest depth, then the smallest index among the points that have it
                dmin = np.full(OH * OW, np.inf, f)
                np.minimum.at(dmin, tgt, q[2][pts])
                first = q[2][pts] == dmin[tgt]
                imin = np.full(OH * OW, N * H * W, np.int64)
                np.minimum.at(imin, tgt[first], pts[first])
                hit = imin < N * H * W
                depth[m][hit], index[m][hit] = dmin[hit], imin[hit]
            # near: the runner-up of a pixel within 1e-4 (relative) of its winner ...
            other = pts != index[m][tgt]
            second = np.full(OH * OW, np.inf, np.float64)
            np.minimum.at(second, tgt[other], q[2][pts[other]].astype(np.float64))
            near[m] |= hit & (second - depth[m] <= 1e-4 * depth[m])
            # ... and every pixel that a point with u or v within 1e-4 of an integer, or |q2| <= 1e-4, covers or could cover
            close = eligible & ((np.abs(u - np.rint(u)) <= 1e-4) | (np.abs(v - np.rint(v)) <= 1e-4) | (np.abs(q[2]) <= 1e-4)) & \
                (u >= -2) & (u <= OW + 1) & (v >= -2) & (v <= OH + 1)
            csel = np.flatnonzero(close)
            cx, cy = np.floor(u[csel]).astype(np.int64), np.floor(v[csel]).astype(np.int64)
            _, ctgt = _footprint(cx, cy, np.arange(csel.size), radius + 1, OH, OW)
            near[m][ctgt] = True
    index = index.astype(np.int32).reshape(M, OH, OW)
    color = None
    if colors is not None:
        bg = np.array([(background >> 16) & 255, (background >> 8) & 255, background & 255], np.uint8)
        src = colour_bytes(colors).transpose(0, 2, 3, 1).reshape(-1, 3)     # the PLY export's bytes of every source pixel
        color = np.where((index >= 0)[..., None], src[np.maximum(index, 0)], bg)
    return dict(color=color, depth=depth.reshape(M, OH, OW), index=index, near=near.reshape(M, OH, OW), landed=landed)


def brute(points, mask, poses, K, skip, OH, OW, radius):
    """the same answer point by point in Python floats (fp64): (depth [M,OH,OW], index [M,OH,OW]); for small scenes"""
    N, H, W = points.shape[:3]
    M = poses.shape[0]
    depth, index = np.zeros((M, OH, OW)), np.full((M, OH, OW), -1, np.int64)
    flat = points.reshape(-1, 3).astype(np.float64)
    for m in range(M):
        R, t, k = poses[m, :3, :3].astype(np.float64), poses[m, :3, 3].astype(np.float64), K[m].astype(np.float64)
        for p, P in enumerate(flat):
            if (mask is not None and not np.asarray(mask).reshape(-1)[p]) or not np.isfinite(P).all():
                continue
            if skip is not None and p // (H * W) == skip[m]:
                continue
            d = P - t
            q = [(R[0, j] * d[0] + R[1, j] * d[1]) + R[2, j] * d[2] for j in range(3)]
            if not (q[2] > 0 and np.isfinite(q[2])):
                continue
            u, v = k[0, 0] * (q[0] / q[2]) + k[0, 2], k[1, 1] * (q[1] / q[2]) + k[1, 2]
            if not (0 <= u < OW and 0 <= v < OH):
                continue
            x0, y0 = int(u), int(v)
            for ty in range(max(y0 - radius, 0), min(y0 + radius, OH - 1) + 1):
                for tx in range(max(x0 - radius, 0), min(x0 + radius, OW - 1) + 1):
                    if index[m, ty, tx] < 0 or q[2] < depth[m, ty, tx]:      # p ascends: an equal depth keeps the lower index
                        depth[m, ty, tx], index[m, ty, tx] = q[2], p
    return depth, index


def scene_colors(N, H, W, seed=0):
    """fp32 [N,3,H,W] in [-0.1, 1.1]: some channels clip at both ends"""
    return (np.random.default_rng(1000 + seed).random((N, 3, H, W)) * 1.2 - 0.1).astype(np.float32)


def targets(s, M, OH, OW, seed=0):
    """M target cameras for a consistency_check.scene: its own cameras first (rescaled to OH x OW), then cameras in between"""
    N = s["poses"].shape[0]
    poses, K = np.zeros((M, 4, 4), np.float64), np.zeros((M, 3, 3), np.float64)
    for m in range(M):
        if m < N and m % 2 == 0:
            poses[m] = s["poses"][m]
        else:
            a = 0.7 * np.pi * (m + 0.37) / max(M, N)
            c = np.array([3.6 * np.cos(a), 3.6 * np.sin(a), 2.3])
            poses[m, :3, :3], poses[m, :3, 3], poses[m, 3, 3] = look_at_origin(c), c, 1.0
        K[m] = [[0.9 * OW, 0, OW / 2.0], [0, 0.9 * OW, OH / 2.0], [0, 0, 1]]
    return poses.astype(np.float32), K.astype(np.float32)
