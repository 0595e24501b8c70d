"""The multi-view consistency rule that csrc/consistency.hip is held to (include/g2vlm_hip.h states it), restated in numpy, and a
synthetic scene to run it on.  Checker side only: nothing here is imported by the product.

rule(...) evaluates the rule in the dtype it is given.  In float32 every ufunc call is one fp32 operation rounded once - separate
calls cannot fuse - which is what the kernel does with contraction switched off, so the two agree byte for byte.  In float64 the
same code is the yardstick for how much of the answer hangs on rounding: margins() marks the pixels that sit within 1e-4 of a
decision, and outside that set both dtypes must give the same counts."""
import numpy as np


FUSED_Q = ("inner", "outer", "both", "both_swapped")          # the ways a compiler may contract (a d0 + b d1) + c d2


def _fma(a, b, c):
    """fp32 a * b + c rounded once (the fp64 product of two fp32 numbers is exact)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def rotate(Rj, d0, d1, d2, k, fused_q=None):
    """q_k = (R[0][k] d0 + R[1][k] d1) + R[2][k] d2 as the rule has it, or - NOT the rule - with the sums contracted"""
    a, b, c = Rj[0, k], Rj[1, k], Rj[2, k]
    if fused_q is None:
        return (a * d0 + b * d1) + c * d2
    inner = {"inner": lambda: _fma(a, d0, b * d1), "outer": lambda: a * d0 + b * d1, "both": lambda: _fma(a, d0, b * d1),
             "both_swapped": lambda: _fma(b, d1, a * d0)}[fused_q]()
    return inner + c * d2 if fused_q == "inner" else _fma(c, d2, inner)


def rule(points, local, poses, K, mask, depth_rtol, dtype=np.float32, min_agree=0, max_in_front=-1, fused_uv=False, fused_q=None):
    """points, local fp32 [N,H,W,3], poses fp32 [N,4,4] camera-to-world, K fp32 [N,3,3], mask bool / uint8 [N,H,W] or None.
    Returns dict(agree uint8 [N,H,W], in_front uint8 [N,H,W], pairs int32 [N,N,2], mask_out bool [N,H,W], eligible bool [N,H,W],
    agree_in / front_in bool [N,N,H,W] = the class of pixel (i, p) in target j, near bool [N,H,W] = some target's decision for
    the pixel lies within 1e-4 of a threshold).
    fused_uv: u and v as a fused multiply-add would give them (one rounding of fx r + cx) - NOT the rule; the GPU test uses it to
    show that its scene tells the two apart.  fused_q (one of FUSED_Q, fp32 only): the same for the sums of R^T d."""
    f = dtype
    assert fused_q is None or f is np.float32
    N, H, W = points.shape[:3]
    P = points.astype(f)
    z = local[..., 2].astype(f)
    R, t = poses[:, :3, :3].astype(f), poses[:, :3, 3].astype(f)
    Kf = K.astype(f)
    rtol = f(np.float32(depth_rtol))
    keep = np.ones((N, H, W), bool) if mask is None else np.asarray(mask) != 0
    eligible = keep & np.isfinite(points).all(-1)
    zvalid = keep & np.isfinite(local[..., 2]) & (local[..., 2] > 0)
    agree_in = np.zeros((N, N, H, W), bool)
    front_in = np.zeros((N, N, H, W), bool)
    near = np.zeros((N, H, W), bool)
    with np.errstate(all="ignore"):
        for j in range(N):
            d0, d1, d2 = P[..., 0] - t[j, 0], P[..., 1] - t[j, 1], P[..., 2] - t[j, 2]
            q = [rotate(R[j], d0, d1, d2, k, fused_q) for k in range(3)]
            r0, r1 = q[0] / q[2], q[1] / q[2]
            if fused_uv:
                u = (Kf[j, 0, 0].astype(np.float64) * r0.astype(np.float64) + Kf[j, 0, 2].astype(np.float64)).astype(f)
                v = (Kf[j, 1, 1].astype(np.float64) * r1.astype(np.float64) + Kf[j, 1, 2].astype(np.float64)).astype(f)
            else:
                u = Kf[j, 0, 0] * r0 + Kf[j, 0, 2]
                v = Kf[j, 1, 1] * r1 + Kf[j, 1, 2]
            inside = (q[2] > 0) & (u >= 0) & (u < f(W)) & (v >= 0) & (v < f(H))
            x = np.where(inside, u, 0).astype(np.int64)       # converted only where inside; truncation = floor there
            y = np.where(inside, v, 0).astype(np.int64)
            zt = z[j][y, x]
            valid = inside & zvalid[j][y, x]
            tol, diff = rtol * zt, q[2] - zt
            a = valid & (np.abs(diff) <= tol)
            b = valid & (diff < -tol)
            other = eligible & (np.arange(N) != j)[:, None, None]
            agree_in[:, j], front_in[:, j] = a & other, b & other
            close = (np.abs(u - np.rint(u)) <= 1e-4) | (np.abs(v - np.rint(v)) <= 1e-4) | (np.abs(q[2]) <= 1e-4) | \
                    (valid & (np.abs(np.abs(diff) - tol) <= 1e-4 * zt))
            near |= close & other
    agree, in_front = agree_in.sum(1), front_in.sum(1)
    pairs = np.stack([agree_in.sum((2, 3)), front_in.sum((2, 3))], -1).astype(np.int32)
    mask_out = eligible & (agree >= min_agree) & ((max_in_front < 0) | (in_front <= max_in_front))
    return dict(agree=agree.astype(np.uint8), in_front=in_front.astype(np.uint8), pairs=pairs, mask_out=mask_out, eligible=eligible,
                agree_in=agree_in, front_in=front_in, near=near)


def mask_out(res, min_agree, max_in_front):
    """mask_out of a rule() result under other thresholds"""
    return res["eligible"] & (res["agree"] >= min_agree) & ((max_in_front < 0) | (res["in_front"] <= max_in_front))


def look_at_origin(c):
    """camera-to-world rotation of a camera at c that looks at the origin, z up: columns = right, down, forward"""
    fwd = -c / np.linalg.norm(c)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(fwd, right), fwd], 1)


def scene(N, H, W, seed=0, flying=0.02, noise=0.002):
    """A floor z = 0 and a sphere of radius 0.8 on it, seen by N cameras on an arc.  Camera i is at (4 cos a, 4 sin a, 2 + 0.3
    (i mod 3)), a = 0.7 pi i / N, and looks at the origin; fx = fy = 0.9 W, principal point at the centre; rays through pixel
    centres.  Depth carries `noise` multiplicative Gaussian noise, and a share `flying` of the pixels is pulled toward the camera
    by a factor uniform in [0.5, 0.9].  A ray that hits nothing (above the horizon) gives NaN.  Everything is formed in fp64 and
    rounded to fp32 once.  Returns dict(points, local fp32 [N,H,W,3], poses fp32 [N,4,4], K fp32 [N,3,3], flying bool [N,H,W])."""
    rng = np.random.default_rng(seed)
    fx = fy = 0.9 * W
    cx, cy = W / 2.0, H / 2.0
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    ray = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], -1)          # local = ray * depth
    points, local = np.empty((N, H, W, 3)), np.empty((N, H, W, 3))
    poses, fly = np.zeros((N, 4, 4)), np.zeros((N, H, W), bool)
    centre, rad = np.array([0.0, 0.0, 0.8]), 0.8
    for i in range(N):
        a = 0.7 * np.pi * i / N
        c = np.array([4 * np.cos(a), 4 * np.sin(a), 2 + 0.3 * (i % 3)])
        R = look_at_origin(c)
        D = ray @ R.T                                                              # world direction per unit of depth
        with np.errstate(all="ignore"):
            s_floor = np.where(D[..., 2] < 0, -c[2] / D[..., 2], np.inf)
            oc = c - centre
            A, B, Cq = (D * D).sum(-1), 2 * (D @ oc), oc @ oc - rad * rad
            disc = B * B - 4 * A * Cq
            s_sph = np.where(disc >= 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), np.inf)
            s_sph = np.where(s_sph > 0, s_sph, np.inf)
        depth = np.minimum(s_floor, s_sph)
        depth = np.where(np.isfinite(depth), depth, np.nan)
        depth = depth * (1 + noise * rng.standard_normal((H, W)))
        fly[i] = rng.random((H, W)) < flying
        depth = np.where(fly[i], depth * rng.uniform(0.5, 0.9, (H, W)), depth)
        local[i] = ray * depth[..., None]
        points[i] = local[i] @ R.T + c
        poses[i, :3, :3], poses[i, :3, 3], poses[i, 3, 3] = R, c, 1.0
    fly &= np.isfinite(local[..., 2])
    K = np.tile(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]), (N, 1, 1))
    return dict(points=points.astype(np.float32), local=local.astype(np.float32), poses=poses.astype(np.float32),
                K=K.astype(np.float32), flying=fly)


def random_mask(shape, seed, keep=0.8):
    return (np.random.default_rng(seed).random(shape) < keep).astype(np.uint8)


def fma_scene(H=4, W=70, focals=(62.7, 61.3, 63.9, 60.1)):
    """Views with identical identity poses whose pixels tell a fused u = fma(fx, r, cx) from the rule's two roundings.
    With R = I, t = 0 and Pz = 1 the projection is exact up to u: q = P, r = Px.  For every target view (one focal length each)
    and every integer m the search takes the fp32 neighbours of (m - cx) / fx and keeps those where the two-step u and the
    once-rounded u fall in different pixels.  Every target depth plane is 1 on even columns (q2 = 1 agrees) and 2 on odd ones
    (q2 = 1 lies in front), so the two pixels classify differently.  The found points are the pixels of view 0.
    Returns (scene dict, picked bool [N,H,W]: the pixels of view 0 whose counts differ between the rule and the fused form)."""
    N = 1 + len(focals)
    cx, cy = np.float32(35.3), np.float32(H / 2.0)
    m = np.repeat(np.arange(1, W - 1), 17)
    off = np.tile(np.arange(-8, 9), W - 2).astype(np.int32)
    found = []
    for fx in np.asarray(focals, np.float32):
        r = ((m - np.float64(cx)) / np.float64(fx)).astype(np.float32)
        r = (r.view(np.int32) + off).view(np.float32)
        two = fx * r + cx
        one = (np.float64(fx) * r.astype(np.float64) + np.float64(cx)).astype(np.float32)
        found += r[np.floor(two) != np.floor(one)].tolist()
    found = np.array(sorted(set(found)), dtype=np.float32)
    assert found.size <= H * W
    points = np.full((N, H, W, 3), np.nan, np.float32)
    flat = points.reshape(N, -1, 3)
    flat[0, :found.size] = np.stack([found, np.zeros_like(found), np.ones_like(found)], 1)     # v = cy: row H / 2
    flat[1:, ::3] = (0.1, 0.0, 1.0)                                                            # generic points for the other directions
    local = np.zeros((N, H, W, 3), np.float32)
    local[..., 2] = np.where(np.arange(W) % 2 == 0, 1.0, 2.0).astype(np.float32)
    poses = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    K = np.tile(np.array([[focals[0], 0, cx], [0, 62.7, cy], [0, 0, 1]], np.float32), (N, 1, 1))
    K[1:, 0, 0] = focals
    sc = dict(points=points, local=local, poses=poses, K=K)
    a = rule(points, local, poses, K, None, 0.25)
    b = rule(points, local, poses, K, None, 0.25, fused_uv=True)
    picked = (a["agree"] != b["agree"]) | (a["in_front"] != b["in_front"])
    return sc, picked


def fma_pose_scene(H=4, W=70, candidates=40000, seed=3):
    """Two views; view 1's pose is a rotation about a generic axis and a translation, so all nine products of R^T d are inexact.
    The pixels of view 0 are points on the plane q2 = 1.25 of view 1, where with depth 1 everywhere and depth_rtol = 0.25 the rule
    decides by `q2 - 1 <= 0.25`: a q2 that a contracted sum moves across 1.25 by an ulp changes the class (agree against neither).
    Of `candidates` random points on that plane the scene keeps, for every form of FUSED_Q, H W / 4 on which it differs from the rule.
    Returns (scene dict, {form: bool [N,H,W], the pixels whose counts differ between the rule and that form})."""
    rng = np.random.default_rng(seed)
    axis = np.array([0.48, -0.6, 0.64])
    ang = 0.83
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)
    t = np.array([0.3, -0.2, 0.1])
    cam = np.stack([rng.uniform(-0.8, 0.8, candidates), rng.uniform(-0.8, 0.8, candidates), np.full(candidates, 1.25)], 1)
    P = (cam @ R.T + t).astype(np.float32)
    R32, t32 = R.astype(np.float32), t.astype(np.float32)
    d = [P[:, k] - t32[k] for k in range(3)]
    plain = rotate(R32, *d, 2) <= np.float32(1.25)
    taken = np.zeros(candidates, bool)
    for form in FUSED_Q:                                       # a quarter of the pixels from each form's own finds
        differs = ((rotate(R32, *d, 2, form) <= np.float32(1.25)) != plain) & ~taken
        taken[np.flatnonzero(differs)[:H * W // len(FUSED_Q)]] = True
    P = P[taken]
    points = np.full((2, H, W, 3), np.nan, np.float32)
    points[0].reshape(-1, 3)[:len(P)] = P
    local = np.zeros((2, H, W, 3), np.float32)
    local[..., 2] = 1.0
    poses = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    poses[1, :3, :3], poses[1, :3, 3] = R32, t32
    K = np.tile(np.array([[20.0, 0, W / 2.0], [0, 1.0, H / 2.0], [0, 0, 1]], np.float32), (2, 1, 1))
    a = rule(points, local, poses, K, None, 0.25)
    picked = {}
    for form in FUSED_Q:
        b = rule(points, local, poses, K, None, 0.25, fused_q=form)
        picked[form] = (a["agree"] != b["agree"]) | (a["in_front"] != b["in_front"])
    return dict(points=points, local=local, poses=poses, K=K), picked
