"""The surface-normal rule that csrc/normals.hip is held to (include/g2vlm_hip.h states it), restated in numpy.  Checker side only:
nothing here is imported by the product.  The scene and the masks are those of tests/mesh_check.py.

rule(...) evaluates the rule in the dtype it is given.  In float32 every ufunc call is one fp32 operation rounded once - separate
calls cannot fuse - which is what the kernel does with contraction switched off, so the two agree byte for byte.  In float64 the
same code is the yardstick for how much of a normal hangs on rounding."""
import numpy as np

from consistency_check import _fma
from mesh_check import checkerboard, depth_edge_mask, random_mask, scene, scene_colors  # noqa: F401  (re-exported for the tests)
from render_check import colour_bytes

NEIGHBOURS = ((0, 1), (1, 0), (0, -1), (-1, 0))              # (dy, dx) in units of step: R, D, L, U
PAIRS = ((0, 1), (1, 2), (2, 3), (3, 0))                     # (R,D) (D,L) (L,U) (U,R)
FUSED = ("minuend", "subtrahend")                            # the two ways a compiler may contract a b - c d
RECORD_DTYPE = np.dtype([("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))])
assert RECORD_DTYPE.itemsize == 27


def shifted(a, dy, dx, fill):
    """out[:, y, x] = a[:, y + dy, x + dx] where that lies inside the view, `fill` elsewhere"""
    H, W = a.shape[1:3]
    out = np.full_like(a, fill)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y1 > y0 and x1 > x0:
        out[:, y0:y1, x0:x1] = a[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def diff_of_products(a, b, c, d, fused=None):
    """a b - c d: each product rounded, then the difference (the rule) or - NOT the rule, fp32 only - as one fused multiply-add
    with the other product rounded first"""
    if fused is None:
        return a * b - c * d
    if fused == "minuend":
        return _fma(a, b, -(c * d))
    return _fma(-c, d, a * b)


def cross(a, b, fused=None):
    return np.stack([diff_of_products(a[..., 1], b[..., 2], a[..., 2], b[..., 1], fused),
                     diff_of_products(a[..., 2], b[..., 0], a[..., 0], b[..., 2], fused),
                     diff_of_products(a[..., 0], b[..., 1], a[..., 1], b[..., 0], fused)], -1)


def sumsq(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def rule(points, mask=None, poses=None, step=1, max_edge=None, dtype=np.float32, fused=None):
    """points fp32 [N,H,W,3], mask bool / uint8 [N,H,W] or None, poses fp32 [N,4,4] or None (the camera at the origin), step >= 1,
    max_edge a number or None (no limit).  Returns dict(normals [N,H,W,3], valid uint8 [N,H,W], cos_view [N,H,W], colors [N,3,H,W]
    in `dtype`, pairs int [N,H,W] = the number of neighbour pairs that were there (0 where the pixel takes no part), part bool
    [N,H,W], t [N,H,W] = n . d before the flip)."""
    f = dtype
    assert fused is None or f is np.float32
    N, H, W = points.shape[:3]
    keep = np.ones((N, H, W), bool) if mask is None else np.asarray(mask) != 0
    part = keep & np.isfinite(points).all(-1)
    P = points.astype(f)
    with np.errstate(all="ignore"):
        e, av = [], []
        for dy, dx in NEIGHBOURS:
            q = shifted(P, dy * step, dx * step, f(0))
            ok = shifted(part, dy * step, dx * step, False)
            d = q - P
            if max_edge is not None:
                lim = f(np.float32(max_edge)) * f(np.float32(max_edge))
                ok = ok & (sumsq(d) <= lim)
            e.append(d)
            av.append(ok)
        m = np.zeros((N, H, W, 3), f)
        have = np.zeros((N, H, W), bool)
        pairs = np.zeros((N, H, W), int)
        for a, b in PAIRS:
            present = av[a] & av[b] & part
            c = cross(e[a], e[b], fused)
            m = np.where((present & have)[..., None], m + c, np.where(present[..., None], c, m))   # starts from the first present product
            have |= present
            pairs += present
        s2 = sumsq(m)
        valid = part & have & np.isfinite(s2) & (s2 > 0)
        n = m / np.sqrt(s2)[..., None]
        C = np.zeros((N, 3), f) if poses is None else np.asarray(poses)[:, :3, 3].astype(f)
        d = P - C[:, None, None, :]
        t = (n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]
        n = np.where((t > 0)[..., None], -n, n)               # numpy's negation flips the sign bit: -0.0 where a component is +0.0
        q = np.abs(t) / np.sqrt(sumsq(d))
        q = np.where(np.isnan(q), f(0), q)
        cos_view = np.where(q < 1, q, f(1))
        colors = n * f(0.5) + f(0.5)
    zero = f(0)
    normals = np.where(valid[..., None], n, zero).astype(f)
    return dict(normals=normals, valid=valid.astype(np.uint8), cos_view=np.where(valid, cos_view, zero).astype(f),
                colors=np.ascontiguousarray(np.moveaxis(np.where(valid[..., None], colors, zero).astype(f), -1, 1)), pairs=pairs, part=part,
                t=np.where(valid, t, zero))


def edge_limits(points, mask, poses, step, tries=8):
    """(the median length of the edges to the R and D neighbours - a max_edge under which a good share of them fails -, a max_edge L
    whose fp32 square equals the squared length of one of those edges bit for bit and on which that edge hangs: under the next
    float below L some pixel has fewer pairs; None where the search finds none)"""
    part = np.isfinite(points).all(-1) & (True if mask is None else np.asarray(mask) != 0)
    e2 = []
    with np.errstate(all="ignore"):
        for dy, dx in NEIGHBOURS[:2]:
            d = sumsq(shifted(points, dy * step, dx * step, np.float32(0)) - points)
            e2.append(d[part & shifted(part, dy * step, dx * step, False) & np.isfinite(d)])
    e2 = np.concatenate(e2)
    if e2.size == 0:
        return 1.0, None
    cand = np.unique(e2)
    root = np.sqrt(cand)                                      # fp32
    hits = np.flatnonzero((root * root == cand) & (cand <= np.quantile(e2, 0.98)))   # not the few edges out to a flying pixel or the horizon
    for h in hits[::-1][:tries]:                             # the longest first: the pixel's other edges are then likely to be there
        L = float(root[h])
        on = rule(points, mask, poses, step, L)["pairs"]
        under = rule(points, mask, poses, step, float(np.nextafter(np.float32(L), np.float32(0))))["pairs"]
        if (on > under).any():
            return float(np.sqrt(np.median(e2))), L
    return float(np.sqrt(np.median(e2))), None


def records(points, normals, colors, mask):
    """g2v_cloud_compact_normals' 27-byte records of the pixels mask keeps: points, normals fp32 [N,H,W,3], colors fp32 [N,3,H,W]"""
    sel = np.asarray(mask).reshape(-1) != 0
    rec = np.zeros(int(sel.sum()), RECORD_DTYPE)
    rec["p"] = points.reshape(-1, 3)[sel]
    rec["n"] = normals.reshape(-1, 3)[sel]
    rec["c"] = colour_bytes(np.moveaxis(colors, 1, -1).reshape(-1, 3)[sel])
    return rec.view(np.uint8).reshape(-1, 27)


def angle_deg(a, b):
    """the angle between vectors a and b [...,3] in degrees: atan2(|a x b|, a . b) in fp64 (arccos of a dot loses everything below
    about 0.03 degrees in fp32 and much in fp64 near 0)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1)))
