"""The image-mesh rule that csrc/mesh.hip is held to (include/g2vlm_hip.h states it), restated in numpy.  Checker side only:
nothing here is imported by the product.  The scene and the masks are those of tests/consistency_check.py.

rule(...) evaluates the rule in the dtype it is given.  In float32 every ufunc call is one fp32 operation rounded once - separate
calls cannot fuse - which is what the kernel does with contraction switched off, so the two agree byte for byte.  In float64 the
same code is the yardstick for how much of the diagonal choice hangs on rounding."""
import numpy as np

from consistency_check import _fma, random_mask, scene  # noqa: F401  (re-exported for the tests)
from render_check import colour_bytes

FUSED = ("inner", "inner_swapped", "outer", "both", "both_swapped")   # the ways a compiler may contract (d0 d0 + d1 d1) + d2 d2
A1, A2, M1, M2 = 1, 2, 4, 8                                  # the bit of a triangle in a quad's code, in face order
# corner (dy, dx) of each triangle's A, B, C
TRIANGLES = (((0, 0), (1, 0), (0, 1)), ((0, 1), (1, 0), (1, 1)), ((0, 0), (1, 0), (1, 1)), ((0, 0), (1, 1), (0, 1)))
FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
VERTEX_DTYPE = np.dtype([("p", "<f4", (3,)), ("c", "u1", (3,))])


def edge2(a, b, fused=None):
    """d = a - b; (d0 d0 + d1 d1) + d2 d2 as the rule has it, or - NOT the rule - with the sums contracted (fp32 only)"""
    d = a - b
    d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
    if fused is None:
        return (d0 * d0 + d1 * d1) + d2 * d2
    inner = {"inner": lambda: _fma(d0, d0, d1 * d1), "inner_swapped": lambda: _fma(d1, d1, d0 * d0), "outer": lambda: d0 * d0 + d1 * d1,
             "both": lambda: _fma(d0, d0, d1 * d1), "both_swapped": lambda: _fma(d1, d1, d0 * d0)}[fused]()
    return inner + d2 * d2 if fused.startswith("inner") else _fma(d2, d2, inner)


def rule(points, mask=None, max_edge=None, dtype=np.float32, fused=None):
    """points fp32 [N,H,W,3], mask bool / uint8 [N,H,W] or None, max_edge a number or None (the stretch filter is off).
    Returns dict(code uint8 [N,H,W] = the triangles of the quad anchored at the pixel, one bit each, used uint8 [N,H,W], vertex_of
    int32 [N,H,W], vertex_pixel int32 [V], faces int32 [F,3], face_pixels int64 [F,3] = the faces in flat pixels, face_records
    uint8 [F,13], counts int32 [N,2], and of every quad [N,H-1,W-1]: anti bool = the anti diagonal is the shorter one, ea / em =
    the diagonals' squared lengths, four bool = all corners kept)."""
    f = dtype
    assert fused is None or f is np.float32
    N, H, W = points.shape[:3]
    keep = np.ones((N, H, W), bool) if mask is None else np.asarray(mask) != 0
    code = np.zeros((N, H, W), np.uint8)
    out = dict(anti=np.zeros((N, max(H - 1, 0), max(W - 1, 0)), bool))
    out["ea"] = out["em"] = np.zeros(out["anti"].shape, f)
    out["four"] = out["anti"]
    if H >= 2 and W >= 2:
        P = points.astype(f)
        p00, p01, p10, p11 = P[:, :-1, :-1], P[:, :-1, 1:], P[:, 1:, :-1], P[:, 1:, 1:]
        k00, k01, k10, k11 = keep[:, :-1, :-1], keep[:, :-1, 1:], keep[:, 1:, :-1], keep[:, 1:, 1:]
        with np.errstate(all="ignore"):
            n = k00.astype(int) + k01 + k10 + k11
            ea, em = edge2(p01, p10, fused), edge2(p00, p11, fused)
            anti = ea < em                                    # false on a tie and on NaN
            four, three = n == 4, n == 3
            t = [(four & anti) | (three & ~k11), (four & anti) | (three & ~k00), (four & ~anti) | (three & ~k01), (four & ~anti) | (three & ~k10)]
            if max_edge is not None:
                lim = f(np.float32(max_edge)) * f(np.float32(max_edge))
                top, left, right, bottom = (edge2(p00, p01, fused) <= lim, edge2(p00, p10, fused) <= lim, edge2(p01, p11, fused) <= lim,
                                            edge2(p10, p11, fused) <= lim)
                da, dm = ea <= lim, em <= lim
                t = [t[0] & left & da & top, t[1] & da & bottom & right, t[2] & left & bottom & dm, t[3] & dm & right & top]
        code[:, :-1, :-1] = t[0] * A1 + t[1] * A2 + t[2] * M1 + t[3] * M2
        out.update(anti=anti, ea=ea, em=em, four=four)
    pix = np.arange(N * H * W, dtype=np.int64).reshape(N, H, W)
    corner = np.stack([np.stack([pix + dy * W + dx for dy, dx in tri], -1) for tri in TRIANGLES], -2)    # [N,H,W,4,3]
    bits = (code[..., None] >> np.arange(4)) & 1
    face_pixels = corner[bits != 0]                           # boolean indexing walks in C order: view, row, column, triangle
    used = np.zeros(N * H * W, np.uint8)
    used[face_pixels.reshape(-1)] = 1
    vertex_of = np.where(used != 0, np.cumsum(used, dtype=np.int64) - 1, -1).astype(np.int32)
    faces = vertex_of[face_pixels].reshape(-1, 3)
    rec = np.zeros(len(faces), FACE_DTYPE)
    rec["n"], rec["v"] = 3, faces
    counts = np.stack([used.reshape(N, -1).sum(1, dtype=np.int64), bits.reshape(N, -1).sum(1, dtype=np.int64)], 1).astype(np.int32)
    out.update(code=code, used=used.reshape(N, H, W), vertex_of=vertex_of.reshape(N, H, W), vertex_pixel=np.flatnonzero(used).astype(np.int32),
               faces=faces, face_pixels=face_pixels.reshape(-1, 3), face_records=rec.view(np.uint8).reshape(-1, 13), counts=counts)
    return out


def vertex_records(points, colors, used):
    """g2v_cloud_compact's 15-byte records of the used pixels: points fp32 [N,H,W,3], colors fp32 [N,3,H,W]"""
    sel = np.asarray(used).reshape(-1) != 0
    rec = np.zeros(int(sel.sum()), VERTEX_DTYPE)
    rec["p"] = points.reshape(-1, 3)[sel]
    rec["c"] = colour_bytes(np.moveaxis(colors, 1, -1).reshape(-1, 3)[sel])
    return rec.view(np.uint8).reshape(-1, 15)


def brute(points, mask=None, max_edge=None):
    """the rule quad by quad in a Python loop, fp32: (faces in flat pixels [F,3], used bool [N,H,W])"""
    f = np.float32
    N, H, W = points.shape[:3]
    keep = np.ones((N, H, W), bool) if mask is None else np.asarray(mask) != 0
    faces, used = [], np.zeros((N, H, W), bool)

    def e2(a, b):
        d0, d1, d2 = f(a[0] - b[0]), f(a[1] - b[1]), f(a[2] - b[2])
        return f(f(f(d0 * d0) + f(d1 * d1)) + f(d2 * d2))

    with np.errstate(all="ignore"):
        for i in range(N):
            for y in range(H - 1):
                for x in range(W - 1):
                    c = {"00": (y, x), "01": (y, x + 1), "10": (y + 1, x), "11": (y + 1, x + 1)}
                    kept = [k for k, (a, b) in c.items() if keep[i, a, b]]
                    pt = {k: points[i, a, b] for k, (a, b) in c.items()}
                    if len(kept) == 4:
                        tris = [("00", "10", "01"), ("01", "10", "11")] if e2(pt["01"], pt["10"]) < e2(pt["00"], pt["11"]) else \
                            [("00", "10", "11"), ("00", "11", "01")]
                    elif len(kept) == 3:
                        missing = (set(c) - set(kept)).pop()
                        tris = [{"11": ("00", "10", "01"), "00": ("01", "10", "11"), "01": ("00", "10", "11"), "10": ("00", "11", "01")}[missing]]
                    else:
                        tris = []
                    for tri in tris:
                        if max_edge is not None:
                            lim = f(f(max_edge) * f(max_edge))
                            if not all(e2(pt[tri[a]], pt[tri[b]]) <= lim for a, b in ((0, 1), (1, 2), (2, 0))):
                                continue
                        faces.append([(i * H + c[k][0]) * W + c[k][1] for k in tri])
                        for k in tri:
                            used[(i,) + c[k]] = True
    return np.array(faces, np.int64).reshape(-1, 3), used


def toward_camera(points, face_pixels, centre):
    """(B - A) x (C - A) . (centre - A) of every face, fp64: positive where the face looks at the camera centre"""
    P = points.reshape(-1, 3).astype(np.float64)
    a, b, c = P[face_pixels[:, 0]], P[face_pixels[:, 1]], P[face_pixels[:, 2]]
    return (np.cross(b - a, c - a) * (np.asarray(centre, np.float64) - a)).sum(-1)


def scene_colors(N, H, W, seed=0):
    """colours fp32 [N,3,H,W] in [-0.1, 1.1]: both clips of the colour byte are met"""
    return np.random.default_rng(1000 + seed).uniform(-0.1, 1.1, (N, 3, H, W)).astype(np.float32)


def checkerboard(N, H, W):
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.broadcast_to(((y + x) % 2).astype(np.uint8), (N, H, W)).copy()


def depth_edge_mask(local, rtol=0.03):
    """the reference's depth_edge on local[..., 2] (3 x 3 window, in-bounds pixels only) as g2v_cloud_mask applies it, with the finite
    test of the depth: fp32, NaN in the window means "not an edge", q = diff / d with NaN -> 0.  uint8 [N,H,W] = kept."""
    z = local[..., 2].astype(np.float32)
    N, H, W = z.shape
    mx = np.full((N, H, W), -np.inf, np.float32)
    mn = np.full((N, H, W), -np.inf, np.float32)
    has_nan = np.zeros((N, H, W), bool)
    pad = np.pad(z, ((0, 0), (1, 1), (1, 1)), constant_values=np.float32(0))
    inb = np.pad(np.ones((H, W), bool), 1)
    with np.errstate(all="ignore"):
        for dy in range(3):
            for dx in range(3):
                v, ok = pad[:, dy:dy + H, dx:dx + W], inb[dy:dy + H, dx:dx + W]
                has_nan |= ok & np.isnan(v)
                mx = np.where(ok & (v > mx), v, mx)
                mn = np.where(ok & (-v > mn), -v, mn)
        q = (mx + mn) / z
        q = np.where(np.isnan(q), np.float32(0), q)
        edge = ~has_nan & (q > np.float32(rtol))
    return (np.isfinite(z) & ~edge).astype(np.uint8)
