"""Helper (no tests): numpy restatements of what csrc/cloud.hip computes, written from the rules and not from the kernels.

  edge_mask      the reference's depth_edge (modeling/pi3/utils/geometry.py:339; 3x3 window, no mask) pixel by pixel in fp32
  keep_mask      the export's keep mask: finite world point, confidence logit above the threshold, not an edge
  pack_records   stable compaction + PLY record packing through host.write_ply_binary's own arithmetic
  fit_intrinsics the per-view pinhole fit as np.linalg.lstsq in fp64
  edge_cases     the depth maps of the committed fixture (tools/gen_depth_edge_golden.py writes it from the same function)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FLT_MAX = np.finfo(np.float32).max
EDGE_SHAPES = ((1, 1), (1, 7), (5, 1), (9, 13), (17, 33), (37, 70))
EDGE_N = 3
EDGE_TOLS = ((0.05, None), (None, 0.03), (0.05, 0.03), (0.0, 0.0))          # (atol, rtol)
GOLDEN = os.path.join(HERE, "golden", "depth_edge_cases")                  # + .safetensors / .json


def edge_cases():
    """{name: fp32 depth [EDGE_N, H, W]}: smooth positive depth with steps, then NaN, +-inf, 0, -0 and negatives sprinkled in,
    view by view more of them (view 0 stays clean)."""
    out = {}
    for h, w in EDGE_SHAPES:
        rng = np.random.default_rng(1000 * h + w)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        d = np.empty((EDGE_N, h, w), dtype=np.float32)
        for n in range(EDGE_N):
            base = 1.5 + 0.01 * xx + 0.02 * yy + 0.005 * rng.standard_normal((h, w)).astype(np.float32)
            base[(xx + 2 * yy) > (w + 2 * h) * 0.5] += np.float32(0.3 * (n + 1))          # a depth step across the view
            d[n] = base
            if n:
                special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.25, -0.01], dtype=np.float32)
                hit = rng.random((h, w)) < 0.06 * n
                d[n][hit] = special[rng.integers(0, len(special), int(hit.sum()))]
        out[f"d_{h}x{w}"] = d
    return out


def edge_mask(depth, atol=None, rtol=None):
    """bool [..., H, W]: True where the pixel is a depth edge.  Per pixel over the in-bounds part of its 3x3 window: a NaN in it
    means no edge; else diff = max(window) + max(-window) in fp32; edge if diff > atol, or if nan_to_num(diff / centre) > rtol."""
    depth = np.asarray(depth, dtype=np.float32)
    shape = depth.shape
    d = depth.reshape(-1, shape[-2], shape[-1])
    edge = np.zeros(d.shape, dtype=bool)
    h, w = d.shape[1:]
    with np.errstate(all="ignore"):
        for n in range(d.shape[0]):
            for y in range(h):
                for x in range(w):
                    win = d[n, max(y - 1, 0):min(y + 2, h), max(x - 1, 0):min(x + 2, w)].ravel()
                    if np.isnan(win).any():
                        continue
                    diff = np.float32(win.max()) + np.float32((-win).max())
                    e = False
                    if atol is not None:
                        e = bool(diff > np.float32(atol))
                    if rtol is not None:
                        q = np.float32(diff) / d[n, y, x]
                        if np.isnan(q):
                            q = np.float32(0)
                        elif np.isposinf(q):
                            q = FLT_MAX
                        elif np.isneginf(q):
                            q = -FLT_MAX
                        e = e or bool(q > np.float32(rtol))
                    edge[n, y, x] = e
    return edge.reshape(shape)


def keep_mask(points=None, local=None, conf=None, conf_logit_min=None, atol=None, rtol=None, finite=True):
    """bool [N,H,W]: the pixels the export keeps.  conf / conf_logit_min: fp32 logits and an fp32 threshold, compared as they are."""
    keep = None
    if finite:
        keep = np.isfinite(np.asarray(points, dtype=np.float32)).all(-1)
    if conf_logit_min is not None:
        c = np.asarray(conf, dtype=np.float32) > np.float32(conf_logit_min)                 # NaN > x is False
        keep = c if keep is None else keep & c
    if atol is not None or rtol is not None:
        e = ~edge_mask(np.asarray(local, dtype=np.float32)[..., 2], atol, rtol)
        keep = e if keep is None else keep & e
    return keep


def pack_records(points, colors, mask):
    """(records uint8 [M,15], counts int64 [N]) for points fp32 [N,H,W,3], colors fp32 [N,3,H,W], mask bool [N,H,W]: numpy boolean
    indexing (view-major, row-major) and the bytes host.write_ply_binary writes behind its header."""
    import tempfile
    from g2vlm_amd import host
    points, colors, mask = np.asarray(points, dtype=np.float32), np.asarray(colors, dtype=np.float32), np.asarray(mask).astype(bool)
    p = points.reshape(-1, 3)[mask.reshape(-1)]
    c = colors.transpose(0, 2, 3, 1).reshape(-1, 3)[mask.reshape(-1)]
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "ref.ply")
        host.write_ply_binary(path, p, c)
        body = open(path, "rb").read().split(b"end_header\n", 1)[1]
    rec = np.frombuffer(body, dtype=np.uint8).reshape(-1, 15)
    assert rec.shape[0] == int(mask.sum())
    return rec, mask.reshape(mask.shape[0], -1).sum(1)


def fit_intrinsics(local, mask=None):
    """(K fp64 [N,3,3], used int [N]) by np.linalg.lstsq in fp64 on the fp32 inputs: u = x + 0.5 against [X/Z, 1], v = y + 0.5
    against [Y/Z, 1], over the pixels mask keeps with finite X, Y, Z and Z > 0.  Fewer than 2 pixels, or ratios that do not vary:
    NaN in the entries they would determine."""
    local = np.asarray(local, dtype=np.float32)
    n_views, h, w, _ = local.shape
    K = np.zeros((n_views, 3, 3))
    K[:, 2, 2] = 1.0
    used = np.zeros(n_views, dtype=np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    for n in range(n_views):
        ok = np.isfinite(local[n]).all(-1) & (local[n, ..., 2] > 0)
        if mask is not None:
            ok &= np.asarray(mask[n]).astype(bool)
        used[n] = int(ok.sum())
        z = local[n, ..., 2][ok].astype(np.float64)
        for axis, ratio, pix in ((0, local[n, ..., 0][ok].astype(np.float64) / z, xx[ok] + 0.5),
                                 (1, local[n, ..., 1][ok].astype(np.float64) / z, yy[ok] + 0.5)):
            if used[n] < 2 or np.ptp(ratio) == 0.0:
                K[n, axis, axis] = K[n, axis, 2] = np.nan
                continue
            sol = np.linalg.lstsq(np.stack([ratio, np.ones_like(ratio)], 1), pix, rcond=None)[0]
            K[n, axis, axis], K[n, axis, 2] = sol
    return K, used
