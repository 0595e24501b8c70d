"""GPU: csrc/cloud.hip against tests/cloud_check.py - the keep mask bit for bit, the compacted PLY records byte for byte, the
intrinsics fit against fp64 lstsq.  Shapes are the smallest at which each kernel takes every path it has: views of 1 x 1, one
row, one column, sizes that are no multiple of the mask's 16 x 128 tile (and 17 x 129, one pixel past it both ways), pixel
counts around the compaction's 1024-pixel block, 2 x 518 x 518 (526 blocks: more than one pass of the 256-wide scan)."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cloud_check  # noqa: E402
from g2vlm_amd import hip, host  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE_H, TILE_W = 16, 128                                     # cloud.hip: CM_TH, CM_TW


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ the mask
_EDGE_CACHE = {}


def scene(name, depth):
    """A scene around a depth map [N,H,W]: local = (x, y, depth), world points with non-finite coordinates sprinkled in, confidence
    logits; the reference edge masks are computed once per (scene, tolerances) and shared."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n, h, w = depth.shape
    local = rng.standard_normal((n, h, w, 3)).astype(np.float32)
    local[..., 2] = depth
    points = rng.standard_normal((n, h, w, 3)).astype(np.float32)
    hit = rng.random((n, h, w, 3)) < 0.05
    points[hit] = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)[rng.integers(0, 3, int(hit.sum()))]
    conf = (2.0 * rng.standard_normal((n, h, w))).astype(np.float32)
    conf[rng.random((n, h, w)) < 0.03] = np.nan
    return dict(name=name, points=points, local=local, conf=conf)


def want_mask(s, finite, logit, atol, rtol):
    keep = cloud_check.keep_mask(s["points"], None, s["conf"], logit, None, None, finite) if (finite or logit is not None) else None
    if atol is not None or rtol is not None:
        key = (s["name"], atol, rtol)
        if key not in _EDGE_CACHE:
            _EDGE_CACHE[key] = cloud_check.edge_mask(s["local"][..., 2], atol, rtol)
        keep = ~_EDGE_CACHE[key] if keep is None else keep & ~_EDGE_CACHE[key]
    return keep


def got_mask(s, finite, logit, atol, rtol):
    m = hip.cloud_mask(dev(s["points"]), dev(s["local"]), dev(s["conf"]) if logit is not None else None, logit or 0.0, atol, rtol, finite=finite)
    assert m.dtype == torch.uint8 and int(m.max()) <= 1
    return m.cpu().numpy().astype(bool)


def _scenes():
    out = []
    for name, d in cloud_check.edge_cases().items():
        if name != "d_17x33":                                # the listed shapes: 1x1, 1x7, 5x1, 9x13, 37x70
            out.append((name, d))
    rng = np.random.default_rng(7)
    h, w = TILE_H + 1, TILE_W + 1                            # one pixel past the tile in each direction
    d = (1.0 + 0.002 * np.arange(w, dtype=np.float32)[None, None, :] + 0.2 * (rng.random((3, h, w)) < 0.2)).astype(np.float32)
    d[rng.random((3, h, w)) < 0.02] = np.nan
    d[:, TILE_H - 1:, TILE_W - 2:] += np.float32(0.5)        # a step across the tile corner
    out.append((f"tile_{h}x{w}", d))
    return out


SCENES = _scenes()
LOGIT = host.conf_logit_threshold(0.6)
SETTINGS = [(True, None, None, None), (False, LOGIT, None, None), (False, None, 0.05, None), (False, None, None, 0.03),
            (True, LOGIT, 0.05, 0.03), (False, None, 0.0, 0.0), (True, None, None, 0.03)]


@pytest.mark.parametrize("name,depth", SCENES, ids=[n for n, _ in SCENES])
def test_mask_equals_the_restated_rule_bit_for_bit(name, depth):
    s = scene(name, depth)
    dropped = 0
    for finite, logit, atol, rtol in SETTINGS:
        want = want_mask(s, finite, logit, atol, rtol)
        got = got_mask(s, finite, logit, atol, rtol)
        assert got.shape == want.shape and np.array_equal(got, want), (name, finite, logit, atol, rtol, int((got != want).sum()))
        dropped += int((~want).sum())
    assert dropped > 0 or depth.size <= 3


@pytest.mark.parametrize("name,depth", [c for c in SCENES if c[0].startswith("d_")], ids=[n for n, _ in SCENES if n.startswith("d_")])
def test_mask_edge_bits_equal_the_reference_fixture(name, depth):
    """the kernel against the REFERENCE's own depth_edge output (tests/golden/depth_edge_cases), every (atol, rtol) pair"""
    from safetensors.numpy import load_file
    g = load_file(cloud_check.GOLDEN + ".safetensors")
    local = np.zeros(depth.shape + (3,), dtype=np.float32)
    local[..., 2] = g[name]
    for i, (atol, rtol) in enumerate(cloud_check.EDGE_TOLS):
        got = hip.cloud_mask(None, dev(local), None, 0.0, atol, rtol, finite=False).cpu().numpy().astype(bool)
        want = ((g["e" + name[1:]] >> i) & 1) == 0
        assert np.array_equal(got, want), (name, atol, rtol)


def test_mask_confidence_at_the_threshold_and_its_neighbours():
    thr = np.float32(host.conf_logit_threshold(0.7))
    vals = np.array([thr, np.nextafter(thr, np.float32(np.inf)), np.nextafter(thr, np.float32(-np.inf)), np.nan, np.inf, -np.inf,
                     0.0, -thr], dtype=np.float32)
    conf = np.resize(vals, (3, 5, 11)).astype(np.float32)
    got = hip.cloud_mask(None, None, dev(conf), float(thr), None, None, finite=False).cpu().numpy().astype(bool)
    want = cloud_check.keep_mask(conf=conf, conf_logit_min=float(thr), finite=False)
    assert np.array_equal(got, want)
    assert want.reshape(-1)[:8].tolist() == [False, True, False, False, True, False, False, False]


def test_mask_relative_edge_within_one_ulp_of_rtol():
    """Per view a plane with one step, a | b, the step placed so that q = (b - a) / a or (b - a) / b lands on rtol or one fp32 ulp
    either side of it.  Kept: the views where fp64 and correctly rounded fp32 put q on the same side of rtol."""
    rtol = np.float32(0.03)
    rng = np.random.default_rng(11)
    views, sides = [], []
    for _ in range(20000):
        a = np.float32(rng.uniform(1.0, 3.0))
        b = np.float32(a * (np.float32(1) + rtol))
        for _k in range(int(rng.integers(0, 4))):
            b = np.nextafter(b, np.float32(np.inf) if rng.random() < 0.5 else np.float32(-np.inf))
        diff = np.float32(b + np.float32(-a))
        for centre in (a, b):
            q32 = np.float32(diff / centre)
            near = abs(int(q32.view(np.int32)) - int(rtol.view(np.int32))) <= 1
            side64 = float(diff) / float(centre) > float(rtol)
            if near and side64 == bool(q32 > rtol):
                views.append((a, b))
                sides.append((int(q32.view(np.int32)) - int(rtol.view(np.int32)), bool(q32 > rtol), centre == a))
                break
        if len(views) == 96:
            break
    assert len(views) == 96 and {s[0] for s in sides} == {-1, 0, 1}
    d = np.empty((len(views), 5, 6), dtype=np.float32)
    for n, (a, b) in enumerate(views):
        d[n, :, :3], d[n, :, 3:] = a, b
    local = np.zeros(d.shape + (3,), dtype=np.float32)
    local[..., 2] = d
    got = hip.cloud_mask(None, dev(local), None, 0.0, None, float(rtol), finite=False).cpu().numpy().astype(bool)
    want = ~cloud_check.edge_mask(d, None, float(rtol))
    assert np.array_equal(got, want)
    for n, (_, edge, at_a) in enumerate(sides):               # the restated rule itself sits on the fp64 side
        assert want[n, 2, 2 if at_a else 3] == (not edge)
    assert want[:, :, 0].all() and want[:, :, 5].all() and 0 < (~want).sum()


# ------------------------------------------------------------------------------------------------ compaction
def _colours(rng, shape):
    special = np.concatenate([np.arange(256, dtype=np.float32) / np.float32(255), np.arange(256, dtype=np.float64).astype(np.float32) / 255,
                              np.array([0.0, 1.0, -0.0, -1e-3, 1.0 + 1e-6, 1.5, -3.0, 1e-40, -1e-40, 1.4e-45, np.nextafter(np.float32(1), np.float32(0)),
                                        np.nextafter(np.float32(1), np.float32(2))], dtype=np.float32)]).astype(np.float32)
    c = rng.random(shape).astype(np.float32)
    flat = c.reshape(-1)
    idx = rng.permutation(flat.size)[:min(flat.size, 4 * special.size)]
    flat[idx] = np.resize(special, idx.size)
    if flat.size < special.size:                              # tiny views: take the specials in turn
        flat[:] = special[rng.integers(0, special.size, flat.size)]
    return c


COMPACT_SHAPES = [(1, 1, 1), (1, 11, 93), (1, 32, 32), (1, 25, 41), (3, 37, 70), (2, 518, 518)]   # 1, 1023, 1024, 1025 pixels, ...
_COMPACT_SCENES = {}


def compact_scene(shape):
    if shape not in _COMPACT_SCENES:
        rng = np.random.default_rng(shape[0] * 1000003 + shape[1] * 1009 + shape[2])
        n, h, w = shape
        points = rng.standard_normal((n, h, w, 3)).astype(np.float32)
        points.reshape(-1)[rng.permutation(points.size)[:max(points.size // 50, 1)]] = np.nan       # records keep whatever the mask keeps
        colors = _colours(rng, (n, 3, h, w))
        _COMPACT_SCENES[shape] = (points, colors, dev(points), dev(colors), rng.random((n, h, w)) < 0.5)
    return _COMPACT_SCENES[shape]


@pytest.mark.parametrize("kind", ["all", "none", "first", "last", "random", "view_empty"])
@pytest.mark.parametrize("shape", COMPACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_compaction_is_stable_and_byte_equal(shape, kind):
    points, colors, dpoints, dcolors, rnd = compact_scene(shape)
    mask = np.zeros(shape, dtype=bool)
    if kind == "all":
        mask[:] = True
    elif kind == "first":
        mask.reshape(-1)[0] = True
    elif kind == "last":
        mask.reshape(-1)[-1] = True
    elif kind == "random":
        mask = rnd.copy()
    elif kind == "view_empty":
        mask = rnd.copy()
        mask[shape[0] // 2] = False
    want, want_counts = cloud_check.pack_records(points, colors, mask)
    rec, counts = hip.cloud_compact(dpoints, dcolors, dev(mask))
    assert rec.dtype == torch.uint8 and tuple(rec.shape) == want.shape and counts.dtype == torch.int32
    assert counts.cpu().tolist() == want_counts.tolist()
    assert np.array_equal(rec.cpu().numpy(), want)
    rec2, counts2 = hip.cloud_compact(dpoints, dcolors, dev(mask.astype(np.uint8) * 255))   # any non-zero byte keeps; a second launch
    assert torch.equal(rec2, rec) and torch.equal(counts2, counts)


def test_compaction_respects_the_record_capacity():
    """records past max_records are not written, counts stay true (the C entry point; hip.cloud_compact always passes N H W)"""
    shape = (3, 37, 70)
    points, colors, dpoints, dcolors, rnd = compact_scene(shape)
    want, want_counts = cloud_check.pack_records(points, colors, rnd)
    cap = want.shape[0] // 2 + 1
    rec = torch.full((cap + 64, 15), 0xA5, dtype=torch.uint8, device=DEV)
    counts = torch.empty(3, dtype=torch.int32, device=DEV)
    ws = torch.empty(hip.cloud_compact_workspace(*shape), dtype=torch.uint8, device=DEV)
    rc = hip.lib().g2v_cloud_compact(hip._p(dpoints), hip._p(dcolors), hip._p(dev(rnd)), *shape, hip._p(rec), cap, hip._p(counts), hip._p(ws),
                                     ws.numel(), hip._stream())
    assert rc == 0 and counts.cpu().tolist() == want_counts.tolist()
    out = rec.cpu().numpy()
    assert np.array_equal(out[:cap], want[:cap]) and (out[cap:] == 0xA5).all()


# ------------------------------------------------------------------------------------------------ intrinsics
INTR_SHAPES = [(3, 37, 70), (1, 518, 518)]


def pinhole(shape, rng, noise=0.0):
    """local points of an exact pinhole camera per view (fx != fy, principal point off centre, random positive depth), fp32"""
    n, h, w = shape
    K = np.zeros((n, 3, 3))
    local = np.empty((n, h, w, 3), dtype=np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    for i in range(n):
        fx, fy = 0.9 * max(h, w) * (1 + 0.1 * i), 0.8 * max(h, w) * (1 + 0.07 * i)
        cx, cy = w / 2 + 0.031 * w + i, h / 2 - 0.043 * h - 0.5 * i
        K[i] = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
        z = rng.uniform(0.5, 5.0, (h, w))
        a = (xx + 0.5 - cx) / fx + noise * rng.standard_normal((h, w))
        b = (yy + 0.5 - cy) / fy + noise * rng.standard_normal((h, w))
        local[i] = np.stack([a * z, b * z, z], -1).astype(np.float32)
    return local, K


def ulps(got, want, scale):
    """|got - fp32(want)| in fp32 ulps of `scale`"""
    return np.abs(got.astype(np.float64) - want) / np.spacing(np.float32(scale)).astype(np.float64)


def check_K(K, ref, h, w, bound=4.0):
    assert K.dtype == np.float32 and K.shape == ref.shape
    assert np.array_equal(np.isnan(K), np.isnan(ref)), (K, ref)
    for r, c in ((0, 1), (1, 0), (2, 0), (2, 1)):
        assert (K[:, r, c] == 0).all()
    assert (K[:, 2, 2] == 1).all()
    ok = ~np.isnan(ref)
    worst = 0.0
    for (r, c), scale in (((0, 0), None), ((1, 1), None), ((0, 2), max(w, h)), ((1, 2), max(w, h))):
        sel = ok[:, r, c]
        if sel.any():
            u = ulps(K[sel, r, c], ref[sel, r, c], np.abs(ref[sel, r, c]) if scale is None else scale)
            worst = max(worst, float(u.max()))
    assert worst <= bound, worst
    return worst


@pytest.mark.parametrize("shape", INTR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_intrinsics_recover_an_exact_pinhole(shape):
    local, K_true = pinhole(shape, np.random.default_rng(3))
    K, used = hip.intrinsics_lsq(dev(local))
    K = K.cpu().numpy()
    assert used.cpu().tolist() == [shape[1] * shape[2]] * shape[0]
    for r, c in ((0, 0), (1, 1), (0, 2), (1, 2)):
        assert np.allclose(K[:, r, c], K_true[:, r, c], rtol=1e-5, atol=0), (r, c, K[:, r, c], K_true[:, r, c])
    K2, used2 = hip.intrinsics_lsq(dev(local))
    assert torch.equal(K2.cpu().view(torch.int32), torch.from_numpy(K).view(torch.int32)) and torch.equal(used2, used)


@pytest.mark.parametrize("shape", INTR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_intrinsics_equal_fp64_lstsq_on_a_noisy_scene(shape):
    """Bound: 4 fp32 ulps on fx, fy and 4 ulps of max(W, H) on cx, cy - fp64 accumulation over <= 2^24 terms errs by about 1e-9
    times the fit's condition number, far below one fp32 ulp for these well-spread ratios; the final rounding adds half an ulp."""
    rng = np.random.default_rng(5)
    local, _ = pinhole(shape, rng, noise=0.01)
    bad = rng.random(shape) < 0.1                             # pixels the fit must leave out
    local[..., 2][bad & (rng.random(shape) < 0.5)] *= -1
    local[..., 2][bad & (rng.random(shape) < 0.2)] = 0.0
    local[..., 0][bad & (rng.random(shape) < 0.2)] = np.nan
    local[..., 1][bad & (rng.random(shape) < 0.2)] = np.inf
    mask = rng.random(shape) < 0.7
    for m in (None, mask):
        ref, ref_used = cloud_check.fit_intrinsics(local, m)
        K, used = hip.intrinsics_lsq(dev(local), None if m is None else dev(m))
        assert used.cpu().tolist() == ref_used.tolist() and 0 < ref_used.min() < shape[1] * shape[2]
        worst = check_K(K.cpu().numpy(), ref, shape[1], shape[2])
        print(f"intrinsics {shape} mask={'yes' if m is not None else 'no'}: worst {worst:.3f} ulp")
        K2, _ = hip.intrinsics_lsq(dev(local), None if m is None else dev(m.astype(np.uint8)))
        assert torch.equal(K2.view(torch.int32), K.view(torch.int32))
    all_ref, _ = cloud_check.fit_intrinsics(local, None)
    assert not np.array_equal(all_ref, ref)                  # the mask did restrict the fit


def test_intrinsics_degenerate_views_give_nan():
    shape = (4, 9, 13)
    local, _ = pinhole(shape, np.random.default_rng(9))
    mask = np.ones(shape, dtype=bool)
    mask[0] = False
    mask[0, 4, 6] = True                                     # one usable pixel: nothing is determined
    local[1, ..., 0] = 0.0                                   # X/Z does not vary: fx, cx undetermined, fy, cy fine
    local[2, ..., 2] *= -1                                   # nothing in front of the camera
    ref, ref_used = cloud_check.fit_intrinsics(local, mask)
    assert np.isnan(ref[0, :2]).sum() == 4 and np.isnan(ref[1]).sum() == 2 and np.isnan(ref[2]).sum() == 4 and not np.isnan(ref[3]).any()
    K, used = hip.intrinsics_lsq(dev(local), dev(mask))
    assert used.cpu().tolist() == ref_used.tolist() == [1, 117, 0, 117]
    check_K(K.cpu().numpy(), ref, 9, 13)
