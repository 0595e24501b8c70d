"""GPU: the voxel kernels (csrc/voxel.hip) against the numpy restatement of their rule (tests/voxel_check.py), byte for byte:
records, counts, the labels voxel_of and the stats, on every shape and edge case at which the kernels take another path - one
pixel, nothing kept, one cell for everything (contention), one cell per point (the singleton property: cloud_compact's bytes),
cell faces and their fp32 neighbours, negative coordinates, non-finite points under a set mask bit, colour sums on .5,
min_points, more blocks than two passes of the scan, an explicit against the default origin, a point out of range."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import voxel_check  # noqa: E402
from g2vlm_amd import hip  # noqa: E402
from g2vlm_amd.g2vlm_utils import save_point_cloud, voxel_downsample  # noqa: E402

pytestmark = pytest.mark.gpu


def run(pts, col, mask, v, origin, flags=0):
    """assign + reduce on the device; numpy arrays back"""
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    p, c, m = d(pts), d(col), d(np.asarray(mask).astype(np.uint8))
    voxel_of, stats = hip.voxel_assign(p, m, v, origin)
    rec, counts, op, oc = hip.voxel_reduce(p, c, voxel_of, stats[0], v, origin, flags=flags)
    torch.cuda.synchronize()
    return dict(records=rec.cpu().numpy(), counts=counts.cpu().numpy(), points=op.cpu().numpy(), colors=oc.cpu().numpy(),
                voxel_of=voxel_of.cpu().numpy(), stats=stats)


def check(pts, col, mask, v, origin, flags=0):
    """the kernels equal the restatement in every output; returns (got, want)"""
    want = voxel_check.downsample(pts, col, mask, v, origin)
    got = run(pts, col, mask, v, origin, flags)
    print(f"{pts.shape[:3]} v {v}: stats {got['stats']} want {want['stats']}")
    assert got["stats"] == want["stats"]
    assert np.array_equal(got["voxel_of"], want["voxel_of"])
    assert got["records"].shape == want["records"].shape and got["records"].tobytes() == want["records"].tobytes()
    assert np.array_equal(got["counts"], want["counts"]) and got["counts"].dtype == np.int32
    assert np.array_equal(got["points"].view(np.uint32), want["points"].view(np.uint32)) and np.array_equal(got["colors"], want["colors"])
    return got, want


def scene(seed, n, h, w, scale=1.0, keep=0.8):
    rng = np.random.default_rng(seed)
    pts = (rng.standard_normal((n, h, w, 3)) * scale).astype(np.float32)
    col = (rng.random((n, 3, h, w)) * 1.2 - 0.1).astype(np.float32)
    return pts, col, (rng.random((n, h, w)) < keep).astype(np.uint8)


def smooth_scene(seed, n, h, w):
    """what recon gives: surfaces - neighbouring pixels of a row mostly share a cell - seen again from every view"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    pts = np.empty((n, h, w, 3), dtype=np.float32)
    for i in range(n):
        pts[i, ..., 0] = xx / w * 4 - 2 + 0.1 * i
        pts[i, ..., 1] = yy / h * 4 - 2
        pts[i, ..., 2] = 2 + np.sin(xx / 40 + i) * np.cos(yy / 50)
    pts += (rng.standard_normal(pts.shape) * 1e-3).astype(np.float32)
    col = rng.random((n, 3, h, w)).astype(np.float32)
    return pts, col, (rng.random((n, h, w)) < 0.9).astype(np.uint8)


def test_one_pixel():
    pts, col = np.array([[[[0.3, -0.2, 7.0]]]], dtype=np.float32), np.array([0.2, 0.5, 1.5], dtype=np.float32).reshape(1, 3, 1, 1)
    got, _ = check(pts, col, np.ones((1, 1, 1)), 0.25, (0.0, 0.0, 0.0))
    assert got["stats"] == [1, 1, 0, 0] and got["colors"].tolist() == [[51, 127, 255]]


def test_everything_masked_out_is_an_empty_valid_result():
    pts, col, _ = scene(1, 2, 9, 13)
    pts[1, 3, 4] = np.nan
    got, _ = check(pts, col, np.zeros((2, 9, 13)), 0.5, (0.0, 0.0, 0.0))
    assert got["stats"] == [0, 0, 0, 0] and got["records"].shape == (0, 15) and (got["voxel_of"] == -1).all()
    mask = np.zeros((2, 9, 13))
    mask[1, 3, 4] = 1                                        # the only set bit is on a NaN
    got, _ = check(pts, col, mask, 0.5, (0.0, 0.0, 0.0))
    assert got["stats"] == [0, 0, 0, 0]


@pytest.mark.parametrize("flags", [0, hip.VOXEL_NO_RUNS])
def test_all_points_in_one_voxel(flags):
    pts, col, _ = scene(2, 2, 37, 70, scale=0.01)
    got, _ = check(pts, col, np.ones((2, 37, 70)), 1.0, (-0.5, -0.5, -0.5), flags)
    assert got["stats"] == [1, 5180, 0, 0] and got["counts"].tolist() == [5180]


def test_every_point_in_a_voxel_of_its_own_returns_cloud_compact_bytes():
    """the singleton property: coordinates in [-4, 4] and v = 2^-10, so v 2^-24 = 2^-34 < ulp32(p) / 4 for |p| >= 2^-8"""
    rng = np.random.default_rng(3)
    n, h, w, v = 3, 37, 70, 2.0 ** -10
    idx = rng.permutation(32 ** 3)[:n * h * w]
    lattice = np.stack([idx % 32, (idx // 32) % 32, idx // 1024], 1)                         # a lattice of spacing 2 v plus jitter:
    centre = np.array([1.0, -2.0, 3.0])                                                      # neighbours are > v apart, wherever the origin is
    pts = (centre + (lattice * 2 + 0.1 + rng.random((len(idx), 3)) * 0.85) * v).astype(np.float32).reshape(n, h, w, 3)
    assert np.abs(pts).max() <= 4 and np.abs(pts).min() >= 2.0 ** -8
    col, mask = rng.random((n, 3, h, w)).astype(np.float32), rng.random((n, h, w)) < 0.9
    origin = voxel_check.default_origin(pts, mask, v)
    got, _ = check(pts, col, mask, v, origin)
    assert got["stats"][0] == got["stats"][1] == int(mask.sum()) and (got["counts"] == 1).all()
    rec, _ = hip.cloud_compact(torch.from_numpy(pts).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(mask.astype(np.uint8)).cuda())
    assert got["records"][:, :12].tobytes() == rec[:, :12].cpu().numpy().tobytes()           # the points' own fp32 bits
    assert got["records"].tobytes() == rec.cpu().numpy().tobytes()                           # and (2 c + 1) // 2 = c: the whole record


def test_faces_negative_coordinates_and_signed_zero():
    v, o = 0.375, (-1.5, 0.25, 0.0)
    xs = []
    for k in (-7, -1, 0, 1, 5, 1000):
        x = np.float32(o[0] + k * v)
        xs += [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]
    xs += [-0.0, 0.0, -1e-30, 1e-30, -2.5, -0.375, 0.375]
    xs = np.array(xs, dtype=np.float32)
    pts = np.zeros((1, 3, len(xs), 3), dtype=np.float32)
    pts[0, 0, :, 0] = xs                                     # along x, y and z in turn, the other two axes at +-0
    pts[0, 1, :, 1] = xs + np.float32(0.25 + 1.5)            # the faces of y are those of x moved by the origin's difference
    pts[0, 2, :, 2] = xs
    pts[0, 2, ::2, 0] = -0.0
    col = np.random.default_rng(4).random((1, 3, 3, len(xs))).astype(np.float32)
    got, want = check(pts, col, np.ones((1, 3, len(xs))), v, o)
    g, _, _, _ = voxel_check.cells(pts[0, 0], v, o)
    assert g[:18, 0].tolist() == [k + d for k in (-7, -1, 0, 1, 5, 1000) for d in (-1, 0, 0)]
    assert want["stats"][0] > 20 and (pts < 0).any()


def test_non_finite_points_under_a_set_mask_bit_are_dropped_and_counted():
    pts, col, mask = scene(5, 2, 17, 33, scale=2.0, keep=1.0)
    bad = [(0, 0, 0, 0, np.nan), (0, 5, 7, 1, np.inf), (1, 16, 32, 2, -np.inf), (1, 3, 3, 0, np.nan), (0, 9, 9, 2, np.inf)]
    for n, y, x, a, val in bad:
        pts[n, y, x, a] = val
    got, _ = check(pts, col, mask, 0.5, (0.1, 0.2, 0.3))
    assert got["stats"][1] == 2 * 17 * 33 - len(bad) and got["stats"][2] == 0
    assert all(got["voxel_of"][n, y, x] == -1 for n, y, x, _, _ in bad)


def test_colour_sums_that_land_on_half():
    b = lambda k: np.float32((k + 0.5) / 255.0)              # noqa: E731  (a colour whose byte is k)
    pairs = [(10, 11), (0, 1), (254, 255), (100, 103), (7, 7), (0, 255)]          # sums 21, 1, 509: .5; 203: .5; 14, 255: .0 and .5
    pts = np.zeros((1, len(pairs), 2, 3), dtype=np.float32)
    pts[0, :, :, 0] = np.arange(len(pairs))[:, None] + np.array([0.25, 0.5])
    col = np.zeros((1, 3, len(pairs), 2), dtype=np.float32)
    for i, (lo, hi) in enumerate(pairs):
        col[0, 0, i], col[0, 1, i], col[0, 2, i] = (b(lo), b(hi)), (b(hi), b(lo)), (b(lo), b(lo))
    got, _ = check(pts, col, np.ones((1, len(pairs), 2)), 1.0, (0.0, -0.5, -0.5))
    assert got["colors"][:, 0].tolist() == [11, 1, 255, 102, 7, 128] and got["colors"][:, 2].tolist() == [10, 0, 254, 100, 7, 0]
    assert (got["counts"] == 2).all()


@pytest.fixture(scope="module")
def big():
    """2 x 518 x 518: 525 blocks of 1 024 pixels, three passes of the block scan; some tens of thousands of cells"""
    pts, col, mask = smooth_scene(6, 2, 518, 518)
    pts[1, 100, 200] = np.nan
    v = 0.05
    origin = voxel_check.default_origin(pts, mask, v)
    return pts, col, mask, v, origin, voxel_check.downsample(pts, col, mask, v, origin)


def test_many_blocks_and_two_runs_give_identical_bytes(big):
    pts, col, mask, v, origin, want = big
    assert 20000 < want["stats"][0] < 100000
    got, _ = check(pts, col, mask, v, origin)
    again = run(pts, col, mask, v, origin)
    for k in ("records", "counts", "voxel_of", "points", "colors"):
        assert got[k].tobytes() == again[k].tobytes(), k
    plain = run(pts, col, mask, v, origin, hip.VOXEL_NO_RUNS)  # one atomic per pixel: the same integer sums
    assert plain["records"].tobytes() == got["records"].tobytes() and np.array_equal(plain["counts"], got["counts"])


@pytest.mark.parametrize("shape,v", [((1, 17, 129), 0.3), ((3, 37, 70), 0.4), ((1, 32, 32), 0.2), ((1, 32, 33), 0.2)])
def test_odd_shapes(shape, v):
    pts, col, mask = scene(sum(shape), *shape)
    got, _ = check(pts, col, mask, v, (0.05, -0.05, 0.0))
    assert 1 < got["stats"][0] < got["stats"][1]


def as_pred(pts, col):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    return dict(points=d(pts)[None], local_points=d(pts)[None], images=d(col)[None], conf=None)


@pytest.mark.parametrize("min_points", [1, 2, 3])
def test_public_function_min_points_and_origins(min_points):
    pts, col, mask = scene(7, 2, 17, 33, scale=0.5)
    pts[0, 2, 2] = np.nan
    v = 0.25
    pred = as_pred(pts, col)
    finite = np.isfinite(pts).all(-1)
    # the default origin: the minimum of the participating points minus v / 2, in fp64
    want = voxel_check.downsample(pts, col, finite, v, voxel_check.default_origin(pts, finite, v), min_points)
    out = voxel_downsample(pred, v, min_points=min_points)
    assert out["origin"] == tuple(voxel_check.default_origin(pts, finite, v).tolist()) and out["num_input_points"] == int(finite.sum())
    assert out["points"].is_cuda and out["points"].dtype == torch.float32 and out["colors"].dtype == torch.uint8 and out["counts"].dtype == torch.int32
    assert np.array_equal(out["points"].cpu().numpy().view(np.uint32), want["points"].view(np.uint32))
    assert np.array_equal(out["colors"].cpu().numpy(), want["colors"]) and np.array_equal(out["counts"].cpu().numpy(), want["counts"])
    assert (want["counts"] >= min_points).all() and 0 < len(want["counts"]) and (min_points == 1 or not want["kept"].all())
    # an explicit origin and an explicit mask (which replaces the filters; non-finite points still never take part)
    origin = (0.0, 0.125, -3.0)
    want2 = voxel_check.downsample(pts, col, mask, v, origin, min_points)
    out2 = voxel_downsample(pred, v, origin=origin, min_points=min_points, mask=torch.from_numpy(mask.astype(bool)).cuda())
    assert out2["origin"] == origin and out2["num_input_points"] == int((finite & (mask != 0)).sum())
    assert np.array_equal(out2["points"].cpu().numpy().view(np.uint32), want2["points"].view(np.uint32))
    assert np.array_equal(out2["counts"].cpu().numpy(), want2["counts"])
    assert not np.array_equal(want["points"][:8], want2["points"][:8])                     # the two grids do differ


def test_a_point_out_of_range_is_counted_and_the_public_functions_refuse(tmp_path):
    pts, col, mask = scene(8, 1, 9, 13, keep=1.0)
    pts[0, 4, 5, 1] = 1e9
    got, _ = check(pts, col, mask, 1.0, (0.0, 0.0, 0.0))
    assert got["stats"][1:] == [9 * 13 - 1, 1, 0] and got["voxel_of"][0, 4, 5] == -1
    pred = as_pred(pts, col)
    with pytest.raises(ValueError, match=r"voxel_size 1\.0.*1000000000\.0"):
        voxel_downsample(pred, 1.0, origin=(0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="voxel_size"):
        save_point_cloud(pred, str(tmp_path / "never.ply"), edge_rtol=None, voxel_size=1.0, voxel_origin=(0.0, 0.0, 0.0), verbose=False)
    assert not os.path.exists(tmp_path / "never.ply")
    # the default origin sits at the cloud's minimum: the far point is out of range from there too
    with pytest.raises(ValueError, match="voxel_size"):
        voxel_downsample(pred, 1.0)
    assert len(voxel_downsample(pred, 1024.0)["counts"]) >= 2                                # a cell size that spans it is fine
