"""CPU (no GPU): voxel-grid downsampling of the exported cloud (csrc/voxel.hip, g2vlm_utils.voxel_downsample /
save_point_cloud(voxel_size=)), in the style of tests/test_cloud_cpu.py.

1. The C ABI: the entry points and the workspace queries are exported, declared and bound; every argument error comes back as
   -22 before anything touches a device; the workspace sizes, as formulas.
2. The rule of tests/voxel_check.py - what the kernels are held to byte for byte on the GPU - against an independent brute-force
   fp64 mean, and its edge cases: floor at negative coordinates, points on cell faces, first-appearance order, rounding half up.
3. The public functions refuse bad arguments before any launch; the inference_recon flags."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import voxel_check  # noqa: E402
from g2vlm_amd import hip  # noqa: E402

ENTRY = ("g2v_voxel_assign", "g2v_voxel_reduce", "g2v_voxel_bounds")
QUERY = ("g2v_voxel_assign_workspace", "g2v_voxel_reduce_workspace")
ASSIGN_NAMES = ("points", "mask", "N", "H", "W", "voxel_size", "origin_x", "origin_y", "origin_z", "voxel_of", "stats", "workspace",
                "workspace_bytes", "stream")
REDUCE_NAMES = ("points", "colors", "voxel_of", "N", "H", "W", "voxel_size", "origin_x", "origin_y", "origin_z", "M", "records", "counts",
                "out_points", "out_colors", "workspace", "workspace_bytes", "flags", "stream")
BOUNDS_NAMES = ("points", "mask", "N", "H", "W", "bounds", "stream")


# ------------------------------------------------------------------------------------------------ 1. the C ABI
@pytest.fixture(scope="module")
def lib():
    from g2vlm_amd import build
    lib = C.CDLL(build.build())
    for name in ENTRY + QUERY:
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = hip._SIGS[name]
    return lib


def test_library_exports_and_declares_the_entry_points(lib):
    from g2vlm_amd import build
    hdr = open(os.path.join(ROOT, "include", "g2vlm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, names in zip(ENTRY, (ASSIGN_NAMES, REDUCE_NAMES, BOUNDS_NAMES)):
        assert hasattr(lib, name) and name in hip.EXPORTS
        decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(decl.split(",")) == len(hip._SIGS[name][0]) == len(names), name
        assert [d.split()[-1].lstrip("*") for d in decl.split(",")] == list(names)
        assert name in doc
    for name, nargs in zip(QUERY, (3, 1)):
        assert hasattr(lib, name) and name in hip.EXPORTS and name in doc
        decl = re.search(r"\bint64_t %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(decl.split(",")) == len(hip._SIGS[name][0]) == nargs and hip._SIGS[name][1] is C.c_int64
    assert "voxel.hip" in build.SOURCES and "voxel.hip" not in build.RESOURCE_AUDIT
    assert re.search(r"#define G2V_VOXEL_NO_RUNS 1\b", hdr) and hip.VOXEL_NO_RUNS == 1
    assert lib.g2v_version() == 1


def call_assign(lib, **kw):
    """A valid argument set (no pointer is dereferenced: every call below is refused before any launch), with overrides."""
    a = dict(points=16, mask=16, N=3, H=37, W=70, voxel_size=0.25, origin_x=0.0, origin_y=-1.0, origin_z=2.0, voxel_of=16, stats=16,
             workspace=16, workspace_bytes=1 << 30, stream=None)
    a.update(kw)
    return lib.g2v_voxel_assign(*[a[k] for k in ASSIGN_NAMES])


def call_reduce(lib, **kw):
    a = dict(points=16, colors=16, voxel_of=16, N=3, H=37, W=70, voxel_size=0.25, origin_x=0.0, origin_y=-1.0, origin_z=2.0, M=100,
             records=16, counts=16, out_points=None, out_colors=None, workspace=16, workspace_bytes=1 << 30, flags=0, stream=None)
    a.update(kw)
    return lib.g2v_voxel_reduce(*[a[k] for k in REDUCE_NAMES])


def call_bounds(lib, **kw):
    a = dict(points=16, mask=16, N=3, H=37, W=70, bounds=16, stream=None)
    a.update(kw)
    return lib.g2v_voxel_bounds(*[a[k] for k in BOUNDS_NAMES])


INF, NAN = float("inf"), float("nan")
SHAPES_BAD = [dict(N=0), dict(N=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-1), dict(N=4, H=32768, W=32768),
              dict(N=1, H=46341, W=46341), dict(N=2, H=2 ** 15, W=2 ** 15)]
GRID_BAD = [dict(voxel_size=0.0), dict(voxel_size=-0.25), dict(voxel_size=NAN), dict(voxel_size=INF), dict(origin_x=NAN),
            dict(origin_y=INF), dict(origin_z=-INF)]
ASSIGN_WS = 12 * 16384 + 5 * 7770 + 8 * 8                   # 3 x 37 x 70 = 7 770 pixels: 16 384 slots, 8 blocks of 1 024


@pytest.mark.parametrize("bad", SHAPES_BAD + GRID_BAD + [dict(points=None), dict(mask=None), dict(voxel_of=None), dict(stats=None),
                                                         dict(workspace=None), dict(workspace_bytes=0),
                                                         dict(workspace_bytes=ASSIGN_WS - 1), dict(workspace=20), dict(points=18)])
def test_assign_argument_errors_return_einval_without_a_device(lib, bad):
    assert call_assign(lib, **bad) == -22


@pytest.mark.parametrize("bad", SHAPES_BAD + GRID_BAD + [dict(points=None), dict(colors=None), dict(voxel_of=None), dict(records=None),
                                                         dict(counts=None), dict(workspace=None), dict(workspace_bytes=0),
                                                         dict(workspace_bytes=64 * 100 - 1), dict(M=-1), dict(M=7771), dict(flags=2),
                                                         dict(M=0, points=None), dict(M=0, voxel_size=0.0), dict(workspace=20)])
def test_reduce_argument_errors_return_einval_without_a_device(lib, bad):
    assert call_reduce(lib, **bad) == -22


def test_reduce_of_no_voxels_is_a_valid_no_op(lib):
    assert call_reduce(lib, M=0, records=None, counts=None, workspace=None, workspace_bytes=0) == 0


@pytest.mark.parametrize("bad", SHAPES_BAD + [dict(points=None), dict(mask=None), dict(bounds=None), dict(points=18)])
def test_bounds_argument_errors_return_einval_without_a_device(lib, bad):
    assert call_bounds(lib, **bad) == -22


def test_the_workspace_queries(lib):
    aw, rw = lib.g2v_voxel_assign_workspace, lib.g2v_voxel_reduce_workspace
    for bad in ((0, 5, 5), (3, 0, 5), (3, 5, -1), (4, 32768, 32768)):
        assert aw(*bad) == 0
    assert rw(-1) == 0 and rw(0) == 0 and rw(2 ** 31) == 0

    def assign_bytes(p):
        # P pixels: a table of S slots, S the power of two >= 2 P (a u64 key and an i32 first index each), a u32 slot and a
        # flag byte per pixel, two i32 per block of 1 024 pixels
        s = 2
        while s < 2 * p:
            s *= 2
        return 12 * s + 5 * p + 8 * ((p + 1023) // 1024)
    for shape in ((1, 1, 1), (3, 37, 70), (1, 32, 32), (1, 32, 33), (1, 17, 129), (2, 518, 518), (32, 518, 518)):
        assert aw(*shape) == assign_bytes(shape[0] * shape[1] * shape[2]), shape
    assert aw(3, 37, 70) == ASSIGN_WS and aw(1, 1, 1) == 24 + 5 + 8 and aw(1, 32, 32) == 12 * 2048 + 5 * 1024 + 8
    # eight u64 per cell: n, three fraction sums, three colour sums, the key
    assert rw(1) == 64 and rw(100) == 6400 and rw(2 ** 31 - 1) == 64 * (2 ** 31 - 1)
    assert (2 * 518 * 518 + 1023) // 1024 > 2 * 256           # the GPU test's 2 x 518 x 518: three passes of the block scan


# ------------------------------------------------------------------------------------------------ 2. the rule
def ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def scene(seed, centre, scale, n=2, h=9, w=13):
    rng = np.random.default_rng(seed)
    pts = (np.asarray(centre) + rng.standard_normal((n, h, w, 3)) * scale).astype(np.float32)
    col = (rng.random((n, 3, h, w)) * 1.2 - 0.1).astype(np.float32)
    mask = rng.random((n, h, w)) < 0.8
    return pts, col, mask


@pytest.mark.parametrize("v,origin", [(0.75, (0.0, 0.0, 0.0)), (0.3, (-10.5, 0.1, 7.0)), (2.0 ** -3, (1e-3, -1e-3, 0.0)), (5.0, (100.0, -100.0, 3.0))])
def test_restatement_against_the_brute_force_mean(v, origin):
    pts, col, mask = scene(int(v * 1000), origin, 2 * v)     # some two hundred points over a few cells each way: shared cells
    pts[0, 0, 0] = np.nan
    pts[1, 2, 3, 1] = np.inf
    mask[0, 0, 0] = mask[1, 2, 3] = True
    out = voxel_check.downsample(pts, col, mask, v, origin)
    brute = voxel_check.brute_means(pts, col, mask, v, origin)
    assert len(brute) == out["stats"][0] == len(out["records"]) > 20
    assert out["stats"][1] == sum(n for _, _, n in brute.values()) == int(voxel_check.participating(pts, mask).sum())
    assert out["voxel_of"][0, 0, 0] == -1 and out["voxel_of"][1, 2, 3] == -1 and (out["voxel_of"][~mask] == -1).all()
    assert max(n for _, _, n in brute.values()) > 1
    for i, (cell, (mean, cmean, n)) in enumerate(brute.items()):            # the same cells in the same (first-appearance) order
        x = out["points"][i]
        assert out["counts"][i] == n
        # v 2^-25 from the 24-bit fractions and half an ulp of the fp32 rounding, each with a factor of two of room
        assert (np.abs(x.astype(np.float64) - mean) <= v * 2.0 ** -24 + ulp32(x)).all(), (cell, x, mean)
        lo = np.asarray(origin) + np.asarray(cell) * v
        assert (x >= (lo - ulp32(lo)).astype(np.float32)).all() and (x <= (lo + v + ulp32(lo + v)).astype(np.float32)).all()
        # cmean = C / n exactly representable sums: floor(mean + 0.5) in integers
        C = np.rint(cmean * n).astype(np.int64)
        assert (out["colors"][i] == (2 * C + n) // (2 * n)).all() and (out["colors"][i] == np.floor(C / n + 0.5)).all()
    assert np.array_equal(out["records"][:, :12].copy().view("<f4"), out["points"]) and np.array_equal(out["records"][:, 12:], out["colors"])


def one_row(xs, col=None):
    xs = np.asarray(xs, dtype=np.float32)
    pts = np.zeros((1, 1, len(xs), 3), dtype=np.float32)
    pts[0, 0, :, 0] = xs
    colors = np.zeros((1, 3, 1, len(xs)), dtype=np.float32) if col is None else np.asarray(col, dtype=np.float32).reshape(1, 3, 1, len(xs))
    return pts, colors, np.ones((1, 1, len(xs)), dtype=np.uint8)


def test_floor_not_truncation_at_negative_coordinates():
    pts, col, mask = one_row([-0.25, 0.25, -0.75, -1.0, -0.0, 0.0])
    out = voxel_check.downsample(pts, col, mask, 1.0, (0.0, 0.0, 0.0))
    assert out["voxel_of"].reshape(-1).tolist() == [0, 1, 0, 0, 1, 1]     # -0.25, -0.75 and -1.0 share cell -1; -0.0 is in cell 0
    assert out["counts"].tolist() == [3, 3]
    assert out["points"][:, 0].tolist() == [np.float32(-2.0 / 3.0), np.float32(0.25 / 3.0)]


@pytest.mark.parametrize("v,o", [(0.25, 0.0), (0.375, -1.5), (3.0, 0.25), (2.0 ** -10, 0.5)])
def test_a_point_on_a_face_goes_up_and_its_neighbours_to_their_sides(v, o):
    faces = []
    for k in (-7, -1, 0, 1, 5, 1000):
        x = np.float32(o + k * v)
        if float(x) == o + k * v and np.floor((float(x) - o) / v) == k:   # the face is an fp32 number and the division finds it
            faces.append((k, x))
    assert len(faces) == 6
    for k, x in faces:
        below, above = np.nextafter(x, np.float32(-np.inf)), np.nextafter(x, np.float32(np.inf))
        pts, col, mask = one_row([below, x, above])
        g, _, _, ok = voxel_check.cells(pts.reshape(-1, 3), v, (o, 0.0, 0.0))
        assert ok.all() and g[:, 0].tolist() == [k - 1, k, k], (k, x)
        out = voxel_check.downsample(pts, col, mask, v, (o, 0.0, 0.0))
        assert out["voxel_of"].reshape(-1).tolist() == [0, 1, 1] and out["counts"].tolist() == [1, 2]


def test_first_appearance_order_and_min_points():
    # cells 5, 2, 5, 9, 2, 2 along x: order 5, 2, 9 with 2, 3, 1 points
    pts, col, mask = one_row([5.5, 2.5, 5.25, 9.5, 2.25, 2.75])
    out = voxel_check.downsample(pts, col, mask, 1.0, (0.0, 0.0, 0.0))
    assert out["voxel_of"].reshape(-1).tolist() == [0, 1, 0, 2, 1, 1] and out["counts"].tolist() == [2, 3, 1]
    assert out["points"][:, 0].tolist() == [5.375, 2.5, 9.5] and out["stats"] == [3, 6, 0, 0]
    two = voxel_check.downsample(pts, col, mask, 1.0, (0.0, 0.0, 0.0), min_points=2)
    assert two["counts"].tolist() == [2, 3] and two["points"][:, 0].tolist() == [5.375, 2.5] and two["kept"].tolist() == [True, True, False]
    assert two["stats"] == [3, 6, 0, 0] and np.array_equal(two["voxel_of"], out["voxel_of"])
    three = voxel_check.downsample(pts, col, mask, 1.0, (0.0, 0.0, 0.0), min_points=3)
    assert three["counts"].tolist() == [3] and three["points"][:, 0].tolist() == [2.5]
    mask[0, 0, 0] = 0                                        # without its first pixel, cell 5 comes after cell 2
    out = voxel_check.downsample(pts, col, mask, 1.0, (0.0, 0.0, 0.0))
    assert out["voxel_of"].reshape(-1).tolist() == [-1, 0, 1, 2, 0, 0]


def test_colour_means_round_half_up_and_out_of_range_points_are_counted():
    b = lambda k: (k + 0.5) / 255.0                          # noqa: E731  (a colour whose byte is k)
    col = np.array([[b(10), b(11), 0.0], [b(0), b(1), 2.0], [b(255), b(254), -1.0]])       # r: 10.5 -> 11, g: 0.5 -> 1, b: 254.5 -> 255
    pts, colors, mask = one_row([0.25, 0.75, 1e9], col)
    assert voxel_check.colour_bytes(colors.transpose(0, 2, 3, 1))[0, 0].tolist() == [[10, 0, 255], [11, 1, 254], [0, 255, 0]]
    out = voxel_check.downsample(pts, colors, mask, 1.0, (0.0, 0.0, 0.0))
    assert out["stats"] == [1, 2, 1, 0] and out["colors"].tolist() == [[11, 1, 255]] and out["voxel_of"].reshape(-1).tolist() == [0, 0, -1]
    assert out["points"][0].tolist() == [0.5, 0.0, 0.0]


def test_a_singleton_voxel_returns_its_point_and_the_default_origin():
    rng = np.random.default_rng(5)
    v = 2.0 ** -10
    # one point per cell: a lattice of spacing 2 v plus jitter inside the cell, coordinates in [-4, 4]: v 2^-24 < ulp32 / 4
    idx = rng.permutation(4096)[:600]
    lattice = np.stack([idx % 16, (idx // 16) % 16, idx // 256], 1) * 2 - 15
    pts = ((lattice + rng.random((600, 3)) * 0.9) * v * 128).astype(np.float32).reshape(2, 10, 30, 3)
    col, mask = rng.random((2, 3, 10, 30)).astype(np.float32), np.ones((2, 10, 30), dtype=np.uint8)
    origin = voxel_check.default_origin(pts, mask, v)
    assert np.array_equal(origin, pts.reshape(-1, 3).astype(np.float64).min(0) - v / 2)
    out = voxel_check.downsample(pts, col, mask, v, origin)
    assert out["stats"][0] == 600 and (out["counts"] == 1).all()
    assert np.array_equal(out["points"].view(np.uint32), pts.reshape(-1, 3).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. the public surface
def test_public_functions_refuse_bad_arguments_before_any_launch(monkeypatch):
    import torch
    import g2vlm_utils as top
    from g2vlm_amd import g2vlm_utils as gu
    assert top.voxel_downsample is gu.voxel_downsample and "voxel_downsample" in top.__all__
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("a refused call reached the library"))
    pred = dict(points=torch.zeros(1, 2, 4, 6, 3), local_points=torch.ones(1, 2, 4, 6, 3), conf=None, images=torch.zeros(1, 2, 3, 4, 6))
    for fn in (lambda **kw: gu.voxel_downsample(pred, **kw), lambda **kw: gu.save_point_cloud(pred, "unused.ply", **{
            dict(origin="voxel_origin").get(k, k): x for k, x in kw.items()})):
        for kw in (dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(voxel_size=float("nan")), dict(voxel_size=float("inf")),
                   dict(voxel_size="wide"), dict(voxel_size=0.1, min_points=0), dict(voxel_size=0.1, min_points=-2),
                   dict(voxel_size=0.1, min_points=1.5), dict(voxel_size=0.1, origin=(0.0, 1.0)),
                   dict(voxel_size=0.1, origin=(0.0, float("nan"), 0.0)), dict(voxel_size=0.1, conf_threshold=0.5),
                   dict(voxel_size=0.1, edge_rtol=-0.01)):
            with pytest.raises(ValueError):
                fn(**kw)
    for bad in (torch.ones(2, 4, 5, dtype=torch.bool), torch.ones(2, 4, 6), torch.ones(3, 4, 6, dtype=torch.uint8), np.ones((2, 4, 6), bool)):
        with pytest.raises(ValueError, match="mask"):
            gu.voxel_downsample(pred, 0.1, mask=bad)
    with pytest.raises(ValueError, match="images"):
        gu.voxel_downsample(dict(pred, images=torch.zeros(1, 2, 3, 8, 6)), 0.1)
    assert not os.path.exists("unused.ply")


def test_signatures_of_the_public_functions():
    import inspect
    from g2vlm_amd import g2vlm_utils as gu
    assert list(inspect.signature(gu.voxel_downsample).parameters) == ["pred_dict", "voxel_size", "origin", "min_points", "conf_threshold",
                                                                        "edge_rtol", "edge_atol", "filter_nan", "mask"]
    sp = inspect.signature(gu.save_point_cloud).parameters
    assert list(sp)[-4:] == ["verbose", "voxel_size", "voxel_origin", "min_points"]
    assert sp["voxel_size"].default is None and sp["voxel_origin"].default is None and sp["min_points"].default == 1
    assert sp["edge_rtol"].default == 0.03                    # the existing defaults stay


def test_inference_recon_has_the_voxel_flags_off_by_default():
    import inference_recon
    a = inference_recon.parser.parse_args([])
    assert a.voxel_size is None and a.voxel_min_points == 1
    assert a.conf_threshold is None and a.edge_rtol is None and a.edge_atol is None and a.intrinsics is False
    b = inference_recon.parser.parse_args(["--voxel-size", "0.05", "--voxel-min-points", "3"])
    assert (b.voxel_size, b.voxel_min_points) == (0.05, 3)
