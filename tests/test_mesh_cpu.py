"""CPU (no GPU): the triangle-mesh export (csrc/mesh.hip, g2vlm_utils.reconstruct_mesh / save_mesh), in the style of
tests/test_render_cpu.py.

1. The C ABI: the entry point and its workspace query are exported, declared and bound; every argument error comes back as -22
   before anything touches a device.
2. The public functions refuse bad arguments before any launch; the inference_recon flags; host.write_ply_mesh.
3. The rule of tests/mesh_check.py - what the kernel is held to on the GPU: every mask of one quad, orientation, a quad-by-quad
   loop, ties and NaN, the invariants of the vertex numbering, fp32 against fp64."""
import ctypes as C
import inspect
import itertools
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import mesh_check as mc  # noqa: E402
from g2vlm_amd import hip  # noqa: E402

NAMES = ("points", "mask", "N", "H", "W", "flags", "max_edge", "used", "vertex_of", "faces", "face_records", "max_faces", "counts", "workspace",
         "workspace_bytes", "stream")


# ------------------------------------------------------------------------------------------------ 1. the C ABI
@pytest.fixture(scope="module")
def lib():
    from g2vlm_amd import build
    lib = C.CDLL(build.build())
    for name in ("g2v_cloud_mesh", "g2v_cloud_mesh_workspace"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = hip._SIGS[name]
    return lib


def test_library_exports_and_declares_the_entry_points(lib):
    from g2vlm_amd import build
    hdr = open(os.path.join(ROOT, "include", "g2vlm_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    name = "g2v_cloud_mesh"
    assert hasattr(lib, name) and name in hip.EXPORTS and ("`%s`" % name) in integration
    decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, re.S).group(1)
    assert len(decl.split(",")) == len(hip._SIGS[name][0]) == len(NAMES)
    assert [d.split()[-1].lstrip("*") for d in decl.split(",")] == list(NAMES)
    q = name + "_workspace"
    assert hasattr(lib, q) and q in hip.EXPORTS and ("`%s`" % q) in integration
    decl = re.search(r"\bint64_t %s\((.*?)\);" % q, hdr, re.S).group(1)
    assert [d.split()[-1] for d in decl.split(",")] == ["N", "H", "W"] and hip._SIGS[q] == ([C.c_int] * 3, C.c_int64)
    assert "mesh.hip" in build.SOURCES and "mesh.hip" not in build.RESOURCE_AUDIT
    assert re.search(r"#define G2V_MESH_MAX_EDGE 1\b", hdr) and hip.MESH_MAX_EDGE == 1
    assert list(inspect.signature(hip.cloud_mesh).parameters)[:4] == ["points", "colors", "mask", "max_edge"]
    assert inspect.signature(hip.cloud_mesh).parameters["max_edge"].default is None
    for export in ("`reconstruct_mesh`", "`save_mesh`"):
        assert export in integration
    assert lib.g2v_version() == 1


def call(lib, **kw):
    """A valid argument set (no pointer is dereferenced: every call below is refused before any launch), with overrides."""
    a = dict(points=16, mask=17, N=3, H=37, W=70, flags=1, max_edge=0.5, used=17, vertex_of=16, faces=16, face_records=17, max_faces=100,
             counts=16, workspace=16, workspace_bytes=1 << 20, stream=None)
    a.update(kw)
    return lib.g2v_cloud_mesh(*[a[k] for k in NAMES])


WS_3_37_70 = 16 * 3 * 3 + 6 * 3 * 37 * 70                    # four ints per block of 1024 pixels, then 4 + 1 + 1 bytes per pixel
BAD = [dict(N=0), dict(N=-1), dict(H=0), dict(W=-1), dict(N=65536, H=1, W=1), dict(N=4, H=32768, W=32768, workspace_bytes=1 << 62),
       dict(N=1, H=32769, W=32769, workspace_bytes=1 << 62),                                      # 2 (H-1) (W-1) = 2^31 faces
       dict(points=None), dict(counts=None), dict(workspace=None), dict(flags=2), dict(flags=-1), dict(max_edge=-1.0),
       dict(max_edge=float("nan")), dict(max_edge=-0.5, flags=1), dict(max_faces=-1), dict(points=18), dict(vertex_of=18), dict(faces=17),
       dict(counts=18), dict(workspace=18), dict(workspace_bytes=0), dict(workspace_bytes=WS_3_37_70 - 1)]


@pytest.mark.parametrize("bad", BAD)
def test_argument_errors_return_einval_without_a_device(lib, bad):
    assert call(lib, **bad) == -22


def test_the_workspace_query(lib):
    ws = lib.g2v_cloud_mesh_workspace
    for bad in ((0, 5, 5), (3, 0, 5), (3, 5, -1), (4, 32768, 32768), (65536, 1, 1), (1, 32769, 32769), (2, 2 ** 30, 2)):
        assert ws(*bad) == 0                                                                       # 0 for every shape the entry point refuses
    assert ws(1, 1, 1) == 16 + 6 and ws(3, 37, 70) == WS_3_37_70 and ws(1, 32, 32) == 16 + 6 * 1024 and ws(1, 32, 33) == 32 + 6 * 1056
    assert ws(8, 518, 518) == 16 * 8 * 263 + 6 * 8 * 518 * 518
    assert ws(1, 2 ** 31 - 1, 1) == 16 * 2 ** 21 + 6 * (2 ** 31 - 1) and ws(1, 32768, 32768) == 16 * 2 ** 20 + 6 * 2 ** 30
    assert ws(65535, 1, 1) == 22 * 65535


# ------------------------------------------------------------------------------------------------ 2. the public surface
def test_public_functions_refuse_bad_arguments_before_any_launch(monkeypatch, tmp_path):
    import torch
    import g2vlm_utils as top
    from g2vlm_amd import g2vlm_utils as gu
    for name in ("reconstruct_mesh", "save_mesh"):
        assert getattr(top, name) is getattr(gu, name) and name in top.__all__
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("a refused call reached the library"))
    pred = dict(points=torch.zeros(1, 2, 4, 6, 3), local_points=torch.ones(1, 2, 4, 6, 3), conf=None, images=torch.zeros(1, 2, 3, 4, 6),
                camera_poses=torch.eye(4).repeat(1, 2, 1, 1))
    ok_mask = torch.ones(2, 4, 6, dtype=torch.bool)
    out = str(tmp_path / "never.ply")
    for kw in (dict(max_edge=-1.0), dict(max_edge=float("nan")), dict(max_edge="long"), dict(max_edge=True), dict(max_edge=[1.0]),
               dict(edge_rtol=-1.0), dict(edge_atol=-0.5), dict(conf_threshold=0.5), dict(min_views=0), dict(min_views=1.5),
               dict(max_in_front=-1), dict(min_views=1, depth_rtol=-1.0), dict(min_views=1, intrinsics=torch.zeros(3, 3, 3)),
               dict(mask=torch.ones(2, 4, 5, dtype=torch.bool)), dict(mask=torch.ones(2, 4, 6)), dict(mask=np.ones((2, 4, 6), bool)),
               dict(mask=ok_mask, conf_threshold=0.5), dict(mask=ok_mask, edge_rtol=0.05), dict(mask=ok_mask, edge_rtol=None),
               dict(mask=ok_mask, edge_atol=0.1), dict(mask=ok_mask, filter_nan=False), dict(mask=ok_mask, min_views=1),
               dict(mask=ok_mask, max_in_front=0), dict(mask=ok_mask, depth_rtol=0.1), dict(mask=ok_mask, intrinsics=torch.eye(3).repeat(2, 1, 1))):
        with pytest.raises(ValueError):
            gu.reconstruct_mesh(pred, **kw)
        with pytest.raises(ValueError):
            gu.save_mesh(pred, out, **kw)
    for bad in (dict(pred, images=torch.zeros(1, 2, 3, 4, 5)), dict(pred, points=torch.zeros(2, 4, 6, 3)),
                dict(pred, local_points=torch.ones(1, 2, 4, 5, 3))):
        with pytest.raises(ValueError):
            gu.reconstruct_mesh(bad)
        with pytest.raises(ValueError):
            gu.save_mesh(bad, out)
    no_poses = {k: v for k, v in pred.items() if k != "camera_poses"}
    with pytest.raises(ValueError, match="camera_poses"):
        gu.reconstruct_mesh(no_poses, min_views=1)
    assert not os.path.exists(out)


def test_signatures_of_the_public_functions():
    from g2vlm_amd import g2vlm_utils as gu
    filters = ["conf_threshold", "edge_rtol", "edge_atol", "filter_nan", "min_views", "max_in_front", "depth_rtol", "intrinsics", "mask", "max_edge"]
    defaults = [None, 0.03, None, True, None, None, 0.03, None, None, None]
    sr = inspect.signature(gu.reconstruct_mesh).parameters
    assert list(sr) == ["pred_dict"] + filters and [sr[k].default for k in filters] == defaults
    ss = inspect.signature(gu.save_mesh).parameters
    assert list(ss) == ["pred_dict", "save_path"] + filters + ["verbose"] and [ss[k].default for k in filters] == defaults
    assert ss["verbose"].default is True


def test_inference_recon_has_the_mesh_flags_off_by_default():
    import inference_recon
    a = inference_recon.parser.parse_args([])
    assert a.mesh is None and a.mesh_max_edge is None
    b = inference_recon.parser.parse_args(["--mesh", "out.ply", "--mesh-max-edge", "0.25", "--edge-rtol", "0.03", "--min-views", "1"])
    assert (b.mesh, b.mesh_max_edge, b.edge_rtol, b.min_views) == ("out.ply", 0.25, 0.03, 1)
    for flag in ("--mesh", "--mesh-max-edge"):
        assert flag in inference_recon.__doc__
    for bad in (["--mesh-max-edge", "0.5"], ["--mesh", "out.ply", "--mesh-max-edge", "-1"]):
        with pytest.raises(SystemExit):                                                            # refused before the model is loaded
            inference_recon.main(["--image_folder", HERE] + bad)


def test_write_ply_mesh_header_and_bytes(tmp_path):
    import torch
    from g2vlm_amd import host
    rng = np.random.default_rng(5)
    vert = np.zeros(7, mc.VERTEX_DTYPE)
    vert["p"], vert["c"] = rng.standard_normal((7, 3)).astype(np.float32), rng.integers(0, 256, (7, 3))
    face = np.zeros(4, mc.FACE_DTYPE)
    face["n"], face["v"] = 3, rng.integers(0, 7, (4, 3))
    vb, fb = vert.view(np.uint8).reshape(-1, 15), face.view(np.uint8).reshape(-1, 13)
    for n, (v, f) in enumerate(((vb, fb), (torch.from_numpy(vb), torch.from_numpy(fb)), (vb[:0], fb[:0]))):
        path = str(tmp_path / f"m{n}.ply")
        host.write_ply_mesh(path, v, f)
        raw = open(path, "rb").read()
        head, body = raw.split(b"end_header\n", 1)
        nv, nf = len(v), len(f)
        assert head.decode("ascii") == ("ply\nformat binary_little_endian 1.0\n" f"element vertex {nv}\n"
                                        "property float x\nproperty float y\nproperty float z\n"
                                        "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                                        f"element face {nf}\nproperty list uchar int vertex_indices\n")
        assert len(body) == 15 * nv + 13 * nf
        got_v = np.frombuffer(body[:15 * nv], mc.VERTEX_DTYPE)
        got_f = np.frombuffer(body[15 * nv:], mc.FACE_DTYPE)
        assert np.array_equal(got_v, vert[:nv]) and np.array_equal(got_f, face[:nf])
        # the vertex header is write_ply_records' header: the vertex part of the file is that file
        host.write_ply_records(path + ".cloud", v)
        cloud = open(path + ".cloud", "rb").read()
        assert cloud.split(b"end_header\n", 1)[0] + f"element face {nf}\nproperty list uchar int vertex_indices\n".encode() == head
        assert cloud.split(b"end_header\n", 1)[1] == body[:15 * nv]
    for v, f in ((vb[:, :14], fb), (vb, fb[:, :12]), (vb.astype(np.int8), fb), (vb, fb.reshape(-1))):
        with pytest.raises(ValueError):
            host.write_ply_mesh(str(tmp_path / "bad.ply"), v, f)


# ------------------------------------------------------------------------------------------------ 3. the rule
def quad(anti_shorter):
    """one quad on the plane z = 2 whose anti diagonal (p01 - p10) is the shorter or the longer one; [1,2,2,3]"""
    p = np.array([[[0, 0, 2], [1, 0, 2]], [[0, 1, 2], [1, 1, 2]]], np.float32)[None]
    if anti_shorter:
        p[0, 1, 1, :2] = (1.5, 1.5)                                                                # p11 pulled away: the main diagonal grows
    else:
        p[0, 0, 1, 0] = 1.5                                                                        # p01 pulled away: the anti diagonal grows
    return p


CORNER = {"00": 0, "01": 1, "10": 2, "11": 3}                                                      # flat pixel of a corner in a 2 x 2 view
ONE_MISSING = {"11": ("00", "10", "01"), "00": ("01", "10", "11"), "01": ("00", "10", "11"), "10": ("00", "11", "01")}


@pytest.mark.parametrize("anti_shorter", [True, False])
def test_all_sixteen_masks_of_one_quad(anti_shorter):
    p = quad(anti_shorter)
    for bits in itertools.product((0, 1), repeat=4):
        mask = np.array(bits, np.uint8).reshape(1, 2, 2)
        r = mc.rule(p, mask)
        kept = [k for k, v in CORNER.items() if bits[v]]
        if len(kept) == 4:
            want = [("00", "10", "01"), ("01", "10", "11")] if anti_shorter else [("00", "10", "11"), ("00", "11", "01")]
        elif len(kept) == 3:
            want = [ONE_MISSING[(set(CORNER) - set(kept)).pop()]]
        else:
            want = []
        want = np.array([[CORNER[k] for k in tri] for tri in want], np.int64).reshape(-1, 3)
        assert np.array_equal(r["face_pixels"], want), bits
        assert r["counts"].tolist() == [[len(kept) if len(want) else 0, len(want)]]
        assert np.array_equal(r["used"].reshape(-1) != 0, np.array(bits, bool) & (len(want) > 0))
        assert np.array_equal(r["vertex_pixel"][r["faces"]], want)                                  # ids are ranks among the used pixels
        assert (mc.toward_camera(p, r["face_pixels"], (0, 0, 0)) > 0).all()
    assert np.array_equal(mc.rule(p, None)["faces"], mc.rule(p, np.ones((1, 2, 2), np.uint8))["faces"])


def test_every_triangle_faces_the_camera():
    """a fronto-parallel plane under every mask pattern that occurs, and the synthetic scene in camera coordinates and, with each
    view's own camera centre, in world coordinates"""
    H, W = 12, 18
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    plane = np.stack([(xs - 8.2) * 0.1, (ys - 5.7) * 0.13, np.full((H, W), 3.0)], -1).astype(np.float32)[None]
    plane[0, ..., :2] += np.random.default_rng(0).uniform(-0.03, 0.03, (H, W, 2)).astype(np.float32)   # both diagonals occur
    for mask in (None, mc.random_mask((1, H, W), 1, keep=0.8), mc.random_mask((1, H, W), 2, keep=0.6)):
        r = mc.rule(plane, mask)
        assert len(r["faces"]) > 10 and (mc.toward_camera(plane, r["face_pixels"], (0, 0, 0)) > 0).all()
        assert {1 | 2, 4 | 8} <= set(r["code"].reshape(-1).tolist())
    s = mc.scene(4, 37, 70)
    hw = 37 * 70
    mask = mc.depth_edge_mask(s["local"])
    for m in (mask, mask & mc.random_mask(mask.shape, 3)):
        r = mc.rule(s["local"], m)
        assert len(r["faces"]) > 300 and (mc.toward_camera(s["local"], r["face_pixels"], (0, 0, 0)) > 0).all()
        r = mc.rule(s["points"], m)
        view = r["face_pixels"][:, 0] // hw
        for i in range(4):
            assert (mc.toward_camera(s["points"], r["face_pixels"][view == i], s["poses"][i, :3, 3]) > 0).all()


def test_the_rule_equals_a_quad_by_quad_loop():
    s = mc.scene(2, 5, 7, seed=3)
    points = np.nan_to_num(s["points"], nan=0.0)
    mask = mc.random_mask((2, 5, 7), 11, keep=0.8)
    lengths = np.sqrt(np.sort(mc.rule(points, None)["ea"].reshape(-1)))
    for m, max_edge in ((None, None), (mask, None), (None, float(lengths[len(lengths) // 2])), (mask, float(lengths[len(lengths) // 3]))):
        r = mc.rule(points, m, max_edge)
        faces, used = mc.brute(points, m, max_edge)
        assert np.array_equal(r["face_pixels"], faces) and np.array_equal(r["used"] != 0, used) and len(faces) > 5
    assert len(mc.rule(points, mask, float(lengths[len(lengths) // 3]))["faces"]) < len(mc.rule(points, mask)["faces"])


def test_ties_and_nan_take_the_main_diagonal_and_the_stretch_filter_drops_nan():
    square = np.array([[[0, 0, 1], [1, 0, 1]], [[0, 1, 1], [1, 1, 1]]], np.float32)[None]        # both diagonals 2.0 exactly
    r = mc.rule(square)
    assert r["ea"].tolist() == r["em"].tolist() == [[[2.0]]] and r["code"][0, 0, 0] == mc.M1 | mc.M2
    assert r["face_pixels"].tolist() == [[0, 2, 3], [0, 3, 1]]
    for corner in range(4):
        for bad in (np.nan, np.inf, -np.inf):
            p = quad(anti_shorter=True)
            p.reshape(-1, 3)[corner, 1] = bad
            r = mc.rule(p)                                                                          # off: kept, main diagonal (inf - inf, or NaN)
            main = not (np.isinf(bad) and corner in (0, 3))                                         # em = +inf alone: the anti diagonal IS shorter
            assert r["code"][0, 0, 0] == (mc.M1 | mc.M2 if main else mc.A1 | mc.A2) and r["counts"].tolist() == [[4, 2]]
            on = mc.rule(p, None, 100.0)                                                            # on: the triangles with the corner go
            gone = [t for t in range(4) if any(dy * 2 + dx == corner for dy, dx in mc.TRIANGLES[t])]
            assert int(on["code"][0, 0, 0]) == int(r["code"][0, 0, 0]) & ~sum(1 << t for t in gone)
            assert mc.rule(p, None, np.inf)["counts"][0, 1] == (on["counts"][0, 1] if np.isnan(bad) else 2)   # inf <= inf holds, NaN never
    # equality with the limit is kept: an edge of exactly max_edge survives, one ulp more does not
    tri = np.array([[[0, 0, 1], [3, 0, 1]], [[0, 4, 1], [9, 9, 1]]], np.float32)[None]              # 3 - 4 - 5: the longest edge is 5 exactly
    three = np.array([[[1, 1], [1, 0]]], np.uint8)
    assert mc.rule(tri, three, 5.0)["counts"].tolist() == [[3, 1]]
    assert mc.rule(tri, three, np.nextafter(np.float32(5), np.float32(0)))["counts"].tolist() == [[0, 0]]
    assert mc.rule(square, three, 1.0)["counts"].tolist() == [[0, 0]]                               # its anti diagonal is sqrt 2 > 1


def test_invariants_of_the_numbering():
    s = mc.scene(3, 37, 70)
    for mask, max_edge in ((None, None), (mc.random_mask((3, 37, 70), 4, keep=0.5), None), (mc.depth_edge_mask(s["local"]), 0.2)):
        r = mc.rule(s["points"], mask, max_edge)
        V, F = len(r["vertex_pixel"]), len(r["faces"])
        assert V == r["counts"][:, 0].sum() and F == r["counts"][:, 1].sum() and F > 0
        assert r["faces"].min() >= 0 and r["faces"].max() < V
        assert np.array_equal(np.unique(r["faces"]), np.arange(V))                                  # every vertex is referenced
        assert (np.diff(r["vertex_pixel"]) > 0).all()
        assert np.array_equal(r["vertex_of"].reshape(-1)[r["vertex_pixel"]], np.arange(V)) and (r["vertex_of"] >= 0).sum() == V
        if mask is not None:
            assert not (r["used"][np.asarray(mask) == 0]).any()
        assert (r["face_pixels"][:, 0] // (37 * 70) == r["face_pixels"][:, 2] // (37 * 70)).all()  # no face joins two views
    board = mc.rule(s["points"], mc.checkerboard(3, 37, 70))
    assert board["counts"].tolist() == [[0, 0]] * 3 and len(board["faces"]) == 0 and len(board["vertex_pixel"]) == 0
    for shape in ((1, 1, 5), (1, 5, 1), (2, 1, 1)):
        empty = mc.rule(np.zeros(shape + (3,), np.float32))
        assert empty["counts"].tolist() == [[0, 0]] * shape[0] and empty["faces"].shape == (0, 3) and empty["face_records"].shape == (0, 13)


def test_fp32_equals_fp64_in_the_diagonal_choice_outside_the_near_ties():
    s = mc.scene(4, 37, 70)
    points = s["points"]
    r32, r64 = mc.rule(points, dtype=np.float32), mc.rule(points, dtype=np.float64)
    ok = np.isfinite(r64["ea"]) & np.isfinite(r64["em"])
    near = np.abs(r64["ea"] - r64["em"]) <= 1e-4 * np.maximum(r64["ea"], r64["em"])
    differ = (r32["anti"] != r64["anti"]) & ok
    print(f"near ties {near[ok].mean():.4%} of {int(ok.sum())} quads; differences {int(differ.sum())}, outside the near ties "
          f"{int((differ & ~near).sum())}; anti diagonals {r64['anti'][ok].mean():.1%}")
    assert ok.mean() > 0.5 and near[ok].mean() <= 0.01
    assert int((differ & ~near).sum()) == 0
    assert 0.2 < r64["anti"][ok].mean() < 0.8
