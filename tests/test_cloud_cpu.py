"""CPU (no GPU): the filtered point-cloud export and the intrinsics fit (csrc/cloud.hip, g2vlm_utils.save_point_cloud /
point_cloud_mask / estimate_intrinsics), in the style of tests/test_score_questions_cpu.py.

1. The C ABI: the three entry points and the two workspace queries are exported, declared and bound; every argument error comes
   back as -22 before anything touches a device.
2. The edge rule of tests/cloud_check.py - what the kernel is held to on the GPU - equals the reference's depth_edge bit for bit:
   on the committed fixture (tools/gen_depth_edge_golden.py) and live against the reference tree where there is one.
3. host.write_ply_records against host.write_ply_binary, the logit threshold, the inference_recon flags."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import cloud_check  # noqa: E402
from g2vlm_amd import hip, host  # noqa: E402

P, I, F, L64 = C.c_void_p, C.c_int, C.c_float, C.c_int64
ENTRY = ("g2v_cloud_mask", "g2v_cloud_compact", "g2v_intrinsics_lsq")
QUERY = ("g2v_cloud_compact_workspace", "g2v_intrinsics_lsq_workspace")
MASK_NAMES = ("points", "local", "conf", "N", "H", "W", "flags", "conf_logit_min", "edge_atol", "edge_rtol", "mask", "stream")
COMPACT_NAMES = ("points", "colors", "mask", "N", "H", "W", "records", "max_records", "counts", "workspace", "workspace_bytes", "stream")
LSQ_NAMES = ("local", "mask", "N", "H", "W", "K", "used", "workspace", "workspace_bytes", "stream")


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
    for name, names in zip(ENTRY, (MASK_NAMES, COMPACT_NAMES, LSQ_NAMES)):
        assert hasattr(lib, name) and name in hip.EXPORTS
        decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(decl.split(",")) == len(hip._SIGS[name][0]) == len(names), name
        assert [d.split()[-1].lstrip("*") for d in decl.split(",")] == list(names)
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in QUERY:
        assert hasattr(lib, name) and name in hip.EXPORTS
        decl = re.search(r"\bint64_t %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(decl.split(",")) == len(hip._SIGS[name][0]) == 3 and hip._SIGS[name][1] is C.c_int64
    assert "cloud.hip" in build.SOURCES and "cloud.hip" not in build.RESOURCE_AUDIT
    for bit, name in ((1, "FINITE"), (2, "CONF"), (4, "EDGE_ATOL"), (8, "EDGE_RTOL")):
        assert re.search(r"#define G2V_CLOUD_%s %d\b" % (name, bit), hdr) and getattr(hip, "CLOUD_" + name) == bit
    assert lib.g2v_version() == 1


def call_mask(lib, **kw):
    """A valid argument set (no pointer is dereferenced: every call below is refused before any launch), with overrides."""
    a = dict(points=16, local=16, conf=16, N=3, H=37, W=70, flags=15, conf_logit_min=0.0, edge_atol=0.1, edge_rtol=0.03, mask=16, stream=None)
    a.update(kw)
    return lib.g2v_cloud_mask(*[a[k] for k in MASK_NAMES])


def call_compact(lib, **kw):
    a = dict(points=16, colors=16, mask=16, N=3, H=37, W=70, records=16, max_records=3 * 37 * 70, counts=16, workspace=16,
             workspace_bytes=1 << 20, stream=None)
    a.update(kw)
    return lib.g2v_cloud_compact(*[a[k] for k in COMPACT_NAMES])


def call_lsq(lib, **kw):
    a = dict(local=16, mask=None, N=3, H=37, W=70, K=16, used=16, workspace=16, workspace_bytes=1 << 20, stream=None)
    a.update(kw)
    return lib.g2v_intrinsics_lsq(*[a[k] for k in LSQ_NAMES])


SHAPES_BAD = [dict(N=0), dict(N=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-1), dict(N=4, H=32768, W=32768),
              dict(N=1, H=46341, W=46341), dict(N=2, H=2 ** 15, W=2 ** 15)]


@pytest.mark.parametrize("bad", SHAPES_BAD + [dict(mask=None), dict(points=None), dict(local=None), dict(conf=None),
                                              dict(flags=1, points=None), dict(flags=2, conf=None), dict(flags=4, local=None),
                                              dict(flags=8, local=None), dict(flags=16), dict(flags=-1), dict(points=18)])
def test_mask_argument_errors_return_einval_without_a_device(lib, bad):
    assert call_mask(lib, **bad) == -22


@pytest.mark.parametrize("bad", SHAPES_BAD + [dict(points=None), dict(colors=None), dict(mask=None), dict(counts=None), dict(records=None),
                                              dict(workspace=None), dict(workspace_bytes=0), dict(workspace_bytes=8 * 3 * 3 - 1),
                                              dict(max_records=-1), dict(N=65536, H=1, W=1)])
def test_compact_argument_errors_return_einval_without_a_device(lib, bad):
    assert call_compact(lib, **bad) == -22


@pytest.mark.parametrize("bad", SHAPES_BAD + [dict(local=None), dict(K=None), dict(used=None), dict(workspace=None), dict(workspace_bytes=0),
                                              dict(workspace_bytes=72 * 3 * 3 - 1), dict(workspace=20)])
def test_intrinsics_argument_errors_return_einval_without_a_device(lib, bad):
    assert call_lsq(lib, **bad) == -22


def test_the_workspace_queries(lib):
    cw, iw = lib.g2v_cloud_compact_workspace, lib.g2v_intrinsics_lsq_workspace
    for bad in ((0, 5, 5), (3, 0, 5), (3, 5, -1), (4, 32768, 32768)):
        assert cw(*bad) == 0 and iw(*bad) == 0
    # two int32 per block of 1024 pixels of a view; nine fp64 sums per workgroup of 1024 pixels, at most 64 workgroups per view
    assert cw(3, 37, 70) == 8 * 3 * 3 and cw(1, 1, 1) == 8 and cw(2, 518, 518) == 8 * 2 * 263 and cw(1, 32, 32) == 8 and cw(1, 32, 33) == 16
    assert iw(3, 37, 70) == 72 * 3 * 3 and iw(1, 1, 1) == 72 and iw(1, 518, 518) == 72 * 64 and iw(8, 518, 518) == 72 * 8 * 64
    assert 2 * 263 > 256                                     # the GPU test's 2 x 518 x 518: more blocks than one pass of the scan takes


# ------------------------------------------------------------------------------------------------ 2. the edge rule
def _check_against(bits_of):
    """bits_of(name, depth) -> uint8 bits as the fixture stores them; compares cloud_check.edge_mask for every case and pair"""
    cases = cloud_check.edge_cases()
    seen = 0
    for name, d in cases.items():
        bits = bits_of(name, d)
        assert bits.shape == d.shape
        for i, (atol, rtol) in enumerate(cloud_check.EDGE_TOLS):
            want = (bits >> i) & 1
            got = cloud_check.edge_mask(d, atol, rtol)
            assert np.array_equal(got, want.astype(bool)), (name, atol, rtol, int((got != want.astype(bool)).sum()))
            seen += int(want.sum())
    assert seen > 100                                         # the cases do contain edges


def test_edge_rule_equals_the_reference_on_the_committed_fixture():
    from safetensors.numpy import load_file
    meta = json.load(open(cloud_check.GOLDEN + ".json"))
    assert [tuple(t) for t in meta["tols"]] == list(cloud_check.EDGE_TOLS) and [tuple(s) for s in meta["shapes"]] == list(cloud_check.EDGE_SHAPES)
    assert os.path.getsize(cloud_check.GOLDEN + ".safetensors") < 100 * 1024
    g = load_file(cloud_check.GOLDEN + ".safetensors")
    cases = cloud_check.edge_cases()
    assert set(g) == set(cases) | {"e" + k[1:] for k in cases}
    special = 0
    for name, d in cases.items():                             # the generator reproduces the stored depths: same bits, NaN included
        assert g[name].dtype == np.float32 and np.array_equal(g[name].view(np.uint32), d.view(np.uint32)), name
        special += int((~np.isfinite(d)).sum() + (d <= 0).sum())
    assert special > 50
    _check_against(lambda name, d: g["e" + name[1:]])


def test_edge_rule_equals_the_reference_live():
    from oracle.ref_shim import REF_ROOT
    if not os.path.exists(os.path.join(REF_ROOT, "modeling", "pi3", "utils", "geometry.py")):
        pytest.skip("no reference tree here")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_depth_edge_golden as gen
    depth_edge = gen.load_depth_edge(REF_ROOT)
    _check_against(lambda name, d: gen.reference_bits(depth_edge, d, cloud_check.EDGE_TOLS))


# ------------------------------------------------------------------------------------------------ 3. host side
def _pack_on_host(points, colors01):
    rec = np.zeros((len(points), 15), dtype=np.uint8)
    rec[:, :12] = np.ascontiguousarray(points, dtype="<f4").view(np.uint8).reshape(-1, 12)
    rec[:, 12:] = (np.clip(colors01.astype(np.float64), 0, 1) * 255).astype(np.uint8)
    return rec


@pytest.mark.parametrize("m", [0, 1, 7, 1000])
def test_write_ply_records_equals_write_ply_binary(tmp_path, m):
    rng = np.random.default_rng(m)
    pts = rng.standard_normal((m, 3)).astype(np.float32)
    col = rng.random((m, 3)).astype(np.float32) * 1.2 - 0.1
    a, b = tmp_path / "a.ply", tmp_path / "b.ply"
    host.write_ply_binary(str(a), pts, col)
    host.write_ply_records(str(b), _pack_on_host(pts, col))
    assert a.read_bytes() == b.read_bytes() and f"element vertex {m}\n".encode() in b.read_bytes()
    import torch
    host.write_ply_records(str(b), torch.from_numpy(_pack_on_host(pts, col)))
    assert a.read_bytes() == b.read_bytes()
    for bad in (np.zeros((3, 14), np.uint8), np.zeros((3, 15), np.int8), np.zeros(15, np.uint8)):
        with pytest.raises(ValueError):
            host.write_ply_records(str(b), bad)


def test_the_logit_threshold():
    f = host.conf_logit_threshold
    assert f(0.5) == 0.0
    ps = [1e-6, 0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1 - 1e-6]
    vals = [f(p) for p in ps]
    assert all(a < b for a, b in zip(vals, vals[1:])) and all(v == float(np.float32(v)) for v in vals)
    assert f(0.9) == float(np.float32(np.log(9.0))) and f(0.1) == -f(0.9)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), 20.0):
        with pytest.raises(ValueError):
            f(bad)


def test_public_functions_refuse_bad_arguments_before_any_launch(monkeypatch):
    import torch
    import g2vlm_utils as top
    from g2vlm_amd import g2vlm_utils as gu
    assert top.save_point_cloud is gu.save_point_cloud and top.point_cloud_mask is gu.point_cloud_mask
    assert top.estimate_intrinsics is gu.estimate_intrinsics
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("a refused call reached the library"))
    pred = dict(points=torch.zeros(1, 2, 4, 6, 3), local_points=torch.ones(1, 2, 4, 6, 3), conf=None, images=torch.zeros(1, 2, 3, 4, 6))
    with_conf = dict(pred, conf=torch.zeros(1, 2, 4, 6, 1))
    for fn in (lambda **kw: gu.point_cloud_mask(pred, **kw), lambda **kw: gu.save_point_cloud(pred, "unused.ply", **kw)):
        with pytest.raises(ValueError, match="conf"):
            fn(conf_threshold=0.5)
        for kw in (dict(edge_rtol=-0.01), dict(edge_atol=-1.0), dict(edge_rtol=float("nan"))):
            with pytest.raises(ValueError):
                fn(**kw)
    for p in (0.0, 1.0, 20.0, -1.0):
        with pytest.raises(ValueError):
            gu.point_cloud_mask(with_conf, conf_threshold=p)
    small = dict(pred, images=torch.zeros(1, 2, 3, 8, 6))
    for fn in (lambda: gu.point_cloud_mask(small), lambda: gu.save_point_cloud(small, "unused.ply"), lambda: gu.estimate_intrinsics(small)):
        with pytest.raises(ValueError, match="images"):
            fn()
    with pytest.raises(ValueError):
        gu.estimate_intrinsics(dict(pred, points=torch.zeros(2, 2, 4, 6, 3), local_points=torch.ones(2, 2, 4, 6, 3)))
    assert not os.path.exists("unused.ply")


def test_inference_recon_has_the_new_flags_off_by_default():
    import inference_recon
    a = inference_recon.parser.parse_args([])
    assert a.conf_threshold is None and a.edge_rtol is None and a.edge_atol is None and a.intrinsics is False
    assert (a.image_folder, a.model_path, a.save_path) == ("examples/dl3dv/", "InternRobotics/G2VLM-2B-MoT", "results/arkitscenes_results.ply")
    b = inference_recon.parser.parse_args(["--conf-threshold", "0.3", "--edge-rtol", "0.03", "--edge-atol", "0.5", "--intrinsics"])
    assert (b.conf_threshold, b.edge_rtol, b.edge_atol, b.intrinsics) == (0.3, 0.03, 0.5, True)
