"""CPU (no GPU): the nearest-neighbour search and the evaluation built on it (csrc/nn.hip, g2vlm_utils.nearest_points / align_points /
evaluate_reconstruction), in the style of tests/test_mesh_cpu.py.

1. The C ABI: the entry point and its workspace query are exported, declared and bound; every argument error comes back as -22
   before anything touches a device; the workspace's closed form.
2. The public functions refuse bad arguments before any launch; signatures; the inference_recon flags.
3. The rule of tests/nn_check.py - what the kernel is held to on the GPU: ties, duplicates, masks, non-finite points, the distance
   limit at equality and one ulp below, overflow, empty sides, fp32 against fp64, a set that a fused multiply-add would change.
4. align_points against an fp64 numpy Umeyama; the metrics on clouds small enough to compute by hand."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import nn_check as nc  # noqa: E402
from g2vlm_amd import hip  # noqa: E402

NAMES = ("query", "query_mask", "Nq", "target", "target_mask", "Nt", "max_distance", "flags", "index", "sq_distance", "stats", "workspace",
         "workspace_bytes", "stream")


# ------------------------------------------------------------------------------------------------ 1. the C ABI
@pytest.fixture(scope="module")
def lib():
    from g2vlm_amd import build
    lib = C.CDLL(build.build())
    for name in ("g2v_cloud_nn", "g2v_cloud_nn_workspace"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = hip._SIGS[name]
    return lib


def test_library_exports_and_declares_the_entry_points(lib):
    from g2vlm_amd import build
    hdr = open(os.path.join(ROOT, "include", "g2vlm_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    name = "g2v_cloud_nn"
    assert hasattr(lib, name) and name in hip.EXPORTS and ("`%s`" % name) in integration
    decl = re.search(r"\bint %s\((.*?)\);" % name, hdr, re.S).group(1)
    assert len(decl.split(",")) == len(hip._SIGS[name][0]) == len(NAMES)
    assert [d.split()[-1].lstrip("*") for d in decl.split(",")] == list(NAMES)
    q = name + "_workspace"
    assert hasattr(lib, q) and q in hip.EXPORTS and ("`%s`" % q) in integration
    decl = re.search(r"\bint64_t %s\((.*?)\);" % q, hdr, re.S).group(1)
    assert [d.split()[-1] for d in decl.split(",")] == ["Nq", "Nt"] and hip._SIGS[q] == ([C.c_int64] * 2, C.c_int64)
    assert "nn.hip" in build.SOURCES and "nn.hip" not in build.RESOURCE_AUDIT
    assert re.search(r"#define G2V_NN_BRUTE 1\b", hdr) and re.search(r"#define G2V_NN_GRID 2\b", hdr) and (hip.NN_BRUTE, hip.NN_GRID) == (1, 2)
    src = open(os.path.join(ROOT, "g2vlm_amd", "csrc", "cloud_common.h")).read()   # sq_dist3: the rule's squared distance
    assert "#pragma clang fp contract(off)" in src
    for export in ("`nearest_points`", "`align_points`", "`evaluate_reconstruction`"):
        assert export in integration
    assert "## 6p. " in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert lib.g2v_version() == 1


def call(lib, **kw):
    """A valid argument set (no pointer is dereferenced: every call below is refused before any launch), with overrides."""
    a = dict(query=16, query_mask=17, Nq=100, target=32, target_mask=19, Nt=5000, max_distance=0.5, flags=0, index=16, sq_distance=16,
             stats=16, workspace=64, workspace_bytes=1 << 30, stream=None)
    a.update(kw)
    return lib.g2v_cloud_nn(*[a[k] for k in NAMES])


def workspace_bytes(Nq, Nt):
    """the stated closed form: 256 + 24 Nt + 8 Nq + 4 (G^3 + 1) + 4 ceil(G^3 / 1024), G = the largest G with G^3 <= 2 Nt in [1, 256]"""
    G = 1
    while G < 256 and (G + 1) ** 3 <= 2 * Nt:
        G += 1
    return 256 + 24 * Nt + 8 * Nq + 4 * (G ** 3 + 1) + 4 * ((G ** 3 + 1023) // 1024)


BAD = [dict(Nq=-1), dict(Nt=-1), dict(Nq=2 ** 31), dict(Nt=2 ** 31, workspace_bytes=1 << 62), dict(query=None), dict(target=None),
       dict(index=None), dict(sq_distance=None), dict(stats=None), dict(workspace=None), dict(query=18), dict(target=34), dict(index=18),
       dict(sq_distance=17), dict(stats=18), dict(workspace=72), dict(workspace=68), dict(max_distance=-1.0), dict(max_distance=-0.5, flags=1),
       dict(max_distance=float("nan")), dict(max_distance=float("-inf")), dict(flags=4), dict(flags=-1), dict(flags=3), dict(flags=8 | 1),
       dict(workspace_bytes=0), dict(workspace_bytes=workspace_bytes(100, 5000) - 1)]


@pytest.mark.parametrize("bad", BAD)
def test_argument_errors_return_einval_without_a_device(lib, bad):
    assert call(lib, **bad) == -22


def test_the_workspace_query(lib):
    ws = lib.g2v_cloud_nn_workspace
    for bad in ((-1, 5), (5, -1), (2 ** 31, 1), (1, 2 ** 31)):
        assert ws(*bad) == 0                                                                       # 0 for every count the entry point refuses
    assert ws(0, 0) == 256 + 8 + 4 and ws(1, 1) == 256 + 24 + 8 + 8 + 4                             # G = 1
    for Nq, Nt in ((1, 3), (1, 4), (65, 63), (7770, 7770), (268324, 300000), (8 * 518 * 518, 8 * 518 * 518), (5, 2 ** 23 - 1), (5, 2 ** 23),
                   (2 ** 31 - 1, 2 ** 31 - 1)):
        assert ws(Nq, Nt) == workspace_bytes(Nq, Nt), (Nq, Nt)
    assert workspace_bytes(1, 3) == 256 + 72 + 8 + 8 + 4 and workspace_bytes(1, 4) == 256 + 96 + 8 + 36 + 4   # G = 2 from four targets on
    assert workspace_bytes(0, 2 ** 23) == 256 + 24 * 2 ** 23 + 4 * (2 ** 24 + 1) + 4 * 2 ** 14                 # G = 256: the cap


# ------------------------------------------------------------------------------------------------ 2. the public surface
def test_public_functions_refuse_bad_arguments_before_any_launch(monkeypatch):
    import torch
    import g2vlm_utils as top
    from g2vlm_amd import g2vlm_utils as gu
    for name in ("nearest_points", "align_points", "evaluate_reconstruction"):
        assert getattr(top, name) is getattr(gu, name) and name in top.__all__
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("a refused call reached the library"))
    q, t = torch.zeros(5, 3), torch.ones(7, 3)
    for args, kw in (((q, t), dict(max_distance=-1.0)), ((q, t), dict(max_distance=float("nan"))), ((q, t), dict(max_distance="far")),
                     ((q, t), dict(max_distance=True)), ((torch.zeros(5, 2), t), {}), ((q, torch.ones(7, 4)), {}), ((q.numpy(), t), {}),
                     ((q.long(), t), {}), ((q, t), dict(query_mask=torch.ones(4, dtype=torch.bool))), ((q, t), dict(target_mask=torch.ones(7))),
                     ((q, t), dict(target_mask=np.ones(7, bool))), ((q, t), {})):                   # the last: not on a GPU
        with pytest.raises(ValueError):
            gu.nearest_points(*args, **kw)
    for args, kw in (((q, t), {}), ((q, q.numpy()), {}), ((q, q), dict(mask=torch.ones(4, dtype=torch.bool))), ((q, q), dict(with_scale=1)),
                     ((q, q), dict(mask=torch.ones(5))), ((torch.zeros(5, 2), torch.zeros(5, 2)), {})):
        with pytest.raises(ValueError):
            gu.align_points(*args, **kw)
    pred = dict(points=torch.zeros(1, 2, 4, 6, 3), local_points=torch.ones(1, 2, 4, 6, 3), conf=None, images=torch.zeros(1, 2, 3, 4, 6))
    grid, cloud = torch.zeros(2, 4, 6, 3), torch.zeros(9, 3)
    ok_mask = torch.ones(2, 4, 6, dtype=torch.bool)
    bad_last_row = torch.eye(4)
    bad_last_row[3, 0] = 1.0
    for gt, kw in ((grid, dict(thresholds=(0.0,))), (grid, dict(thresholds=(-1.0,))),
                   (grid, dict(thresholds=(float("nan"),))), (grid, dict(thresholds=0.05)), (grid, dict(thresholds=("a",))),
                   (grid, dict(thresholds=(True,))), (grid, dict(max_distance=-1.0)), (grid, dict(max_distance=float("nan"))),
                   (grid, dict(align="icp")), (grid, dict(align=None)), (grid, dict(align=torch.eye(3))), (grid, dict(align=bad_last_row)),
                   (grid, dict(align=torch.full((4, 4), float("nan")))), (cloud, {}), (cloud, dict(align="sim3")),
                   (torch.zeros(2, 4, 5, 3), {}), (torch.zeros(2, 4, 6, 2), {}), (torch.zeros(4, 6, 3), {}), (grid.numpy(), {}),
                   (grid.long(), {}), (grid, dict(gt_mask=torch.ones(2, 4, 5, dtype=torch.bool))), (grid, dict(gt_mask=torch.ones(2, 4, 6))),
                   (cloud, dict(align="none", gt_mask=torch.ones(8, dtype=torch.bool))), (grid, dict(conf_threshold=0.5)),
                   (grid, dict(edge_rtol=-1.0)), (grid, dict(edge_atol=-0.5)), (grid, dict(mask=torch.ones(2, 4, 5, dtype=torch.bool))),
                   (grid, dict(mask=torch.ones(2, 4, 6))), (grid, dict(mask=ok_mask, edge_rtol=0.03)), (grid, dict(mask=ok_mask, edge_atol=0.1)),
                   (grid, dict(mask=ok_mask, filter_nan=False)), (grid, dict(mask=ok_mask, conf_threshold=0.5)),
                   (grid, dict(return_distances=1))):
        with pytest.raises(ValueError):
            gu.evaluate_reconstruction(pred, gt, **kw)
    for bad in (dict(pred, points=torch.zeros(2, 4, 6, 3)), dict(pred, local_points=torch.ones(1, 2, 4, 5, 3))):
        with pytest.raises(ValueError):
            gu.evaluate_reconstruction(bad, grid)


def test_signatures_of_the_public_functions():
    from g2vlm_amd import g2vlm_utils as gu

    def sig(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()]
    E = inspect.Parameter.empty
    assert sig(gu.nearest_points) == [("query", E), ("target", E), ("max_distance", None), ("query_mask", None), ("target_mask", None)]
    assert sig(gu.align_points) == [("src", E), ("dst", E), ("mask", None), ("with_scale", True)]
    assert sig(gu.evaluate_reconstruction) == [("pred_dict", E), ("gt_points", E), ("gt_mask", None), ("align", "sim3"), ("thresholds", (0.05,)),
                                               ("max_distance", None), ("mask", None), ("conf_threshold", None), ("edge_rtol", None),
                                               ("edge_atol", None), ("filter_nan", True), ("return_distances", False)]
    assert sig(hip.cloud_nn) == [("query", E), ("target", E), ("max_distance", None), ("query_mask", None), ("target_mask", None), ("flags", 0),
                                 ("workspace", None)]
    assert sig(hip.cloud_nn_workspace) == [("Nq", E), ("Nt", E)]


def test_inference_recon_has_the_evaluation_flags_off_by_default(tmp_path):
    import inference_recon
    a = inference_recon.parser.parse_args([])
    assert a.evaluate is None and a.eval_threshold is None and a.eval_max_distance is None and a.eval_align is None
    b = inference_recon.parser.parse_args(["--evaluate", "gt.npy", "--eval-threshold", "0.05", "--eval-threshold", "0.1", "--eval-max-distance",
                                           "0.5", "--eval-align", "none"])
    assert (b.evaluate, b.eval_threshold, b.eval_max_distance, b.eval_align) == ("gt.npy", [0.05, 0.1], 0.5, "none")
    for flag in ("--evaluate", "--eval-threshold", "--eval-max-distance", "--eval-align"):
        assert flag in inference_recon.__doc__
    good, cloud, wrong = str(tmp_path / "gt.npy"), str(tmp_path / "cloud.npy"), str(tmp_path / "wrong.npy")
    np.save(good, np.zeros((2, 4, 6, 3), np.float32))
    np.save(cloud, np.zeros((9, 3), np.float32))
    np.save(wrong, np.zeros((9, 2), np.float32))
    for bad in (["--eval-threshold", "0.05"], ["--eval-max-distance", "1"], ["--eval-align", "none"], ["--evaluate", good, "--eval-threshold", "0"],
                ["--evaluate", good, "--eval-threshold", "nan"], ["--evaluate", good, "--eval-max-distance", "-1"],
                ["--evaluate", good, "--eval-align", "icp"], ["--evaluate", str(tmp_path / "missing.npy")], ["--evaluate", wrong],
                ["--evaluate", cloud, "--eval-align", "sim3"]):
        with pytest.raises(SystemExit):                                                            # refused before the model is loaded
            inference_recon.main(["--image_folder", HERE] + bad)


# ------------------------------------------------------------------------------------------------ 3. the rule
def centres(n=4):
    """the centres of the (n-1)^3 cells of the integer lattice: eight lattice points each at squared distance 0.75 exactly"""
    return nc.lattice(n - 1) + np.float32(0.5)


def test_ties_go_to_the_lowest_index_and_duplicates_too():
    T, Q = nc.lattice(4), centres(4)
    r = nc.rule(Q, T)
    assert (r["sq_distance"] == np.float32(0.75)).all()
    want = (Q[:, 0] - 0.5) + 4 * (Q[:, 1] - 0.5) + 16 * (Q[:, 2] - 0.5)                            # the corner with the lowest index
    assert np.array_equal(r["index"], want.astype(np.int32))
    perm = np.random.default_rng(0).permutation(64)
    rp = nc.rule(Q, T[perm])
    d2 = ((Q[:, None, :] - T[perm][None]) ** 2).sum(-1)
    assert np.array_equal(rp["index"], np.array([np.flatnonzero(row == 0.75)[0] for row in d2], np.int32))   # the first of the eight
    dup = np.concatenate([T, T, T[:5]])                                                              # every target twice, five three times
    rd = nc.rule(T, dup)
    assert np.array_equal(rd["index"], np.arange(64, dtype=np.int32)) and (rd["sq_distance"] == 0).all()
    masked = np.ones(len(dup), np.uint8)
    masked[:64] = 0
    assert np.array_equal(nc.rule(T, dup, target_mask=masked)["index"], np.arange(64, 128, dtype=np.int32))
    assert r["stats"].tolist() == [27, 64, 0, 27]


def test_masked_and_non_finite_points_take_no_part():
    rng = np.random.default_rng(1)
    Q, T = rng.standard_normal((40, 3)).astype(np.float32), rng.standard_normal((50, 3)).astype(np.float32)
    Q[3, 1], Q[7, 0], Q[9, 2] = np.nan, np.inf, -np.inf
    T[0, 0], T[11, 2] = np.nan, np.inf
    qm, tm = nc.random_mask(40, 2, keep=0.7), nc.random_mask(50, 3, keep=0.5)
    qm[3] = tm[0] = 200                                                                              # any non-zero byte keeps, but not a NaN
    r = nc.rule(Q, T, query_mask=qm, target_mask=tm)
    qpart, tpart = (qm != 0) & np.isfinite(Q).all(1), (tm != 0) & np.isfinite(T).all(1)
    assert (r["index"][~qpart] == -1).all() and np.isinf(r["sq_distance"][~qpart]).all()
    assert (r["index"][qpart] >= 0).all() and tpart[r["index"][qpart]].all()
    assert r["stats"].tolist() == [int(qpart.sum()), int(tpart.sum()), 0, int(qpart.sum())]
    for i in np.flatnonzero(qpart):                                                                  # a plain loop over the survivors
        d2 = ((Q[i].astype(np.float64) - T[tpart].astype(np.float64)) ** 2).sum(1)
        assert np.flatnonzero(tpart)[d2.argmin()] == r["index"][i]
    none = nc.rule(Q, T, target_mask=np.zeros(50, np.uint8))
    assert (none["index"] == -1).all() and none["stats"].tolist() == [37, 0, 37, 0]
    one = np.zeros(50, np.uint8)
    one[17] = 1
    assert set(nc.rule(Q, T, target_mask=one)["index"].tolist()) == {-1, 17}


def test_the_distance_limit_keeps_equality_and_drops_one_ulp_less():
    Q = np.zeros((1, 3), np.float32)
    T = np.array([[3, 4, 0], [0, 0, 6]], np.float32)                                                 # distances 5 and 6, exactly
    assert nc.rule(Q, T, 5.0)["index"].tolist() == [0] and nc.rule(Q, T, 5.0)["sq_distance"].tolist() == [25.0]
    below = float(np.nextafter(np.float32(5), np.float32(0)))
    r = nc.rule(Q, T, below)
    assert r["index"].tolist() == [-1] and np.isinf(r["sq_distance"][0]) and r["stats"].tolist() == [1, 2, 1, 0]
    assert nc.rule(Q, T[::-1].copy(), 5.5)["index"].tolist() == [1]                                   # the nearer one beyond a farther first
    assert nc.rule(Q, T, 0.0)["index"].tolist() == [-1] and nc.rule(Q, Q, 0.0)["index"].tolist() == [0]
    assert nc.rule(Q, T, np.inf)["index"].tolist() == [0] and nc.rule(Q, T, 1e30)["index"].tolist() == [0]   # the square overflows: no limit


def test_overflow_gives_inf_and_the_lowest_participating_index():
    Q = np.array([[1e20, 1e20, 1e20], [-1e20, 0, 0], [0, 0, 0]], np.float32)
    T = np.array([[-1e20, -1e20, -1e20], [-1e20, 1e20, -1e20], [1e20, -1e20, 1e20]], np.float32)
    r = nc.rule(Q, T)
    assert np.isinf(r["sq_distance"]).all() and r["index"].tolist() == [0, 0, 0] and r["stats"].tolist() == [3, 3, 0, 3]
    r = nc.rule(Q, T, target_mask=np.array([0, 1, 1], np.uint8))
    assert r["index"].tolist() == [1, 1, 1]
    r = nc.rule(Q, T, 1e19)                                                                          # a finite limit: +inf does not count
    assert r["index"].tolist() == [-1, -1, -1] and r["stats"].tolist() == [3, 3, 3, 0]
    mixed = np.concatenate([T, np.array([[1e20, 1e20, 0.9e20]], np.float32)])                        # one finite d2 among the infinite
    assert nc.rule(Q[:1], mixed)["index"].tolist() == [3]


def test_empty_sides_are_valid():
    Q, T = np.zeros((4, 3), np.float32), np.zeros((0, 3), np.float32)
    r = nc.rule(Q, T)
    assert r["index"].tolist() == [-1] * 4 and np.isinf(r["sq_distance"]).all() and r["stats"].tolist() == [4, 0, 4, 0]
    r = nc.rule(T, Q)
    assert r["index"].shape == (0,) and r["sq_distance"].shape == (0,) and r["stats"].tolist() == [0, 4, 0, 0]
    assert nc.rule(T, T)["stats"].tolist() == [0, 0, 0, 0]


def test_fp32_equals_fp64_in_the_chosen_index_outside_the_near_ties():
    s = nc.scene(3, 37, 70)
    P = s["points"].reshape(-1, 3)
    P = P[np.isfinite(P).all(1)]
    G = nc.moved(P, seed=4, scale=1.0, noise=0.004)
    r32 = nc.rule(P, G)
    idx64, gap = nc.gap64(P, G)
    near = gap < 1e-5
    differ = r32["index"] != idx64
    print(f"{len(P)} queries against {len(G)} targets: near ties (relative fp64 gap below 1e-5) {near.mean():.4%}, the index differs on "
          f"{int(differ.sum())}, outside the near ties on {int((differ & ~near).sum())}")
    assert len(P) > 5000 and near.mean() <= 0.01
    assert int((differ & ~near).sum()) == 0


def test_a_set_on_which_a_fused_multiply_add_would_change_a_bit():
    Q, T = nc.fma_set()
    assert 48 <= len(Q) <= 48 * len(nc.FUSED)
    r = nc.rule(Q, T)
    assert np.array_equal(r["index"], np.arange(len(Q), dtype=np.int32))                             # query k's neighbour is target k
    plain = nc.sq_dist(Q, T)
    assert np.array_equal(r["sq_distance"].view(np.int32), plain.view(np.int32))
    for form in nc.FUSED:
        # the FMA emulated in fp64: the product of two fp32 numbers is exact there, the sum is rounded once
        fused = nc.sq_dist(Q, T, form)
        differ = fused.view(np.int32) != plain.view(np.int32)
        assert differ.sum() >= 8, (form, int(differ.sum()))
        rf = nc.rule(Q, T, fused=form)
        assert (rf["sq_distance"].view(np.int32) != r["sq_distance"].view(np.int32)).sum() >= 8


# ------------------------------------------------------------------------------------------------ 4. alignment and metrics
def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_align_points_recovers_a_planted_similarity_and_equals_numpy():
    import torch
    from g2vlm_amd import g2vlm_utils as gu
    rng = np.random.default_rng(6)
    src = rng.uniform(-2, 2, (8000, 3)).astype(np.float32)
    s, R, t = nc.similarity(seed=2, scale=1.7)
    exact = (s * (src.astype(np.float64) @ R.T) + t).astype(np.float32)
    got = gu.align_points(torch.from_numpy(src), torch.from_numpy(exact))
    assert abs(got["scale"] - s) < 1e-6 and rel(got["rotation"].numpy(), R) < 1e-6 and rel(got["translation"].numpy(), t) < 1e-5
    assert got["num_points"] == 8000 and got["transform"].dtype == torch.float64 and tuple(got["transform"].shape) == (4, 4)
    noisy = nc.moved(src, seed=2, scale=1.7, noise=0.01)
    for with_scale in (True, False):
        got = gu.align_points(torch.from_numpy(src), torch.from_numpy(noisy), with_scale=with_scale)
        ws, wR, wt = nc.umeyama(src, noisy, with_scale)
        assert rel(got["transform"].numpy(), nc.transform_of(ws, wR, wt)) < 1e-9
        assert rel(got["rotation"].numpy(), wR) < 1e-9 and abs(got["scale"] - ws) < 1e-9 * ws and rel(got["translation"].numpy(), wt) < 1e-9
        assert abs(np.linalg.det(got["rotation"].numpy()) - 1) < 1e-12 and (with_scale or got["scale"] == 1.0)
    # any shape [...,3]
    got = gu.align_points(torch.from_numpy(src.reshape(20, 400, 3)), torch.from_numpy(noisy.reshape(20, 400, 3)))
    assert rel(got["transform"].numpy(), nc.transform_of(*nc.umeyama(src, noisy))) < 1e-9


def test_align_points_handles_the_reflection_case_and_a_masked_subset():
    import torch
    from g2vlm_amd import g2vlm_utils as gu
    rng = np.random.default_rng(8)
    src = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    mirrored = src * np.array([1, 1, -1], np.float32) + 0.01 * rng.standard_normal((500, 3)).astype(np.float32)
    got = gu.align_points(torch.from_numpy(src), torch.from_numpy(mirrored))
    assert abs(np.linalg.det(got["rotation"].numpy()) - 1) < 1e-12                                  # a rotation, not the mirror
    want = nc.umeyama(src, mirrored)
    assert np.linalg.det(want[1]) > 0 and rel(got["transform"].numpy(), nc.transform_of(*want)) < 1e-9
    # a masked subset, with non-finite rows and outliers outside it
    dst = nc.moved(src, seed=5, scale=0.6, noise=0.002)
    mask = nc.random_mask(500, 9, keep=0.6)
    wild_s, wild_d = src.copy(), dst.copy()
    wild_d[mask == 0] += 50.0
    wild_s[3], wild_d[10, 1] = np.nan, np.inf
    keep = (mask != 0) & np.isfinite(wild_s).all(1) & np.isfinite(wild_d).all(1)
    for m in (torch.from_numpy(mask), torch.from_numpy(mask != 0)):
        got = gu.align_points(torch.from_numpy(wild_s), torch.from_numpy(wild_d), mask=m)
        assert got["num_points"] == int(keep.sum())
        assert rel(got["transform"].numpy(), nc.transform_of(*nc.umeyama(src[keep], dst[keep]))) < 1e-9
    with pytest.raises(ValueError):
        gu.align_points(torch.from_numpy(src), torch.from_numpy(dst), mask=torch.zeros(500, dtype=torch.bool))
    with pytest.raises(ValueError):
        gu.align_points(torch.zeros(10, 3), torch.from_numpy(dst[:10]))                             # no spread


def metrics_of(pred, gt, thresholds, max_distance=None):
    """the product's metrics from the rule's two searches, and nn_check's own"""
    import torch
    from g2vlm_amd import g2vlm_utils as gu
    a, c = nc.rule(pred, gt, max_distance), nc.rule(gt, pred, max_distance)
    out, dist = gu._metrics_from_distances(torch.from_numpy(a["sq_distance"]), torch.from_numpy(a["index"] >= 0),
                                           torch.from_numpy(c["sq_distance"]), torch.from_numpy(c["index"] >= 0), thresholds, max_distance)
    return out, dist, nc.metrics(pred, gt, thresholds, max_distance)


def test_metrics_on_clouds_small_enough_to_compute_by_hand():
    pred = np.array([[0, 0, 0], [30, 0, 0]], np.float32)
    gt = np.array([[0, 0, 0.75], [33, 4, 0], [30, 0, -7]], np.float32)
    # pred -> gt: 0.75 and 5; gt -> pred: 0.75, 5, 7
    out, dist, ref = metrics_of(pred, gt, (0.75, 4.5, 5.0))
    assert dist["accuracy"].tolist() == [0.75, 5.0] and dist["completeness"].tolist() == [0.75, 5.0, 7.0]
    assert out["accuracy"] == 2.875 and out["completeness"] == 4.25 and out["chamfer"] == 0.5 * (2.875 + 4.25)
    assert out["accuracy_median"] == 2.875 and out["completeness_median"] == 5.0
    assert (out["n_pred"], out["n_gt"]) == (2, 3) and out["thresholds"] == (0.75, 4.5, 5.0)
    assert out["precision_hits"] == [1, 1, 2] and out["recall_hits"] == [1, 1, 2]                   # a threshold equal to a distance counts
    assert out["precision"] == [0.5, 0.5, 1.0] and out["recall"] == [1 / 3, 1 / 3, 2 / 3]
    assert out["fscore"] == [2 * 0.5 * (1 / 3) / (0.5 + 1 / 3), 2 * 0.5 * (1 / 3) / (0.5 + 1 / 3), 2 * 1.0 * (2 / 3) / (1.0 + 2 / 3)]
    below = float(np.nextafter(np.float32(0.75), np.float32(0)))
    assert metrics_of(pred, gt, (below,))[0]["precision_hits"] == [0]
    for k, T in enumerate(out["thresholds"]):
        assert ref[T] == dict(precision=out["precision"][k], recall=out["recall"][k], fscore=out["fscore"][k])
    assert (ref["accuracy"], ref["completeness"], ref["chamfer"]) == (out["accuracy"], out["completeness"], out["chamfer"])

    # the clipping rule: with max_distance 4.5 the neighbours at 5 and 7 do not count - misses at every threshold, 4.5 in the means
    out, dist, ref = metrics_of(pred, gt, (4.5, 100.0), max_distance=4.5)
    assert dist["accuracy"].tolist() == [0.75, 4.5] and dist["completeness"].tolist() == [0.75, 4.5, 4.5]
    assert out["accuracy"] == 2.625 and out["completeness"] == 3.25 and out["completeness_median"] == 4.5
    assert out["precision_hits"] == [1, 1] and out["recall_hits"] == [1, 1]
    assert (ref["accuracy"], ref["completeness"]) == (out["accuracy"], out["completeness"]) and ref["hits"]["accuracy"] == [1, 1]
    out, dist, _ = metrics_of(pred, gt, (1.0,), max_distance=5.0)                                   # equality with max_distance counts
    assert dist["accuracy"].tolist() == [0.75, 5.0] and out["precision_hits"] == [1]

    # an empty prediction: NaN for its side, the chamfer distance and the F-score; recall 0
    out, dist, ref = metrics_of(np.zeros((0, 3), np.float32), gt, (1.0,), max_distance=2.0)
    assert np.isnan(out["accuracy"]) and np.isnan(out["accuracy_median"]) and np.isnan(out["chamfer"]) and np.isnan(out["precision"][0])
    assert out["completeness"] == 2.0 and out["recall"] == [0.0] and np.isnan(out["fscore"][0]) and (out["n_pred"], out["n_gt"]) == (0, 3)
    assert np.isnan(ref["accuracy"]) and ref["completeness"] == 2.0
    out, _, _ = metrics_of(np.zeros((0, 3), np.float32), gt, (1.0,))
    assert np.isinf(out["completeness"]) and out["recall"] == [0.0]
    out, _, _ = metrics_of(pred + 100, gt, (1.0,))                                                   # nothing within the threshold
    assert out["precision"] == [0.0] and out["recall"] == [0.0] and out["fscore"] == [0.0]


def test_apply_transform_equals_the_checker_bit_for_bit():
    import torch
    from g2vlm_amd import g2vlm_utils as gu
    P = nc.scene(2, 9, 13)["points"].reshape(-1, 3).copy()
    P[5, 1] = np.nan
    M =nc.transform_of(*nc.similarity(seed=3, scale=0.8))
    got = gu._apply_transform(M, torch.from_numpy(P)).numpy()
    assert np.array_equal(got.view(np.int32), nc.apply_transform(M, P).view(np.int32)) and np.isnan(got).any()
    lines = gu.format_evaluation(metrics_of(P[np.isfinite(P).all(1)], nc.moved(P[np.isfinite(P).all(1)], 1, 1.0), (0.05, 0.1))[0])
    assert len(lines) == 6 and "chamfer" in lines[3] and "fscore" in lines[5]
