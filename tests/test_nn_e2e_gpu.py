"""GPU, end to end: nearest_points and evaluate_reconstruction on a recon-shaped result built from the synthetic scene, against the
rule and the fp64 metrics of tests/nn_check.py; inference_recon --evaluate on the tiny synthetic model."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import nn_check as nc  # noqa: E402
from g2vlm_amd.g2vlm_utils import evaluate_reconstruction, format_evaluation, nearest_points, point_cloud_mask  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPE = (3, 37, 70)                                                                                  # 7 770 points: the means have < 1e4 terms
THRESHOLDS = (0.005, 0.02, 0.05)


@functools.lru_cache(maxsize=None)
def case():
    """(the scene, a prediction dict of it on the device, ground truth = the scene under a planted similarity plus noise, with holes)"""
    s = nc.scene(*SHAPE)
    points = s["points"].copy()
    points[0, :3, :5] = np.nan                                                                       # a patch the prediction lacks
    gt = nc.moved(s["points"], seed=7, scale=1.4, noise=0.004)
    gt[1, 10:14, 20:30] = np.nan                                                                     # and one the ground truth lacks
    pred = dict(points=torch.from_numpy(points)[None].cuda(), local_points=torch.from_numpy(s["local"])[None].cuda(), conf=None,
                images=torch.rand(1, SHAPE[0], 3, SHAPE[1], SHAPE[2]).cuda(), camera_poses=torch.from_numpy(s["poses"])[None].cuda())
    return s, pred, gt


def rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


def check_metrics(out, ref, thresholds):
    for key in ("accuracy", "completeness", "chamfer", "accuracy_median", "completeness_median"):
        print(f"{key}: {out[key]!r} against {ref[key]!r}")
        assert rel(out[key], ref[key]) <= 1e-10, key
    assert (out["n_pred"], out["n_gt"]) == (ref["n_pred"], ref["n_gt"]) and out["thresholds"] == tuple(thresholds)
    assert out["precision_hits"] == ref["hits"]["accuracy"] and out["recall_hits"] == ref["hits"]["completeness"]   # counts: exactly
    for k, T in enumerate(thresholds):
        for key in ("precision", "recall", "fscore"):
            assert rel(out[key][k], ref[T][key]) <= 1e-10, (key, T)


def test_nearest_points_equals_the_rule():
    s, pred, gt = case()
    P = s["points"]
    q, t = torch.from_numpy(gt).cuda(), torch.from_numpy(P).cuda()
    qm, tm = nc.random_mask(SHAPE, 1, keep=0.7), nc.random_mask(SHAPE, 2, keep=0.6)
    for kw, args in ((dict(), (None, None, None)), (dict(max_distance=0.3), (0.3, None, None)),
                     (dict(query_mask=torch.from_numpy(qm).cuda(), target_mask=torch.from_numpy(tm != 0).cuda()), (None, qm, tm))):
        out = nearest_points(q, t, **kw)                                                             # [N,H,W,3] on both sides: flattened
        want = nc.rule(gt, P, *args)
        assert set(out) == {"index", "sq_distance", "distance"} and all(v.is_cuda and tuple(v.shape) == (7770,) for v in out.values())
        assert (out["index"].dtype, out["sq_distance"].dtype, out["distance"].dtype) == (torch.int32, torch.float32, torch.float32)
        assert np.array_equal(out["index"].cpu().numpy(), want["index"])
        sq = out["sq_distance"].cpu().numpy()
        assert np.array_equal(sq.view(np.int32), want["sq_distance"].view(np.int32))
        d, root = out["distance"].cpu().numpy(), np.sqrt(sq)
        fin = np.isfinite(root)
        assert (np.abs(d[fin].view(np.int32) - root[fin].view(np.int32)) <= 1).all() and np.isinf(d[~fin]).all()   # one fp32 ulp
    out = nearest_points(q.double(), t.half())                                                       # other float dtypes are cast to fp32
    assert np.array_equal(out["index"].cpu().numpy(), nc.rule(gt, P.astype(np.float16).astype(np.float32))["index"])


def test_evaluate_reconstruction_with_sim3_alignment_equals_numpy():
    s, pred, gt = case()
    snap = {k: v.clone() for k, v in pred.items() if torch.is_tensor(v)}                            # fp32, NaN included: compared as bits
    P = pred["points"][0].cpu().numpy()
    out = evaluate_reconstruction(pred, torch.from_numpy(gt), thresholds=THRESHOLDS, return_distances=True)
    both = np.isfinite(P).all(-1) & np.isfinite(gt).all(-1)
    ws, wR, wt = nc.umeyama(P[both], gt[both])
    M = out["transform"].numpy()
    assert out["transform"].dtype == torch.float64 and np.abs(M - nc.transform_of(ws, wR, wt)).max() <= 1e-9 * np.abs(M).max()
    assert abs(ws - 1.4) < 0.01                                                                      # the planted scale comes back
    aligned = nc.apply_transform(M, P.reshape(-1, 3))
    keep = np.isfinite(aligned).all(1)
    assert np.array_equal(out["pred_points"].cpu().numpy().view(np.int32), aligned[keep].view(np.int32))
    ref = nc.metrics(aligned, gt.reshape(-1, 3), THRESHOLDS)
    check_metrics(out, ref, THRESHOLDS)
    assert ref["n_pred"] == 7770 - 15 and ref["n_gt"] == 7770 - 40
    assert np.array_equal(out["accuracy_distances"].cpu().numpy(), ref["accuracy_distances"])
    assert np.array_equal(out["completeness_distances"].cpu().numpy(), ref["completeness_distances"])
    assert 0.002 < out["accuracy"] < 0.02 and 0 < out["precision"][0] < out["precision"][1] <= out["precision"][2] and out["precision"][2] > 0.9
    assert all(torch.equal(pred[k].view(torch.int32), v.view(torch.int32)) for k, v in snap.items())   # the inputs are untouched
    plain = evaluate_reconstruction(pred, torch.from_numpy(gt).cuda()[None], thresholds=THRESHOLDS)  # [1,N,H,W,3], on the device
    assert "pred_points" not in plain and plain["accuracy"] == out["accuracy"] and plain["fscore"] == out["fscore"]
    assert len(format_evaluation(plain)) == 4 + len(THRESHOLDS)


def test_alignment_none_an_explicit_transform_and_an_unordered_cloud():
    s, pred, gt = case()
    P = pred["points"][0].cpu().numpy().reshape(-1, 3)
    cloud = gt.reshape(-1, 3)[np.random.default_rng(3).permutation(7770)[:5000]]                     # unordered: no correspondences
    M = nc.transform_of(*nc.similarity(seed=7, scale=1.4))                                           # the planted one itself
    for align, moved in (("none", P), (torch.from_numpy(M), nc.apply_transform(M, P)), (M.astype(np.float32), None)):
        out = evaluate_reconstruction(pred, torch.from_numpy(cloud), align=align, thresholds=THRESHOLDS)
        if moved is None:
            moved = nc.apply_transform(M.astype(np.float32).astype(np.float64), P)
        check_metrics(out, nc.metrics(moved, cloud, THRESHOLDS), THRESHOLDS)
        want = np.eye(4) if isinstance(align, str) else np.asarray(align, np.float64)
        assert np.array_equal(out["transform"].numpy(), want)
    assert out["accuracy"] < 0.25 * evaluate_reconstruction(pred, torch.from_numpy(cloud), align="none")["accuracy"]
    # the pixel-aligned form with align="none" is the same computation on the flattened grid; a ground-truth mask drops points
    gm = nc.random_mask(SHAPE, 5, keep=0.8)
    out = evaluate_reconstruction(pred, torch.from_numpy(gt), gt_mask=torch.from_numpy(gm != 0), align="none", thresholds=THRESHOLDS)
    check_metrics(out, nc.metrics(P, gt.reshape(-1, 3), THRESHOLDS, gt_mask=gm), THRESHOLDS)
    out = evaluate_reconstruction(pred, torch.from_numpy(cloud), gt_mask=torch.from_numpy(gm.reshape(-1)[:5000]), align="none")
    check_metrics(out, nc.metrics(P, cloud, (0.05,), gt_mask=gm.reshape(-1)[:5000]), (0.05,))


def test_max_distance_clips_the_means_and_counts_misses():
    s, pred, gt = case()
    P = pred["points"][0].cpu().numpy()
    free = evaluate_reconstruction(pred, torch.from_numpy(gt), thresholds=THRESHOLDS, return_distances=True)
    M = free["transform"].numpy()
    aligned = nc.apply_transform(M, P.reshape(-1, 3))
    lim = float(np.median(free["accuracy_distances"].cpu().numpy()))
    out = evaluate_reconstruction(pred, torch.from_numpy(gt), thresholds=THRESHOLDS + (10.0,), max_distance=lim, return_distances=True)
    ref = nc.metrics(aligned, gt.reshape(-1, 3), THRESHOLDS + (10.0,), max_distance=lim)
    check_metrics(out, ref, THRESHOLDS + (10.0,))
    d = out["accuracy_distances"].cpu().numpy()
    assert d.max() == lim and 0.3 < (d == lim).mean() < 0.7 and out["accuracy"] < free["accuracy"]
    assert 0 < out["precision_hits"][3] < ref["n_pred"] and out["precision_hits"][3] >= int((d < lim).sum())   # a miss at every threshold


def test_filters_an_explicit_mask_and_an_empty_prediction():
    s, pred, gt = case()
    P = pred["points"][0].cpu().numpy()
    g = torch.from_numpy(gt)
    keep = point_cloud_mask(pred, edge_rtol=0.03)
    assert 0 < int(keep.sum()) < int(point_cloud_mask(pred).sum())
    by_filter = evaluate_reconstruction(pred, g, thresholds=THRESHOLDS, edge_rtol=0.03)
    for mask in (keep, keep.view(torch.uint8), keep[None]):
        by_mask = evaluate_reconstruction(pred, g, thresholds=THRESHOLDS, mask=mask)
        assert {k: v for k, v in by_mask.items() if k != "transform"} == {k: v for k, v in by_filter.items() if k != "transform"}
        assert torch.equal(by_mask["transform"], by_filter["transform"])
    k = keep.cpu().numpy()
    both = k & np.isfinite(P).all(-1) & np.isfinite(gt).all(-1)
    M = by_filter["transform"].numpy()
    assert np.abs(M - nc.transform_of(*nc.umeyama(P[both], gt[both]))).max() <= 1e-9 * np.abs(M).max()
    check_metrics(by_filter, nc.metrics(nc.apply_transform(M, P.reshape(-1, 3)), gt.reshape(-1, 3), THRESHOLDS, pred_mask=k), THRESHOLDS)
    assert by_filter["n_pred"] == int((k & np.isfinite(P).all(-1)).sum())
    # an empty prediction: NaN on its side, no launch fault; with a limit the other side is clipped to it
    empty = torch.zeros_like(keep)
    out = evaluate_reconstruction(pred, g, align="none", mask=empty, max_distance=0.5)
    assert out["n_pred"] == 0 and np.isnan(out["accuracy"]) and np.isnan(out["chamfer"]) and np.isnan(out["precision"][0])
    assert out["completeness"] == 0.5 and out["recall"] == [0.0] and np.isnan(out["fscore"][0])
    assert np.isinf(evaluate_reconstruction(pred, g, align="none", mask=empty)["completeness"])
    with pytest.raises(ValueError):                                                                  # nothing to fit a similarity on
        evaluate_reconstruction(pred, g, mask=empty)
    none = evaluate_reconstruction(pred, torch.zeros(0, 3), align="none")
    assert none["n_gt"] == 0 and np.isnan(none["completeness"]) and np.isinf(none["accuracy"]) and none["precision"] == [0.0]


def test_inference_recon_prints_the_table(tiny_checkpoint, golden_dir, tmp_path, monkeypatch, capsys):
    from PIL import Image
    from safetensors.torch import load_file
    path, _, _ = tiny_checkpoint
    monkeypatch.chdir(tmp_path)
    g = load_file(os.path.join(golden_dir, "recon_real2_dl3dv_2v.safetensors"))
    folder = tmp_path / "frames"
    folder.mkdir()
    for i, name in enumerate(("a_first.png", "b_second.png")):
        Image.fromarray(g["inp.images_u8"][i].permute(1, 2, 0).numpy()).save(folder / name)
    import inference_recon
    args = ["--image_folder", str(folder), "--model_path", path]
    pred = inference_recon.main(args + ["--save_path", str(tmp_path / "plain.ply")])
    assert "evaluation" not in pred and "accuracy" not in capsys.readouterr().out                    # off by default
    points = pred["points"][0].float().cpu().numpy()
    gt = nc.moved(points, seed=2, scale=0.7, noise=1e-3 * float(np.nanstd(points)))
    np.save(tmp_path / "gt.npy", gt)
    np.save(tmp_path / "cloud.npy", gt.reshape(-1, 3)[::3])
    pred = inference_recon.main(args + ["--save_path", str(tmp_path / "e.ply"), "--evaluate", str(tmp_path / "gt.npy"), "--eval-threshold",
                                        "0.01", "--eval-threshold", "0.1"])
    printed = capsys.readouterr().out
    assert (tmp_path / "e.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()              # the export is unchanged
    want = evaluate_reconstruction(pred, torch.from_numpy(gt), thresholds=(0.01, 0.1), mask=point_cloud_mask(pred))
    assert pred["evaluation"]["accuracy"] == want["accuracy"] and pred["evaluation"]["fscore"] == want["fscore"]
    for line in format_evaluation(want):
        assert line in printed
    assert "align sim3" in printed and abs(np.linalg.det(want["transform"].numpy()[:3, :3]) - 0.7 ** 3) < 0.01
    pred = inference_recon.main(args + ["--save_path", str(tmp_path / "c.ply"), "--evaluate", str(tmp_path / "cloud.npy"),
                                        "--eval-max-distance", "0.5"])
    printed = capsys.readouterr().out
    assert "align none" in printed and pred["evaluation"]["thresholds"] == (0.05,) and pred["evaluation"]["n_gt"] == len(gt.reshape(-1, 3)[::3])
    assert pred["evaluation"]["accuracy"] <= 0.5
