"""Time the exact nearest-neighbour search (g2v_cloud_nn: csrc/nn.hip) and evaluate_reconstruction on the synthetic floor-and-sphere
scene of tests/consistency_check.py: N views of 518 x 518, the prediction (moved by the planted similarity) against a
similarity-moved, noised copy of itself.  Needs the GPU; bench.py is a different measurement and is not touched.

    python tools/bench_nn.py [--views 8 32] [--out profiles/nn_bench.json]

  default, grid  device events around single calls of the entry point (outputs and workspace allocated once), all queries against all
                 targets, under the default dispatch and with G2V_NN_GRID; the two must agree byte for byte
  subset         the same for a strided subset of the queries against all targets, on the grid path, the brute path and the same
                 rule in torch on the same device - chunks of queries, broadcast subtract, square, sum, argmin -; grid and brute
                 must agree byte for byte before anything is timed, and the share of queries on which torch picks the same index is
                 recorded (ties may resolve differently)
  evaluate       the whole evaluate_reconstruction under the default dispatch (mask, Umeyama fit, transform, two searches,
                 metrics): host clock around the call, which ends in read-backs
  sweep          brute against grid over Nt at two query counts: where the default dispatch should switch

Calls: the first call of anything is timed; 30 calls after 5 warm-ups where one call takes under 0.1 s, otherwise as many calls (30 at
most) after that first one as fit into BUDGET_S seconds; where not even one fits, the first call is the figure (runs = 1, warm_ups =
0).  Every dict says how many runs and warm-ups it had.  The JSON is rewritten after the sweep and after every configuration."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nn_check as nc  # noqa: E402
from g2vlm_amd import hip  # noqa: E402
from g2vlm_amd.g2vlm_utils import evaluate_reconstruction  # noqa: E402

H = W = 518
LAUNCHES, WARM = 30, 5
BUDGET_S = 15.0                                               # seconds of measured calls for anything that takes 0.1 s or more per call
SUBSET = 16384                                                # queries of the subset runs
TORCH_PAIRS = 1 << 28                                         # pairs per chunk of the torch form: 3 GiB of fp32 differences
SWEEP_NT = (256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072)
SWEEP_NQ = (7770, 268324)


def percentiles(ms):
    ms = sorted(ms)
    return dict(median_ms=round(statistics.median(ms), 4), p10_ms=round(ms[len(ms) // 10], 4), p90_ms=round(ms[(len(ms) * 9) // 10], 4), runs=len(ms))


def one_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def plan(first_ms):
    """(further warm-ups, measured calls) after a first call of first_ms"""
    if first_ms < 100.0:
        return WARM - 1, LAUNCHES
    return 0, min(LAUNCHES, int(BUDGET_S * 1e3 / first_ms))


def event_times(fn):
    first = one_call(fn)
    warm, launches = plan(first)
    if launches == 0:
        return dict(median_ms=round(first, 4), p10_ms=round(first, 4), p90_ms=round(first, 4), runs=1, warm_ups=0)
    for _ in range(warm):
        one_call(fn)
    out = percentiles([one_call(fn) for _ in range(launches)])
    out["warm_ups"] = warm + 1
    return out


class Search:
    """preallocated outputs and workspace of one (queries, targets) pair"""

    def __init__(self, Q, T):
        self.Q, self.T = Q, T
        n = Q.shape[0]
        self.index = torch.empty(n, dtype=torch.int32, device="cuda")
        self.sq = torch.empty(n, dtype=torch.float32, device="cuda")
        self.stats = torch.empty(4, dtype=torch.int32, device="cuda")
        self.ws = torch.empty((hip.cloud_nn_workspace(n, T.shape[0]) + 7) // 8, dtype=torch.int64, device="cuda")

    def run(self, flags, max_distance=None):
        hip.cloud_nn_raw(self.Q, None, self.T, None, max_distance, flags, self.index, self.sq, self.stats, workspace=self.ws)

    def result(self, flags):
        self.run(flags)
        torch.cuda.synchronize()
        return self.index.clone(), self.sq.clone(), self.stats.tolist()


def torch_nn(Q, T):
    """the rule's nearest neighbour in torch: chunks of queries, the squared distances by broadcast subtract, square and sum (separate
    kernels, so nothing fuses: the rule's own numbers), argmin; non-finite targets are moved far away first so that they never win.
    (torch.cdist is not used: in a first run of this tool its argmin agreed with the rule on 3 % of the queries at 2.1 M targets.)"""
    Tc = torch.where(torch.isfinite(T).all(1, keepdim=True), T, torch.full_like(T, 1e18))
    step = max(1, TORCH_PAIRS // max(1, T.shape[0]))
    out = torch.empty(Q.shape[0], dtype=torch.int64, device=Q.device)
    for a in range(0, Q.shape[0], step):
        d = Q[a:a + step, None, :] - Tc[None, :, :]
        out[a:a + step] = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).argmin(1)
    return out


def bench_views(n):
    s = nc.scene(n, H, W)
    P = s["points"].reshape(-1, 3)
    del s["local"]
    M = nc.transform_of(*nc.similarity(seed=7, scale=1.4))
    gt = nc.moved(P, seed=7, scale=1.4, noise=0.004)
    Q, T = torch.from_numpy(nc.apply_transform(M, P)).cuda(), torch.from_numpy(gt).cuda()          # the aligned prediction, the ground truth
    res = dict(config=f"{n}v", views=n, height=H, width=W, queries=int(Q.shape[0]), targets=int(T.shape[0]),
               cells_per_axis=int(round((hip.cloud_nn_workspace(0, T.shape[0]) - 256 - 24 * T.shape[0]) ** (1 / 3) / 4 ** (1 / 3))))
    full = Search(Q, T)
    index, sq, stats = full.result(0)
    g_index, g_sq, g_stats = full.result(hip.NN_GRID)
    if not (torch.equal(index, g_index) and torch.equal(sq.view(torch.int32), g_sq.view(torch.int32)) and stats == g_stats):
        raise SystemExit(f"{res['config']}: the default dispatch and the grid path differ")
    del g_index, g_sq
    res.update(participating_queries=stats[0], participating_targets=stats[1], default_equals_grid=True,
               median_distance=float(sq[index >= 0].double().sqrt().median()))
    res["default"] = event_times(lambda: full.run(0))
    res["default"]["pairs_per_s"] = round(stats[0] * stats[1] / res["default"]["median_ms"] * 1e3)
    res["grid"] = event_times(lambda: full.run(hip.NN_GRID))
    res["default_over_grid"] = round(res["default"]["median_ms"] / res["grid"]["median_ms"], 2)
    print(res, file=sys.stderr, flush=True)

    stride = Q.shape[0] // SUBSET
    Qs = Q[::stride][:SUBSET].contiguous()
    sub = Search(Qs, T)
    g, b = sub.result(hip.NN_GRID), sub.result(hip.NN_BRUTE)
    if not (torch.equal(g[0], b[0]) and torch.equal(g[1].view(torch.int32), b[1].view(torch.int32)) and g[2] == b[2]):
        raise SystemExit(f"{res['config']}: the grid and the brute path differ")
    if not (torch.equal(g[0], index[::stride][:SUBSET]) and torch.equal(g[1].view(torch.int32), sq[::stride][:SUBSET].view(torch.int32))):
        raise SystemExit(f"{res['config']}: the subset run and the full run differ")
    tn = torch_nn(Qs, T)
    ok = g[0] >= 0
    same = float((tn[ok] == g[0][ok].long()).double().mean())
    if same < 0.999:
        raise SystemExit(f"{res['config']}: torch picks the same index on {same:.4%} of the queries only")
    subset = dict(queries=int(Qs.shape[0]), targets=int(T.shape[0]), grid_equals_brute=True, torch_same_index_share=round(same, 6))
    subset["brute"] = event_times(lambda: sub.run(hip.NN_BRUTE))
    subset["grid"] = event_times(lambda: sub.run(hip.NN_GRID))
    subset["torch_form"] = event_times(lambda: torch_nn(Qs, T))
    subset["brute_over_grid"] = round(subset["brute"]["median_ms"] / subset["grid"]["median_ms"], 3)
    subset["torch_over_grid"] = round(subset["torch_form"]["median_ms"] / subset["grid"]["median_ms"], 2)
    subset["torch_over_brute"] = round(subset["torch_form"]["median_ms"] / subset["brute"]["median_ms"], 2)
    subset["brute_pairs_per_s"] = round(int(ok.sum()) * stats[1] / subset["brute"]["median_ms"] * 1e3)
    res["subset"] = subset
    print(subset, file=sys.stderr, flush=True)
    del full, sub, tn, index, sq

    pts = torch.from_numpy(P.reshape(n, H, W, 3)).cuda()[None]
    pred = dict(points=pts, local_points=pts, conf=None, images=None)                               # no edge filter: the depth is not read
    gt_dev = T.view(n, H, W, 3)

    def evaluate():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = evaluate_reconstruction(pred, gt_dev, thresholds=(0.01, 0.05))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out
    first, out = evaluate()
    rounds = min(5, int(BUDGET_S * 1e3 / first))
    times = [evaluate()[0] for _ in range(rounds)] or [first]
    res["evaluate_reconstruction"] = dict(median_ms=round(statistics.median(times), 3), min_ms=round(min(times), 3), max_ms=round(max(times), 3),
                                          rounds=len(times), warm_ups=1 if rounds else 0, accuracy=out["accuracy"],
                                          completeness=out["completeness"], fscore=out["fscore"], n_pred=out["n_pred"], n_gt=out["n_gt"])
    print(res["evaluate_reconstruction"], file=sys.stderr, flush=True)
    return res


def sweep():
    s = nc.scene(8, H, W)
    P = s["points"].reshape(-1, 3)
    P = P[np.isfinite(P).all(1)]
    G = nc.moved(P, seed=7, scale=1.0, noise=0.004)
    _, R, t = nc.similarity(7, 1.0)
    G = ((G.astype(np.float64) - t) @ R).astype(np.float32)
    rows = []
    for nq in SWEEP_NQ:
        Q = torch.from_numpy(G[::len(G) // nq][:nq].copy()).cuda()
        for nt in SWEEP_NT:
            T = torch.from_numpy(P[::len(P) // nt][:nt].copy()).cuda()
            run = Search(Q, T)
            g, b = run.result(hip.NN_GRID), run.result(hip.NN_BRUTE)
            if not (torch.equal(g[0], b[0]) and torch.equal(g[1].view(torch.int32), b[1].view(torch.int32))):
                raise SystemExit(f"sweep Nq {nq} Nt {nt}: the grid and the brute path differ")
            row = dict(queries=nq, targets=nt, brute=event_times(lambda: run.run(hip.NN_BRUTE)), grid=event_times(lambda: run.run(hip.NN_GRID)))
            row["brute_over_grid"] = round(row["brute"]["median_ms"] / row["grid"]["median_ms"], 2)
            rows.append(row)
            print(row, file=sys.stderr, flush=True)
    cross = {}
    for nq in SWEEP_NQ:
        faster = [r["targets"] for r in rows if r["queries"] == nq and r["brute_over_grid"] > 1.0]
        cross[str(nq)] = min(faster) if faster else None                                            # the smallest Nt at which the grid wins
    return dict(rows=rows, grid_faster_from_targets=cross)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_nn.py measures on the GPU; there is none here")
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0]
    res = dict(what="exact nearest neighbour between two clouds: g2v_cloud_nn's grid and brute paths vs the same rule in chunked torch; "
                    "evaluate_reconstruction", measured_on="1x MI355X (gfx950)" if arch == "gfx950" else "1x " + torch.cuda.get_device_name(0),
               arch=arch, library=os.path.basename(hip.LIB_PATH),
               method=f"device events around one call: {LAUNCHES} calls after {WARM} warm-ups where a call takes under 0.1 s, otherwise as many "
                      f"calls (at most {LAUNCHES}) after the first as fit into {BUDGET_S:g} s, or the first call alone where none fits (every "
                      "entry records its runs and warm-ups); evaluate_reconstruction: host clock around a call that ends in read-backs, up "
                      "to 5 rounds by the same budget", configs=[])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def write():
        with open(a.out + ".tmp", "w") as fh:
            json.dump(res, fh, indent=1)
        os.replace(a.out + ".tmp", a.out)
    if not a.no_sweep:
        res["sweep"] = sweep()
        write()
    for n in a.views:
        res["configs"].append(bench_views(n))
        write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
