"""The nearest-neighbour rule that csrc/nn.hip is held to (include/g2vlm_hip.h and DESIGN.md 6p state it), restated in numpy as a
chunked brute force, with Umeyama's alignment and the reconstruction metrics in fp64.  Checker side only: nothing here is imported by
the product.  The scene is that of tests/consistency_check.py.

rule(...) evaluates the rule in the dtype it is given.  In float32 every ufunc call is one fp32 operation rounded once - separate
calls cannot fuse - which is what the kernel does with contraction switched off, so the two agree byte for byte.  In float64 the
same code is the yardstick for how much of the chosen index hangs on rounding."""
import numpy as np

from consistency_check import _fma, random_mask, scene  # noqa: F401  (re-exported for the tests)

FUSED = ("inner", "inner_swapped", "outer", "both", "both_swapped")   # the ways a compiler may contract (dx dx + dy dy) + dz dz
CHUNK = 1 << 22                                                # pairs per chunk of the brute force


def sq_dist(q, t, fused=None):
    """d = q - t; (d0 d0 + d1 d1) + d2 d2 as the rule has it, or - NOT the rule - with the sums contracted (fp32 only).
    q [...,3] and t [...,3] broadcast."""
    d0, d1, d2 = q[..., 0] - t[..., 0], q[..., 1] - t[..., 1], q[..., 2] - t[..., 2]
    if fused is None:
        return (d0 * d0 + d1 * d1) + d2 * d2
    inner = {"inner": lambda: _fma(d0, d0, d1 * d1), "inner_swapped": lambda: _fma(d1, d1, d0 * d0), "outer": lambda: d0 * d0 + d1 * d1,
             "both": lambda: _fma(d0, d0, d1 * d1), "both_swapped": lambda: _fma(d1, d1, d0 * d0)}[fused]()
    return inner + d2 * d2 if fused.startswith("inner") else _fma(d2, d2, inner)


def takes_part(points, mask):
    keep = np.ones(len(points), bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    return keep & np.isfinite(points).all(-1)


def rule(query, target, max_distance=None, query_mask=None, target_mask=None, dtype=np.float32, fused=None):
    """query fp32 [Nq,3], target fp32 [Nt,3], masks bool / uint8 or None, max_distance a number or None (no limit).
    Returns dict(index int32 [Nq], sq_distance dtype [Nq], stats int32 [4] = participating queries, participating targets, queries
    without / with a neighbour).  The answer is the minimum of the key (bits(d2) << 32) | index over the counting targets: the
    smallest d2, the lowest index among equals, and the lowest participating index where every d2 is +inf."""
    f = dtype
    assert fused is None or f is np.float32
    query, target = np.asarray(query, np.float32).reshape(-1, 3), np.asarray(target, np.float32).reshape(-1, 3)
    Nq = len(query)
    qpart, tpart = takes_part(query, query_mask), takes_part(target, target_mask)
    tsel = np.flatnonzero(tpart)
    T = target[tsel].astype(f)
    index = np.full(Nq, -1, np.int32)
    sq = np.full(Nq, np.inf, f)
    with np.errstate(over="ignore"):                                                        # a square that overflows is no limit
        m2 = None if max_distance is None else f(np.float32(max_distance)) * f(np.float32(max_distance))
    qsel = np.flatnonzero(qpart)
    if len(tsel) and len(qsel):
        step = max(1, CHUNK // len(tsel))
        with np.errstate(over="ignore"):
            for a in range(0, len(qsel), step):
                rows = qsel[a:a + step]
                d2 = sq_dist(query[rows].astype(f)[:, None, :], T[None, :, :], fused)      # never NaN: both sides are finite
                counts = np.ones(d2.shape, bool) if m2 is None else ~(d2 > m2)
                d = np.where(counts, d2, f(np.inf))
                best = d.argmin(1)                                                          # the first minimum: the lowest index
                val = d[np.arange(len(rows)), best]
                some = counts.any(1)
                allinf = some & np.isinf(val)                                               # +inf by overflow: the lowest counting index
                best[allinf] = counts[allinf].argmax(1)
                index[rows[some]] = tsel[best[some]]
                sq[rows[some]] = val[some]
    found = int((index >= 0).sum())
    stats = np.array([len(qsel), len(tsel), len(qsel) - found, found], np.int32)
    return dict(index=index, sq_distance=sq, stats=stats)


def gap64(query, target, target_mask=None):
    """fp64: (index of the nearest target, relative gap (second - best) / second of the squared distances) of every query; all
    queries and at least two participating targets assumed finite"""
    tsel = np.flatnonzero(takes_part(target, target_mask))
    T = target[tsel].astype(np.float64)
    idx, gap = np.empty(len(query), np.int64), np.empty(len(query))
    step = max(1, CHUNK // len(tsel))
    for a in range(0, len(query), step):
        d2 = sq_dist(query[a:a + step].astype(np.float64)[:, None, :], T[None, :, :])
        two = np.argpartition(d2, 1, axis=1)[:, :2]
        v = np.take_along_axis(d2, two, 1)
        first = np.where(v[:, 0] <= v[:, 1], 0, 1)
        lo, hi = v[np.arange(len(v)), first], v[np.arange(len(v)), 1 - first]
        idx[a:a + step] = tsel[two[np.arange(len(v)), first]]
        gap[a:a + step] = np.where(hi > 0, (hi - lo) / np.where(hi > 0, hi, 1), 0.0)
    return idx, gap


def similarity(seed=0, scale=1.7):
    """a planted similarity (scale, rotation [3,3], translation [3]) in fp64: a rotation about a generic axis"""
    rng = np.random.default_rng(seed)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    ang = 0.3 + 0.5 * rng.random()
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    return scale, R, rng.uniform(-1, 1, 3)


def moved(points, seed=0, scale=1.7, noise=0.004):
    """points [...,3] under similarity(seed, scale) plus Gaussian noise, fp32 (NaN stays NaN)"""
    s, R, t = similarity(seed, scale)
    rng = np.random.default_rng(100 + seed)
    out = s * (points.astype(np.float64) @ R.T) + t + noise * rng.standard_normal(points.shape)
    return out.astype(np.float32)


def umeyama(src, dst, with_scale=True):
    """Umeyama's closed form in fp64: (scale, R, t) minimising sum |dst - (s R src + t)|^2 over corresponding rows"""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    n = len(src)
    mu_s, mu_d = src.mean(0), dst.mean(0)
    xs, xd = src - mu_s, dst - mu_d
    cov = xd.T @ xs / n
    U, D, Vt = np.linalg.svd(cov)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    s = float((D * S).sum() / ((xs * xs).sum() / n)) if with_scale else 1.0
    t = mu_d - s * (R @ mu_s)
    return s, R, t


def transform_of(s, R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s * R, t
    return M


def apply_transform(M, points):
    """the product's way, op by op in fp64 and rounded to fp32 once: ((a0 x + a1 y) + a2 z) + t per row of the 4 x 4"""
    p = points.astype(np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([((M[k, 0] * x + M[k, 1] * y) + M[k, 2] * z) + M[k, 3] for k in range(3)], -1).astype(np.float32)


def metrics(pred, gt, thresholds=(0.05,), max_distance=None, pred_mask=None, gt_mask=None):
    """The reconstruction metrics in fp64 from rule(): distances are the fp64 square roots of the fp32 squared distances, clipped to
    max_distance where it is given (a point without a neighbour then has that distance); a point is a hit at threshold T iff it has a
    neighbour and its squared distance is <= T T (fp64 product)."""
    a = rule(pred, gt, max_distance, pred_mask, gt_mask)
    c = rule(gt, pred, max_distance, gt_mask, pred_mask)
    out = dict(n_pred=int(a["stats"][0]), n_gt=int(c["stats"][0]))
    part = dict(accuracy=takes_part(np.asarray(pred).reshape(-1, 3), pred_mask), completeness=takes_part(np.asarray(gt).reshape(-1, 3), gt_mask))
    hits = {}
    for name, r in (("accuracy", a), ("completeness", c)):
        sq = r["sq_distance"][part[name]].astype(np.float64)
        with np.errstate(invalid="ignore"):
            d = np.sqrt(sq)
            if max_distance is not None:
                d = np.minimum(d, float(max_distance))
            out[name] = float(d.mean()) if len(d) else float("nan")
            out[name + "_median"] = float(np.median(d)) if len(d) else float("nan")
        out[name + "_distances"] = d
        hits[name] = [int(((r["index"][part[name]] >= 0) & (sq <= float(T) * float(T))).sum()) for T in thresholds]
    out["chamfer"] = 0.5 * (out["accuracy"] + out["completeness"])
    out["hits"] = hits
    for k, T in enumerate(thresholds):
        p = hits["accuracy"][k] / out["n_pred"] if out["n_pred"] else float("nan")
        r = hits["completeness"][k] / out["n_gt"] if out["n_gt"] else float("nan")
        out[T] = dict(precision=p, recall=r, fscore=fscore(p, r))
    return out


def fscore(p, r):
    if np.isnan(p) or np.isnan(r):
        return float("nan")
    return 2 * p * r / (p + r) if p + r > 0 else 0.0


def lattice(n=4):
    """the n^3 integer lattice, fp32 [n^3,3], x fastest"""
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)


def fma_set(K=4000, keep=48, seed=23):
    """(queries, targets): K random pairs of which the set keeps, for every form of FUSED, `keep` on which that contraction would
    change a bit of d2; target k is far nearer to query k than any other target (the pairs sit on a coarse lattice), so the chosen
    sq_distance of query k IS that d2."""
    rng = np.random.default_rng(seed)
    base = (lattice(16)[rng.permutation(16 ** 3)[:K]] * 8).astype(np.float32)
    q = base + rng.uniform(-0.5, 0.5, (K, 3)).astype(np.float32)
    t = base + rng.uniform(-0.5, 0.5, (K, 3)).astype(np.float32)
    plain = sq_dist(q, t)
    take = np.zeros(K, bool)
    for form in FUSED:
        take[np.flatnonzero(sq_dist(q, t, form).view(np.int32) != plain.view(np.int32))[:keep]] = True
    return q[take], t[take]
