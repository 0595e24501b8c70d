"""GPU: g2v_cloud_nn (csrc/nn.hip) against the fp32 rule of tests/nn_check.py, byte for byte, on index, sq_distance and stats: both
forced paths and the default dispatch at every size class under every mask and distance limit, target sets built against the grid
(degenerate boxes, ties, far queries, overflow, a set that a fused multiply-add would change), one large case, canaries around the
outputs, empty sides, determinism and graph capture."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import nn_check as nc  # noqa: E402
from g2vlm_amd import hip  # noqa: E402

pytestmark = pytest.mark.gpu
# targets: one (a box of zero extent, one cell); two (G = 1); one short of a wave, a wave, one past it (G = 5: 125 cells, one scan
# block); one LDS tile of the brute path, one past it (two tiles, two target slices; G = 12: 1 728 cells, two scan blocks); 7 770
# (G = 24: 13 824 cells, 14 scan blocks, 8 tiles).  The default dispatch has no threshold to cross: it is the brute path for every Nt
NT = [1, 2, 63, 64, 65, 1024, 1025, 7770]
# queries: one; one past a wave (one workgroup, most lanes idle); 31 workgroups of 256, the last one partial
NQ = [1, 65, 7770]
PATHS = {"brute": hip.NN_BRUTE, "grid": hip.NN_GRID, "default": 0}
MASKS = ["null", "ones", "keep50", "zero", "single"]
CANARY = 3


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def clouds(nq, nt):
    """(queries [nq,3], targets [nt,3]): the first nt finite points of the synthetic scene, and nq points of a noised copy of the
    whole scene (its NaN points included: queries that take no part)"""
    s = nc.scene(3, 37, 70, seed=nq % 7)
    P = s["points"].reshape(-1, 3)
    T = P[np.isfinite(P).all(1)]
    step = max(1, len(T) // nt)
    T = T[::step][:nt]
    assert len(T) == nt
    Q = nc.moved(P, seed=3, scale=1.0, noise=0.01)
    s_, R, t = nc.similarity(3, 1.0)
    Q = ((Q.astype(np.float64) - t) @ R).astype(np.float32)                                          # back onto the scene: neighbours are near
    Q = Q[::max(1, len(Q) // nq)][:nq].copy()
    assert len(Q) == nq
    if nq > 1:
        Q[5::97, 1] = np.nan                                                                         # queries that take no part
    return Q, T


def mask_of(n, name, seed):
    if name == "null":
        return None
    if name == "ones":
        return np.full(n, 255, np.uint8)                                                             # any non-zero byte keeps
    if name == "keep50":
        return nc.random_mask(n, seed, keep=0.5)
    if name == "zero":
        return np.zeros(n, np.uint8)
    m = np.zeros(n, np.uint8)
    m[(n * 2) // 3] = 1
    return m


def run(Q, T, max_distance=None, qmask=None, tmask=None, flags=0):
    """the raw entry point into sentinel-filled outputs with CANARY rows before and after, from a junk-filled workspace"""
    nq, nt = len(Q), len(T)
    tQ, tT, tqm, ttm = dev(Q.reshape(-1, 3)), dev(T.reshape(-1, 3)), dev(qmask), dev(tmask)
    before = (tQ.clone(), tT.clone())
    index = torch.full((nq + 2 * CANARY,), -7, dtype=torch.int32, device="cuda")
    sq = torch.full((nq + 2 * CANARY,), -3.0, dtype=torch.float32, device="cuda")
    stats = torch.full((4 + 2 * CANARY,), -9, dtype=torch.int32, device="cuda")
    nbytes = hip.cloud_nn_workspace(nq, nt)
    assert nbytes > 0
    ws = torch.full(((nbytes + 7) // 8,), 0x0123456789ABCDEF, dtype=torch.int64, device="cuda")     # junk: needs no initialisation
    hip.cloud_nn_raw(tQ, tqm, tT, ttm, max_distance, flags, index[CANARY:CANARY + nq], sq[CANARY:CANARY + nq], stats[CANARY:CANARY + 4],
                     workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(tQ.view(torch.int32), before[0].view(torch.int32)) and torch.equal(tT.view(torch.int32), before[1].view(torch.int32))
    for t, sentinel in ((index, -7), (sq, -3.0), (stats, -9)):
        assert bool((t[:CANARY] == sentinel).all()) and bool((t[-CANARY:] == sentinel).all())        # nothing outside the outputs
    return dict(index=index[CANARY:CANARY + nq].cpu().numpy(), sq_distance=sq[CANARY:CANARY + nq].cpu().numpy(),
                stats=stats[CANARY:CANARY + 4].cpu().numpy())


def check(got, want, what=""):
    assert np.array_equal(got["stats"], want["stats"]), (what, got["stats"].tolist(), want["stats"].tolist())
    bad = np.flatnonzero(got["index"] != want["index"])
    assert bad.size == 0, (what, bad[:5].tolist(), got["index"][bad[:5]].tolist(), want["index"][bad[:5]].tolist())
    assert np.array_equal(got["sq_distance"].view(np.int32), want["sq_distance"].view(np.int32)), what


def all_paths(Q, T, max_distance=None, qmask=None, tmask=None, what="", want=None):
    """the rule's result (computed here unless given) after every path's outputs were found equal to it"""
    if want is None:
        want = nc.rule(Q, T, max_distance, qmask, tmask)
    for name, flags in PATHS.items():
        check(run(Q, T, max_distance, qmask, tmask, flags), want, (what, name))
    return want


@functools.lru_cache(maxsize=None)
def want_of(nq, nt, max_distance):
    """the rule on clouds(nq, nt) without masks: computed once, shared, never written to"""
    return nc.rule(*clouds(nq, nt), max_distance)


@functools.lru_cache(maxsize=None)
def limits_of(nq, nt):
    """(the median neighbour distance, a distance whose fp32 square equals some neighbour's d2 bit for bit - or None -, a distance
    below every neighbour's)"""
    Q, T = clouds(nq, nt)
    r = want_of(nq, nt, None)
    d2 = r["sq_distance"][r["index"] >= 0]
    median = float(np.sqrt(np.median(d2)))
    cand = np.unique(d2)
    root = np.sqrt(cand)
    exact = None
    for delta in (0, 1, -1):
        L = (root.view(np.int32) + delta).view(np.float32)
        hit = np.flatnonzero(L * L == cand)
        if hit.size:
            exact = float(L[hit[len(hit) // 2]])
            break
    return median, exact, float(np.sqrt(d2.min())) * 0.5


@pytest.mark.parametrize("nq", NQ)
@pytest.mark.parametrize("nt", NT)
def test_kernel_equals_the_rule_byte_for_byte(nt, nq):
    Q, T = clouds(nq, nt)
    median, exact, below = limits_of(nq, nt)
    assert exact is not None or nq == 1                                                              # a single distance may have no exact root
    for max_distance in (None, median, below) + (() if exact is None else (exact,)):
        want = all_paths(Q, T, max_distance, what=max_distance, want=want_of(nq, nt, max_distance))
        found = int(want["stats"][3])
        print(f"Nq {nq} Nt {nt} max_distance {max_distance}: {found} of {int(want['stats'][0])} participating queries have a neighbour")
        if max_distance is None:
            assert found == want["stats"][0] > 0 or nq == 1
        elif max_distance == below:
            assert found == 0
        elif max_distance == exact:
            lim = np.float32(exact) * np.float32(exact)
            assert (want["sq_distance"] == lim).any()                                                # equality with the limit counts
    if exact is not None:                                                                            # `<` in place of `<=` would lose one
        less = nc.rule(Q, T, float(np.nextafter(np.float32(exact), np.float32(0))))
        assert less["stats"][3] < want_of(nq, nt, exact)["stats"][3]


@pytest.mark.parametrize("tmask_name", MASKS)
@pytest.mark.parametrize("qmask_name", MASKS)
def test_masks_on_both_sides(qmask_name, tmask_name):
    for nq, nt in ((65, 65), (7770, 1025), (2000, 7770)):
        Q, T = clouds(nq, nt)
        qm, tm = mask_of(nq, qmask_name, 11), mask_of(nt, tmask_name, 12)
        median = limits_of(nq, nt)[0]
        for max_distance in (None, median):
            want = all_paths(Q, T, max_distance, qm, tm, (qmask_name, tmask_name, nq, nt))
            if tmask_name == "zero" or qmask_name == "zero":
                assert want["stats"][3] == 0 and (want["index"] == -1).all()
            if tmask_name == "single" and max_distance is None:
                assert set(want["index"].tolist()) <= {-1, (nt * 2) // 3}
    Q, T = clouds(65, 65)
    want = nc.rule(Q, T, None, mask_of(65, "keep50", 11), mask_of(65, "keep50", 12))
    for as_bool in (False, True):                                                                    # the wrapper takes bool masks too
        qm, tm = dev(mask_of(65, "keep50", 11)), dev(mask_of(65, "keep50", 12))
        if as_bool:
            qm, tm = qm.view(torch.bool), tm.view(torch.bool)
        index, sq, stats = hip.cloud_nn(dev(Q), dev(T), None, qm, tm)
        check(dict(index=index.cpu().numpy(), sq_distance=sq.cpu().numpy(), stats=stats.cpu().numpy()), want)


def test_degenerate_boxes():
    """all targets identical, on a line, on a plane (three, two and one axis of zero extent), one target (three), and a box whose extents
    differ by 1e6 between the axes (none)"""
    rng = np.random.default_rng(5)
    Q = rng.uniform(-2, 2, (700, 3)).astype(np.float32)
    same = np.tile(np.array([[0.3, -1.2, 0.7]], np.float32), (500, 1))
    line = np.zeros((3000, 3), np.float32)
    line[:, 1] = rng.uniform(-1, 1, 3000)
    plane = rng.uniform(-1, 1, (3000, 3)).astype(np.float32)
    plane[:, 2] = 0.25
    thin = rng.uniform(-1, 1, (3000, 3)).astype(np.float32) * np.array([1, 1e-6, 1e-3], np.float32)
    for name, T in (("same", same), ("line", line), ("plane", plane), ("one", same[:1]), ("thin", thin)):
        want = all_paths(Q, T, what=name)
        assert (want["index"] >= 0).all()
        if name == "same":
            assert (want["index"] == 0).all()                                                        # 500 equal keys but for the index
        all_paths(Q, T, 1.5, what=name)
        k = min(200, len(T))
        on = np.concatenate([T[:k], Q[:50]])                                                         # queries on the targets themselves
        assert (all_paths(on, T, what=name)["sq_distance"][:k] == 0).all()


def test_the_lattice_with_queries_on_cell_centres_and_cell_faces():
    T = nc.lattice(4)
    centres = nc.lattice(3) + np.float32(0.5)                                                        # eight targets at 0.75 exactly
    faces = nc.lattice(3) + np.array([0.5, 0.5, 0.0], np.float32)                                    # four targets at 0.5 exactly
    want = all_paths(centres, T)
    assert (want["sq_distance"] == 0.75).all()
    assert np.array_equal(want["index"], ((centres[:, 0] - 0.5) + 4 * (centres[:, 1] - 0.5) + 16 * (centres[:, 2] - 0.5)).astype(np.int32))
    want = all_paths(faces, T)
    assert (want["sq_distance"] == 0.5).all() and np.array_equal(want["index"], (faces[:, 0] - 0.5 + 4 * (faces[:, 1] - 0.5) + 16 * faces[:, 2]).astype(np.int32))
    big = nc.lattice(20)                                                                             # 8 000 targets: the grid's cells cut the lattice
    c = nc.lattice(19)[::7] + np.float32(0.5)
    want = all_paths(c, big)
    assert (want["sq_distance"] == 0.75).all()
    assert np.array_equal(want["index"], ((c[:, 0] - 0.5) + 20 * (c[:, 1] - 0.5) + 400 * (c[:, 2] - 0.5)).astype(np.int32))
    perm = np.random.default_rng(2).permutation(len(big))
    all_paths(c, big[perm])                                                                          # ties to the lowest index, wherever it lies
    all_paths(c, big, float(np.sqrt(np.float32(0.75))))
    all_paths(c, np.concatenate([big, big[::-1]]))                                                   # every target twice


def test_queries_far_outside_the_box_and_overflow():
    Q, T = clouds(65, 7770)
    Q = Q[np.isfinite(Q).all(1)]
    ext = float(np.ptp(T, axis=0).max())
    far = np.concatenate([Q[:20] + np.float32(1e6 * ext), Q[:20] * np.array([1, 1, -1e6], np.float32), Q[:20] + np.float32(3 * ext), Q[:10]])
    want = all_paths(far, T, what="far")
    assert (want["index"] >= 0).all()
    all_paths(far, T, 10 * ext, what="far, limited")
    big = np.float32(1e20)
    Qo = np.array([[1, 1, 1], [-1, 0, 0], [0, 0, 0], [1, -1, 0]], np.float32) * big
    To = np.array([[-1, -1, -1], [-1, 1, -1], [1, -1, 1]], np.float32) * big
    To = np.concatenate([To, (np.random.default_rng(3).choice([-2, 2], (3000, 3)) * big).astype(np.float32)])   # every difference >= 1e20
    want = all_paths(Qo, To, what="overflow")
    assert np.isinf(want["sq_distance"]).all() and want["index"].tolist() == [0, 0, 0, 0]
    tm = np.ones(len(To), np.uint8)
    tm[:2] = 0
    assert all_paths(Qo, To, None, None, tm, "overflow, masked")["index"][0] == 2                    # the lowest PARTICIPATING index
    assert (all_paths(Qo, To, 1e19, what="overflow, limited")["index"][:2] == -1).all()
    wide = np.array([[3e38, 0, 0], [-3e38, 0, 0], [0, 3e38, -3e38]], np.float32)                     # the differences overflow, not the inputs
    all_paths(np.concatenate([wide, Qo]), np.concatenate([wide[::-1], To[:100]]), what="wide")


def test_a_set_that_a_fused_sum_of_squares_would_change():
    Q, T = nc.fma_set()
    want = all_paths(Q, T)
    assert np.array_equal(want["index"], np.arange(len(Q), dtype=np.int32))
    for name, flags in PATHS.items():
        got = run(Q, T, None, None, None, flags)
        for form in nc.FUSED:
            fused = nc.sq_dist(Q, T, form)
            differ = fused.view(np.int32) != want["sq_distance"].view(np.int32)
            assert differ.sum() >= 8, form
            assert (got["sq_distance"].view(np.int32) != fused.view(np.int32))[differ].all(), (name, form)


def test_the_scene_against_a_moved_copy_of_itself():
    s = nc.scene(3, 37, 70)
    P = s["points"].reshape(-1, 3)
    G = nc.moved(P, seed=1, scale=1.3, noise=0.003)                                                  # not aligned: most queries lie outside the box
    all_paths(P, G, what="moved")
    all_paths(G, P, 0.5, what="moved back")
    mask = nc.random_mask(len(P), 4, keep=0.7)
    all_paths(P, P, None, mask, 1 - mask, what="complement")                                         # no query is its own neighbour


@functools.lru_cache(maxsize=None)
def large_case():
    s = nc.scene(2, 518, 518, seed=2)
    P = s["points"].reshape(-1, 3)
    Q = nc.moved(P[:518 * 518], seed=3, scale=1.0, noise=0.004)                                      # the full first view
    _, R, t = nc.similarity(3, 1.0)
    Q = ((Q.astype(np.float64) - t) @ R).astype(np.float32)
    Q[7::1009, 2] = np.inf
    T = P[np.isfinite(P).all(1)][:300000].copy()                                                     # the first view and part of the second
    T[::1000] = np.nan                                                                               # some targets take no part
    assert len(T) == 300000
    return Q, T


@pytest.mark.parametrize("path", list(PATHS))
def test_one_large_case(path):
    """Nt = 300 000, Nq = 268 324, on each forced path and the default.  Grid: at most 84^3 = 592 704 cells, scanned in 579 blocks of
    1 024 - more than the 256 that one pass of the block-sum scan holds, so its carry is used.  Brute: 293 tiles for 1 049 query
    workgroups are more than one launch's 2^36 pairs (249 tiles), so the launches' merge by the atomic minimum is used."""
    flags = PATHS[path]
    Q, T = large_case()
    rng = np.random.default_rng(9)
    qpart = np.isfinite(Q).all(1)
    tpart = np.flatnonzero(np.isfinite(T).all(1))
    got = run(Q, T, None, None, None, flags)
    assert got["stats"].tolist() == [int(qpart.sum()), len(tpart), 0, int(qpart.sum())]
    assert (got["index"][~qpart] == -1).all() and np.isinf(got["sq_distance"][~qpart]).all()
    pick = rng.choice(np.flatnonzero(qpart), 256, replace=False)
    want, sub = large_rule()
    assert np.array_equal(got["index"][pick], want["index"]) and np.array_equal(got["sq_distance"][pick].view(np.int32), want["sq_distance"].view(np.int32))
    rows = np.flatnonzero(qpart)
    idx = got["index"][rows]
    assert (idx >= 0).all() and np.isfinite(T[idx]).all()
    with np.errstate(over="ignore"):
        own = nc.sq_dist(Q[rows], T[idx])
        assert np.array_equal(own.view(np.int32), got["sq_distance"][rows].view(np.int32))           # the d2 to the returned index
        for _ in range(16):
            other = tpart[rng.integers(0, len(tpart), len(rows))]
            d2 = nc.sq_dist(Q[rows], T[other])
            assert ((own < d2) | ((own == d2) & (idx <= other))).all()
    limited = run(Q, T, 0.004, None, None, flags)
    assert np.array_equal(limited["index"][pick[:64]], sub["index"]) and 0 < limited["stats"][3] < limited["stats"][0]
    inside = got["sq_distance"] <= np.float32(0.004) * np.float32(0.004)
    assert np.array_equal(limited["index"], np.where(inside, got["index"], -1))


@functools.lru_cache(maxsize=None)
def large_rule():
    """the rule on the 256 queries that test_one_large_case picks (the same generator, the same draw): computed once, shared"""
    Q, T = large_case()
    pick = np.random.default_rng(9).choice(np.flatnonzero(np.isfinite(Q).all(1)), 256, replace=False)
    return nc.rule(Q[pick], T), nc.rule(Q[pick[:64]], T, 0.004)


def test_empty_sides():
    Q, T = clouds(65, 65)
    assert np.isfinite(Q).all(1).sum() == 64
    none = np.zeros((0, 3), np.float32)
    for name, flags in PATHS.items():
        got = run(Q, none, None, None, None, flags)
        check(got, nc.rule(Q, none), name)
        assert (got["index"] == -1).all() and np.isinf(got["sq_distance"]).all() and got["stats"].tolist() == [64, 0, 64, 0]
        got = run(none, T, 0.5, None, None, flags)
        assert got["index"].shape == (0,) and got["stats"].tolist() == [0, 65, 0, 0]
        assert run(none, none, None, None, None, flags)["stats"].tolist() == [0, 0, 0, 0]
    index, sq, stats = hip.cloud_nn(dev(none), dev(T))
    assert tuple(index.shape) == (0,) and tuple(sq.shape) == (0,) and stats.tolist() == [0, 65, 0, 0]


def test_two_runs_give_the_same_bytes_on_every_path():
    Q, T = clouds(7770, 7770)
    qm, tm = mask_of(7770, "keep50", 1), mask_of(7770, "keep50", 2)
    median = limits_of(7770, 7770)[0]
    runs = [run(Q, T, median, qm, tm, flags) for flags in list(PATHS.values()) * 2]
    for r in runs[1:]:
        assert all(np.array_equal(r[k].view(np.int32), runs[0][k].view(np.int32)) for k in ("index", "sq_distance", "stats"))


@pytest.mark.parametrize("path", list(PATHS))
def test_the_call_is_capturable_and_the_replay_equals_the_eager_run(path):
    Q, T = clouds(7770, 7770)
    qm = mask_of(7770, "keep50", 1)
    median = limits_of(7770, 7770)[0]
    want = nc.rule(Q, T, median, qm, None)
    tQ, tT, tqm = dev(Q), dev(T), dev(qm)

    def outputs():
        return dict(index=torch.full((7770,), -7, dtype=torch.int32, device="cuda"), sq_distance=torch.full((7770,), -3.0, device="cuda"),
                    stats=torch.full((4,), -9, dtype=torch.int32, device="cuda"))
    eager = outputs()
    hip.cloud_nn_raw(tQ, tqm, tT, None, median, PATHS[path], **eager)                                 # loads the code object, sizes the workspace
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    out = outputs()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):                                                                  # one stream, no parallel branches
        ws = torch.empty((hip.cloud_nn_workspace(7770, 7770) + 7) // 8, dtype=torch.int64, device="cuda")
        with torch.cuda.graph(g, stream=stream):
            hip.cloud_nn_raw(tQ, tqm, tT, None, median, PATHS[path], workspace=ws, **out)
    for _ in range(2):
        for o in out.values():
            o.fill_(9)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(out[k], eager[k]) for k in out)
        check({k: v.cpu().numpy() for k, v in out.items()}, want)
