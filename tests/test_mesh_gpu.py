"""GPU: g2v_cloud_mesh (csrc/mesh.hip) against the fp32 rule of tests/mesh_check.py, byte for byte, on used, vertex_of, faces,
face_records, counts and - through g2v_cloud_compact with `used` as its mask - the vertex records: the synthetic scene at every
shape class under every mask, the stretch filter off and on, hand-built inputs for each branch of the rule, a scene that a fused
multiply-add would triangulate differently, a capacity below the face count, determinism and graph capture."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import mesh_check as mc  # noqa: E402
from g2vlm_amd import hip  # noqa: E402

pytestmark = pytest.mark.gpu
# the single quad; no quads; exactly one 32 x 8 tile; one past it in both directions; 3 x 3; the family's usual scene; more than one block
# of 1024 pixels per view and a width that is no multiple of anything; more blocks (524) than one pass of the scan holds (256)
SHAPES = [(1, 2, 2), (1, 1, 5), (1, 5, 1), (1, 8, 32), (1, 9, 33), (2, 3, 3), (3, 37, 70), (2, 65, 129), (2, 518, 518)]
MASKS = ["null", "ones", "keep50", "keep90", "checkerboard", "zero", "hole", "last_row_and_column", "depth_edge"]
CANARY_ROWS = 3


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def scene_of(shape):
    n = SHAPES.index(shape)
    s = mc.scene(*shape, seed=n)
    return s["points"], mc.scene_colors(*shape, seed=n), s["local"]


def mask_of(shape, name):
    N, H, W = shape
    if name == "null":
        return None
    if name == "ones":
        return np.ones(shape, np.uint8)
    if name in ("keep50", "keep90"):
        return mc.random_mask(shape, 300 + SHAPES.index(shape), keep=0.5 if name == "keep50" else 0.9)
    if name == "checkerboard":
        return mc.checkerboard(*shape)
    if name == "zero":
        return np.zeros(shape, np.uint8)
    if name == "hole":
        m = np.full(shape, 255, np.uint8)                                                           # any non-zero byte keeps
        m[N - 1, H // 2, W // 2] = 0
        return m
    if name == "last_row_and_column":
        m = np.zeros(shape, np.uint8)
        m[:, -1, :] = 1
        m[:, :, -1] = 1
        return m
    return mc.depth_edge_mask(scene_of(shape)[2])


@functools.lru_cache(maxsize=None)
def limits_of(shape):
    """(a max_edge under which about half of the scene's candidates fail, a max_edge whose fp32 square equals the squared length of
    one of the diagonals the scene's quads are cut along, bit for bit - or None where the search finds none)"""
    r = mc.rule(scene_of(shape)[0])
    longer = np.maximum(r["ea"], r["em"])
    longer = longer[np.isfinite(longer)]
    if longer.size == 0:
        return 1.0, None
    median = np.median(longer)
    cut = np.where(r["anti"], r["ea"], r["em"])                                                     # the diagonal a quad is cut along
    cand = np.unique(cut[np.isfinite(r["ea"]) & np.isfinite(r["em"])]).astype(np.float32)
    root = np.sqrt(cand)                                                                            # fp32
    exact = None
    for delta in (0, 1, -1):
        L = (root.view(np.int32) + delta).view(np.float32)
        hit = np.flatnonzero(L * L == cand)
        if hit.size:
            exact = float(L[hit[np.argmin(np.abs(cand[hit] - median))]])
            break
    return float(np.sqrt(median)), exact


def run(points, mask, max_edge, cap=None, outputs="uvfr", record_offset=0):
    """the raw entry point with exactly the optional outputs asked for - u(sed), v(ertex_of), f(aces), (face_)r(ecords) - into
    sentinel-filled tensors with CANARY_ROWS rows after the capacity, from a junk-filled workspace"""
    n, h, w = points.shape[:3]
    t_points, t_mask = dev(points), dev(mask)
    before = (t_points.clone(), None if t_mask is None else t_mask.clone())
    if cap is None:
        cap = 2 * n * (h - 1) * (w - 1)
    room = cap + CANARY_ROWS
    store = torch.full((room * 13 + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    out = dict(u=torch.full((n, h, w), 77, dtype=torch.uint8, device="cuda"), v=torch.full((n, h, w), -9, dtype=torch.int32, device="cuda"),
               f=torch.full((room, 3), -7, dtype=torch.int32, device="cuda"), r=store[record_offset:record_offset + room * 13].view(room, 13))
    counts = torch.full((n, 2), -3, dtype=torch.int32, device="cuda")
    nbytes = hip.cloud_mesh_workspace(n, h, w)
    assert nbytes > 0
    ws = torch.full(((nbytes + 7) // 8,), 0x0123456789ABCDEF, dtype=torch.int64, device="cuda")     # junk: needs no initialisation
    ptr = {k: hip._p(out[k]) if k in outputs else None for k in "uvfr"}
    rcode = hip.lib().g2v_cloud_mesh(hip._p(t_points), hip._p(t_mask), n, h, w, 0 if max_edge is None else hip.MESH_MAX_EDGE,
                                     float(max_edge or 0.0), ptr["u"], ptr["v"], ptr["f"], ptr["r"], cap, hip._p(counts), hip._p(ws), nbytes,
                                     hip._stream())
    assert rcode == 0
    torch.cuda.synchronize()
    assert torch.equal(t_points.view(torch.int32), before[0].view(torch.int32)) and (t_mask is None or torch.equal(t_mask, before[1]))
    for k, sentinel in (("u", 77), ("v", -9), ("f", -7), ("r", 0xEE)):
        if k not in outputs:
            assert bool((out[k] == sentinel).all()), k                                              # an output not asked for is not written
    assert bool((store[:record_offset] == 0xEE).all()) and bool((store[record_offset + room * 13:] == 0xEE).all())
    got = {k: out[k].cpu().numpy() for k in outputs}
    got["counts"], got["used_dev"], got["cap"] = counts.cpu().numpy(), out["u"], cap
    return got


def check(got, want):
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"].tolist(), want["counts"].tolist())   # the true numbers, whatever the capacity
    if "u" in got:
        assert np.array_equal(got["u"], want["used"]), int((got["u"] != want["used"]).sum())
    if "v" in got:
        assert np.array_equal(got["v"], want["vertex_of"]), int((got["v"] != want["vertex_of"]).sum())
    written = min(len(want["faces"]), got["cap"])
    if "f" in got:
        assert np.array_equal(got["f"][:written], want["faces"][:written]), int((got["f"][:written] != want["faces"][:written]).any(1).sum())
        assert (got["f"][written:] == -7).all()                                                     # nothing past the count or the capacity
    if "r" in got:
        assert np.array_equal(got["r"][:written], want["face_records"][:written])
        assert (got["r"][written:] == 0xEE).all()


def check_vertex_records(points, colors, got, want):
    """the vertex block: g2v_cloud_compact with the kernel's `used` as its mask, against the rule's used pixels"""
    records, per_view = hip.cloud_compact(dev(points), dev(colors), got["used_dev"])
    assert np.array_equal(records.cpu().numpy(), mc.vertex_records(points, colors, want["used"]))
    assert np.array_equal(per_view.cpu().numpy(), want["counts"][:, 0])


@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_rule_byte_for_byte(shape, mask_name):
    points, colors, _ = scene_of(shape)
    mask = mask_of(shape, mask_name)
    half, exact = limits_of(shape)
    quads = shape[0] * (shape[1] - 1) * (shape[2] - 1)
    for max_edge in (None, half) + (() if exact is None else (exact,)):
        want = mc.rule(points, mask, max_edge)
        got = run(points, mask, max_edge)
        check(got, want)
        check_vertex_records(points, colors, got, want)
        F = int(want["counts"][:, 1].sum())
        print(f"{shape} {mask_name} max_edge {max_edge}: {int(want['counts'][:, 0].sum())} vertices, {F} faces of {2 * quads} candidates at most")
        if quads == 0 or mask_name in ("checkerboard", "zero"):
            assert F == 0 and not want["used"].any()                                                # valid and empty
        elif mask_name == "last_row_and_column" and max_edge is None:
            assert want["counts"].tolist() == [[3, 1]] * shape[0]                                   # the corner where the row meets the column
        elif mask_name in ("null", "ones") and max_edge is None:
            assert F == 2 * quads                                                                   # NaN points included: the flag is off
    if quads * 2 < 20000 and mask_name == "keep90":                                                 # every optional output on and off
        want = mc.rule(points, mask, half)
        for k in range(4):
            for outputs in itertools.combinations("uvfr", k):
                check(run(points, mask, half, outputs="".join(outputs)), want)


def test_the_limits_do_what_the_test_above_needs_them_for():
    shape = (3, 37, 70)
    points = scene_of(shape)[0]
    half, exact = limits_of(shape)
    off, on = mc.rule(points)["counts"][:, 1].sum(), mc.rule(points, None, half)["counts"][:, 1].sum()
    assert 0.25 * off < on < 0.75 * off                                                             # about half the candidates fail
    assert exact is not None
    r = mc.rule(points, None, exact)
    lim = np.float32(exact) * np.float32(exact)
    at = ((r["ea"] == lim) & r["anti"]) | ((r["em"] == lim) & ~r["anti"] & np.isfinite(r["ea"]))     # the diagonal the quad is cut along
    assert at.any()
    below = mc.rule(points, None, np.nextafter(np.float32(exact), np.float32(0)))
    assert below["counts"][:, 1].sum() < r["counts"][:, 1].sum()                                    # equality is kept: `<` would lose faces
    for name in ("depth_edge", "keep50", "hole"):
        m = mask_of(shape, name)
        assert 0 < mc.rule(points, m)["counts"][:, 1].sum() < off and (m == 0).any()


def quad(anti_shorter):
    p = np.array([[[0, 0, 2], [1, 0, 2]], [[0, 1, 2], [1, 1, 2]]], np.float32)
    if anti_shorter:
        p[1, 1, :2] = (1.5, 1.5)
    else:
        p[0, 1, 0] = 1.5
    return p


def both(points, mask, max_edge):
    """the rule's result after the kernel's outputs were found equal to it"""
    want = mc.rule(points, mask, max_edge)
    got = run(points, mask, max_edge)
    check(got, want)
    check_vertex_records(points, mc.scene_colors(*points.shape[:3], seed=7), got, want)
    return want


def test_all_sixteen_masks_of_one_quad_under_both_diagonals():
    """32 views of 2 x 2: view 2 m + a has mask m and the anti diagonal shorter (a = 1) or longer (a = 0)"""
    points = np.stack([quad(bool(a)) for _ in range(16) for a in (0, 1)])
    mask = np.stack([np.array([(m >> k) & 1 for k in range(4)], np.uint8).reshape(2, 2) for m in range(16) for _ in (0, 1)])
    for max_edge in (None, 100.0):
        w = both(points, mask, max_edge)
        kept = mask.reshape(32, 4).sum(1)
        assert w["counts"][:, 1].tolist() == [2 if k == 4 else 1 if k == 3 else 0 for k in kept]
        assert w["code"][30, 0, 0] == mc.M1 | mc.M2 and w["code"][31, 0, 0] == mc.A1 | mc.A2
    w = both(points, mask, 1.2)                                                                     # sides 1 and 1.5, diagonals 1.41 and up
    assert w["counts"][:, 1].sum() == 0
    w = both(points, None, 1.45)                                                                    # the short diagonal survives, the long sides do not
    assert set(w["counts"][:, 1].tolist()) == {1}


def test_exact_ties_nan_and_inf_points():
    square = np.array([[[0, 0, 1], [1, 0, 1]], [[0, 1, 1], [1, 1, 1]]], np.float32)                 # both diagonals 2.0 exactly
    views, names = [square], ["tie"]
    for corner in range(4):
        for bad in (np.nan, np.inf, -np.inf):
            p = quad(True)
            p.reshape(-1, 3)[corner, 1] = bad
            views.append(p)
            names.append((corner, bad))
    views.append(np.full((2, 2, 3), np.nan, np.float32))
    points = np.stack(views)
    off = both(points, None, None)
    assert off["code"][0, 0, 0] == mc.M1 | mc.M2                                                    # a tie takes the main diagonal
    assert off["counts"].tolist() == [[4, 2]] * len(views)                                          # the flag is off: non-finite vertices survive
    for k, name in enumerate(names[1:], 1):
        corner, bad = name
        anti = np.isinf(bad) and corner in (0, 3)                                                   # em = +inf alone: the anti diagonal IS shorter
        assert off["code"][k, 0, 0] == (mc.A1 | mc.A2 if anti else mc.M1 | mc.M2), name
    on = both(points, None, 100.0)
    assert on["counts"][0].tolist() == [4, 2] and on["counts"][-1].tolist() == [0, 0]
    assert (on["counts"][1:-1, 1] <= 1).all() and (on["counts"][1:-1, 1] == 0).any() and (on["counts"][1:-1, 1] == 1).any()
    inf = both(points, None, float("inf"))                                                          # inf <= inf holds, NaN <= inf does not
    assert inf["counts"][-1].tolist() == [0, 0] and inf["counts"][:, 1].sum() > on["counts"][:, 1].sum()
    masked = np.ones(points.shape[:3], np.uint8)
    masked[:, 1, 1] = 0                                                                             # three kept: one triangle, with or without a NaN in it
    assert both(points, masked, None)["counts"].tolist() == [[3, 1]] * len(views)
    # equality with the limit is kept: 3 - 4 - 5, the longest edge 5 exactly; one ulp less drops the triangle
    tri = np.array([[[0, 0, 1], [3, 0, 1]], [[0, 4, 1], [9, 9, 1]]], np.float32)[None]
    three = np.array([[[1, 1], [1, 0]]], np.uint8)
    assert both(tri, three, 5.0)["counts"].tolist() == [[3, 1]]
    assert both(tri, three, float(np.nextafter(np.float32(5), np.float32(0))))["counts"].tolist() == [[0, 0]]
    assert both(tri, three, 0.0)["counts"].tolist() == [[0, 0]]


def test_a_scene_that_a_fused_sum_of_squares_would_triangulate_differently():
    """Quads whose two diagonals are coordinate permutations of one another: the three squares are the same numbers, so the choice
    hangs on the order and the rounding of the sums alone.  d_main = (a, b, c) and d_anti = a permutation of it, exactly (p00 = p10 =
    the origin).  For every way of contracting (d0 d0 + d1 d1) + d2 d2 the search keeps views on which that form cuts the other
    diagonal; the kernel gives the unfused choice on all of them."""
    rng = np.random.default_rng(17)
    K = 6000
    d = rng.uniform(0.1, 1.0, (K, 3)).astype(np.float32)
    perms = np.array(list(itertools.permutations(range(3)))[1:])
    anti = np.take_along_axis(d, perms[rng.integers(0, len(perms), K)], 1)
    points = np.zeros((K, 2, 2, 3), np.float32)
    points[:, 1, 1], points[:, 0, 1] = d, anti                                                      # p11 - p00 = d, p01 - p10 = its permutation
    want = mc.rule(points)
    keep = np.zeros(K, bool)
    for form in mc.FUSED:
        differs = mc.rule(points, fused=form)["code"][:, 0, 0] != want["code"][:, 0, 0]
        assert differs.sum() >= 8, (form, int(differs.sum()))
        keep[np.flatnonzero(differs)[:64]] = True
    points = points[keep]
    want = both(points, None, None)
    assert set(want["code"][:, 0, 0].tolist()) == {mc.A1 | mc.A2, mc.M1 | mc.M2}
    got = run(points, None, None)
    for form in mc.FUSED:
        fused = mc.rule(points, fused=form)
        differ = fused["code"][:, 0, 0] != want["code"][:, 0, 0]
        assert differ.sum() >= 8, form
        F = 2 * len(points)                                                                         # every view: four vertices, two faces
        assert len(fused["faces"]) == len(want["faces"]) == F
        assert (got["f"][:F] != fused["faces"]).any(1).reshape(-1, 2).any(1)[differ].all(), form


@pytest.mark.parametrize("record_offset", [0, 1, 2, 3])
def test_a_capacity_below_the_face_count(record_offset):
    """counts stay true, the first max_faces faces are written and nothing after them - the canary rows stay as they were -, whatever
    the alignment of the record buffer"""
    points = scene_of((3, 37, 70))[0]
    mask = mask_of((3, 37, 70), "keep90")
    want = mc.rule(points, mask, None)
    F = len(want["faces"])
    assert F > 5000
    for cap in (0, 1, 2, 700, F // 2, F - 1, F, F + 5):
        got = run(points, mask, None, cap=cap, record_offset=record_offset)
        check(got, want)
        for outputs in ("f", "r"):
            check(run(points, mask, None, cap=cap, outputs=outputs, record_offset=record_offset), want)


def test_two_runs_give_the_same_bytes_and_the_wrapper_equals_the_entry_point():
    shape = (2, 65, 129)
    points, colors, _ = scene_of(shape)
    mask = mask_of(shape, "depth_edge")
    half = limits_of(shape)[0]
    first, second = run(points, mask, half), run(points, mask, half)
    assert all(np.array_equal(first[k], second[k]) for k in "uvfr") and np.array_equal(first["counts"], second["counts"])
    want = mc.rule(points, mask, half)
    for m in (dev(mask), dev(mask).view(torch.bool)):
        out = hip.cloud_mesh(dev(points), dev(colors), m, half)
        F = len(want["faces"])
        assert tuple(out["faces"].shape) == (F, 3) and tuple(out["face_records"].shape) == (F, 13) and F > 0        # exact sizes
        check(dict(u=out["used"].cpu().numpy(), v=out["vertex_of"].cpu().numpy(), f=np.concatenate([out["faces"].cpu().numpy(), np.full((1, 3), -7)]),
                   r=np.concatenate([out["face_records"].cpu().numpy(), np.full((1, 13), 0xEE)]), counts=out["counts"].cpu().numpy(), cap=F), want)
        assert np.array_equal(out["vertex_records"].cpu().numpy(), mc.vertex_records(points, colors, want["used"]))
    only = hip.cloud_mesh(dev(points), dev(colors), None, None, face_records=False)
    assert only["face_records"] is None and np.array_equal(only["faces"].cpu().numpy(), mc.rule(points)["faces"])
    empty = hip.cloud_mesh(dev(points), dev(colors), dev(np.zeros(shape, np.uint8)))
    assert tuple(empty["faces"].shape) == (0, 3) and tuple(empty["face_records"].shape) == (0, 13) and tuple(empty["vertex_records"].shape) == (0, 15)


def test_the_call_is_capturable_and_the_replay_equals_the_eager_run():
    shape = (3, 37, 70)
    points, _, _ = scene_of(shape)
    mask = mask_of(shape, "keep90")
    half = limits_of(shape)[0]
    want = mc.rule(points, mask, half)
    F = len(want["faces"])
    t_points, t_mask = dev(points), dev(mask)

    def outputs():
        return dict(counts=torch.full((3, 2), -3, dtype=torch.int32, device="cuda"), used=torch.full(shape, 77, dtype=torch.uint8, device="cuda"),
                    vertex_of=torch.full(shape, -9, dtype=torch.int32, device="cuda"), faces=torch.full((F, 3), -7, dtype=torch.int32, device="cuda"),
                    face_records=torch.full((F, 13), 0xEE, dtype=torch.uint8, device="cuda"))
    eager = outputs()
    hip.cloud_mesh_raw(t_points, t_mask, half, **eager)                                             # loads the code object, sizes the workspace
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    out = outputs()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            hip.cloud_mesh_raw(t_points, t_mask, half, **out)
    for _ in range(2):
        for o in out.values():
            o.fill_(9)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(out[k], eager[k]) for k in out)
        check(dict(u=out["used"].cpu().numpy(), v=out["vertex_of"].cpu().numpy(), f=np.concatenate([out["faces"].cpu().numpy(), np.full((1, 3), -7)]),
                   r=np.concatenate([out["face_records"].cpu().numpy(), np.full((1, 13), 0xEE)]), counts=out["counts"].cpu().numpy(), cap=F), want)
