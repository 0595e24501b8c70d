"""GPU: g2v_cloud_normals and g2v_cloud_compact_normals (csrc/normals.hip) against the fp32 rule of tests/normals_check.py, byte for
byte, on normals (as int32 bits: -0.0 counts), valid, cos_view and colors_out: the synthetic scene at every shape class under every
mask, steps 1, 2 and 8, the edge limit off, at the median edge and at an edge's exact length, with poses and without, both forms of
the kernel, every subset of the outputs, a scene on which a fused multiply-add gives other bytes, repeatability, graph capture; the
27-byte records at every alignment and under a capacity below the count."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import normals_check as nc  # noqa: E402
from g2vlm_amd import hip  # noqa: E402

pytestmark = pytest.mark.gpu
# the single pixel; one row; one column; the smallest view with a pair; exactly one 32 x 8 tile; one past it in both directions; 3 x 3;
# the family's usual scene; more than one block of 1024 pixels per view and a width that is no multiple of anything; more blocks (524)
# than one pass of the scan holds (256)
SHAPES = [(1, 1, 1), (1, 1, 5), (1, 5, 1), (1, 2, 2), (1, 8, 32), (1, 9, 33), (2, 3, 3), (3, 37, 70), (2, 65, 129), (2, 518, 518)]
MASKS = ["null", "ones", "keep50", "keep90", "checkerboard", "zero", "hole", "last_row_and_column", "depth_edge"]   # tests/test_mesh_gpu.py's
STEPS = (1, 2, 8)
OUTPUTS = "nvcq"                                             # n(ormals), v(alid), c(os_view), q = colors_out
SENTINEL = {"n": -7.5, "v": 77, "c": -3.25, "q": 9.5}
KEY = {"n": "normals", "v": "valid", "c": "cos_view", "q": "colors"}
CANARY_ROWS = 3
BIG = (2, 518, 518)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def scene_of(shape):
    n = SHAPES.index(shape)
    s = nc.scene(*shape, seed=n)
    return s["points"], nc.scene_colors(*shape, seed=n), s["local"], s["poses"]


def mask_of(shape, name):
    N, H, W = shape
    if name == "null":
        return None
    if name == "ones":
        return np.ones(shape, np.uint8)
    if name in ("keep50", "keep90"):
        return nc.random_mask(shape, 300 + SHAPES.index(shape), keep=0.5 if name == "keep50" else 0.9)
    if name == "checkerboard":
        return nc.checkerboard(*shape)
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
    return nc.depth_edge_mask(scene_of(shape)[2])


@functools.lru_cache(maxsize=None)
def limits_of(shape, step):
    """nc.edge_limits of the unmasked scene: (about the median edge, a max_edge whose square equals an edge's squared length bit for bit
    - or None where the view has no edge at this step)"""
    points, _, _, poses = scene_of(shape)
    return nc.edge_limits(points, None, poses, step, tries=2 if shape == BIG else 8)


def run(points, mask, poses, step=1, max_edge=None, outputs=OUTPUTS, flags=0):
    """the raw entry point with exactly the optional outputs asked for, into sentinel-filled tensors that sit inside a larger sentinel-
    filled store (nothing may be written before or after them); the inputs must keep their bits"""
    n, h, w = points.shape[:3]
    t_points, t_mask, t_poses = dev(points), dev(mask), dev(poses)
    before = (t_points.clone(), None if t_mask is None else t_mask.clone(), None if t_poses is None else t_poses.clone())
    pad = 16
    sizes = {"n": n * h * w * 3, "v": n * h * w, "c": n * h * w, "q": n * 3 * h * w}
    shapes = {"n": (n, h, w, 3), "v": (n, h, w), "c": (n, h, w), "q": (n, 3, h, w)}
    store = {k: torch.full((sizes[k] + 2 * pad,), SENTINEL[k], dtype=torch.uint8 if k == "v" else torch.float32, device="cuda") for k in OUTPUTS}
    out = {k: store[k][pad:pad + sizes[k]].view(shapes[k]) for k in OUTPUTS}
    ptr = {k: hip._p(out[k]) if k in outputs else None for k in OUTPUTS}
    rcode = hip.lib().g2v_cloud_normals(hip._p(t_points), hip._p(t_mask), hip._p(t_poses), n, h, w, step,
                                        flags | (0 if max_edge is None else hip.NORMALS_MAX_EDGE), float(max_edge or 0.0), ptr["n"], ptr["v"],
                                        ptr["c"], ptr["q"], hip._stream())
    assert rcode == 0
    torch.cuda.synchronize()
    assert torch.equal(t_points.view(torch.int32), before[0].view(torch.int32)) and (t_mask is None or torch.equal(t_mask, before[1])) and \
        (t_poses is None or torch.equal(t_poses.view(torch.int32), before[2].view(torch.int32)))
    for k in OUTPUTS:
        assert bool((store[k][:pad] == SENTINEL[k]).all()) and bool((store[k][pad + sizes[k]:] == SENTINEL[k]).all()), k   # nothing past an end
        if k not in outputs:
            assert bool((out[k] == SENTINEL[k]).all()), k                                           # an output not asked for is not written
    return {k: out[k].cpu().numpy() for k in outputs}


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def check(got, want):
    for k, a in got.items():
        w = want[KEY[k]]
        assert a.dtype == w.dtype and a.shape == w.shape, k
        assert np.array_equal(bits(a), bits(w)), (k, int((bits(a) != bits(w)).sum()), a.size)


@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_rule_byte_for_byte(shape, mask_name):
    points, _, local, poses = scene_of(shape)
    mask = mask_of(shape, mask_name)
    big = shape == BIG
    cases = []                                                                                      # (points, poses, step, max_edge, flags)
    if not big:
        for step in STEPS:
            half, exact = limits_of(shape, step)
            for max_edge in (None, half) + (() if exact is None else (exact,)):
                cases.append((points, poses, step, max_edge, 0))
        cases += [(local, None, 1, None, 0), (local, None, 2, limits_of(shape, 2)[0], 0), (points, None, 1, None, 0)]   # poses NULL
        cases += [(points, poses, 1, None, hip.NORMALS_HALO), (points, poses, 1, limits_of(shape, 1)[0], hip.NORMALS_HALO),
                  (local, None, 1, None, hip.NORMALS_HALO), (points, poses, 2, None, hip.NORMALS_PLAIN)]
    elif mask_name in ("null", "keep50", "depth_edge"):                                             # the large view: one case of every kind
        half, exact = limits_of(shape, 1)
        cases = [(points, poses, 1, None, 0), (points, poses, 1, exact, 0), (points, poses, 2, None, 0), (points, poses, 8, None, 0),
                 (local, None, 1, None, 0), (points, poses, 1, half, hip.NORMALS_HALO)]
    else:
        cases = [(points, poses, 1, None, 0), (points, poses, 1, None, hip.NORMALS_HALO)]
    for pts, pose, step, max_edge, flags in cases:
        want = nc.rule(pts, mask, pose, step, max_edge)
        check(run(pts, mask, pose, step, max_edge, flags=flags), want)
        nvalid = int(want["valid"].sum())
        if mask_name == "zero" or (mask_name == "checkerboard" and step % 2 == 1) or min(shape[1:]) <= step:
            assert nvalid == 0                                                                      # valid and empty (an even step stays on one colour)
        elif mask_name in ("null", "ones", "hole") and max_edge is None:
            assert nvalid > 0
    print(f"{shape} {mask_name}: {len(cases)} cases equal")


def test_the_limits_do_what_the_test_above_needs_them_for():
    shape = (3, 37, 70)
    points, _, _, poses = scene_of(shape)
    for step in STEPS:
        half, exact = limits_of(shape, step)
        off, on = nc.rule(points, None, poses, step), nc.rule(points, None, poses, step, half)
        assert 0.02 * off["pairs"].sum() < on["pairs"].sum() < 0.9 * off["pairs"].sum()             # a good share of the pairs fails
        assert exact is not None
        under = nc.rule(points, None, poses, step, float(np.nextafter(np.float32(exact), np.float32(0))))
        assert (nc.rule(points, None, poses, step, exact)["pairs"] > under["pairs"]).any()          # equality is kept: `<` would lose pairs
    for name in ("depth_edge", "keep50", "hole"):
        m = mask_of(shape, name)
        assert 0 < nc.rule(points, m, poses)["valid"].sum() < off["valid"].size and (m == 0).any()
    counts = set()
    for name in MASKS:
        counts |= set(np.unique(nc.rule(points, mask_of(shape, name), poses)["pairs"]).tolist())
    assert counts == {0, 1, 2, 4}


def test_every_subset_of_the_outputs():
    shape = (3, 37, 70)
    points, _, _, poses = scene_of(shape)
    mask = mask_of(shape, "keep90")
    half = limits_of(shape, 1)[0]
    want = nc.rule(points, mask, poses, 1, half)
    for flags in (0, hip.NORMALS_HALO):
        for k in range(1, 5):
            for outputs in itertools.combinations(OUTPUTS, k):
                check(run(points, mask, poses, 1, half, outputs="".join(outputs), flags=flags), want)
    t = dev(points)
    assert hip.lib().g2v_cloud_normals(hip._p(t), None, None, 3, 37, 70, 1, 0, 0.0, None, None, None, None, hip._stream()) == -22


def test_hand_built_inputs_for_each_branch_of_the_rule():
    # 3 - 4 - 5: an edge of exactly max_edge is kept, one ulp less drops it; -0.0 components
    p = np.zeros((1, 2, 2, 3), np.float32)
    p[..., 2] = 1
    p[0, 0, 1, 0], p[0, 1, 0, 1], p[0, 1, 1, :2] = 3, 4, (3, 4)
    for max_edge in (None, 4.0, float(np.nextafter(np.float32(4), np.float32(0))), 0.0, float("inf")):
        want = nc.rule(p, None, None, 1, max_edge)
        for flags in (0, hip.NORMALS_HALO):
            check(run(p, None, None, 1, max_edge, flags=flags), want)
    assert np.signbit(nc.rule(p, None, None, 1, 4.0)["normals"][0, 0, 0]).all()
    # NaN, inf and huge points, collinear and coincident neighbours, a point at the camera centre, overflow of s2
    rng = np.random.default_rng(3)
    base = nc.scene(1, 5, 5, seed=2)["local"][0]
    views = []
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        v = base.copy()
        v[2, 2, 1] = bad
        views.append(v)
    huge = base.copy()
    huge[2, 2] = (1e30, -1e30, 1e30)
    line = np.zeros((5, 5, 3), np.float32)
    line[..., 0] = np.arange(5)[None, :] + 10 * np.arange(5)[:, None]
    at_camera = base.copy()
    at_camera[2, 2] = 0
    views += [huge, line, np.ones((5, 5, 3), np.float32), base * np.float32(1e19), at_camera, base * np.float32(1e-25),
              rng.standard_normal((5, 5, 3)).astype(np.float32)]
    points = np.stack(views)
    poses = np.tile(np.eye(4, dtype=np.float32), (len(views), 1, 1))
    poses[:, :3, 3] = rng.standard_normal((len(views), 3)).astype(np.float32) * 0.1
    poses[-1, :3, 3] = (np.inf, 0, np.nan)                                                          # a non-finite centre: t and dd are what they are
    for pose in (None, poses):
        for max_edge in (None, 1.0):
            for step in (1, 2):
                want = nc.rule(points, None, pose, step, max_edge)
                check(run(points, None, pose, step, max_edge), want)
                if step == 1:
                    check(run(points, None, pose, step, max_edge, flags=hip.NORMALS_HALO), want)
    want = nc.rule(points, None, None)
    assert want["valid"][5, 2, 2] == 0 and want["valid"][6].sum() == 0 and want["valid"][7].sum() == 0 and want["valid"][8].sum() == 0
    assert want["valid"][9, 2, 2] == 1 and want["cos_view"][9, 2, 2] == 0


def test_a_scene_on_which_a_fused_multiply_add_gives_other_bytes():
    """asserted first: both ways of contracting a b - c d change the normals of this scene; the kernel equals the uncontracted rule"""
    shape = (3, 37, 70)
    points, _, local, poses = scene_of(shape)
    want = nc.rule(points, None, poses)
    for form in nc.FUSED:
        fused = nc.rule(points, None, poses, fused=form)
        differ = (bits(fused["normals"]) != bits(want["normals"])).any(-1)
        assert differ.mean() > 0.1, form
        assert (bits(fused["colors"]) != bits(want["colors"])).any() and (bits(fused["cos_view"]) != bits(want["cos_view"])).any()
    for flags in (0, hip.NORMALS_HALO):
        got = run(points, None, poses, flags=flags)
        check(got, want)
        for form in nc.FUSED:
            assert (bits(got["n"]) != bits(nc.rule(points, None, poses, fused=form)["normals"])).any()


def test_two_runs_give_the_same_bytes_and_the_wrapper_equals_the_entry_point():
    shape = (2, 65, 129)
    points, _, local, poses = scene_of(shape)
    mask = mask_of(shape, "depth_edge")
    half = limits_of(shape, 2)[0]
    first, second = run(points, mask, poses, 2, half), run(points, mask, poses, 2, half)
    assert all(np.array_equal(bits(first[k]), bits(second[k])) for k in OUTPUTS)
    want = nc.rule(points, mask, poses, 2, half)
    for m in (dev(mask), dev(mask).view(torch.bool)):
        out = hip.cloud_normals(dev(points), m, dev(poses), 2, half, colors=True)
        check({k: out[KEY[k]].cpu().numpy() for k in OUTPUTS}, want)
    out = hip.cloud_normals(dev(local), None, None)
    assert out["colors"] is None
    check({k: out[KEY[k]].cpu().numpy() for k in "nvc"}, nc.rule(local, None, None))


def test_the_call_is_capturable_and_the_replay_equals_the_eager_run():
    shape = (3, 37, 70)
    points, _, _, poses = scene_of(shape)
    mask = mask_of(shape, "keep90")
    half = limits_of(shape, 1)[0]
    want = nc.rule(points, mask, poses, 1, half)
    t_points, t_mask, t_poses = dev(points), dev(mask), dev(poses)

    def outputs():
        return dict(normals=torch.full(shape + (3,), 5.0, device="cuda"), valid=torch.full(shape, 77, dtype=torch.uint8, device="cuda"),
                    cos_view=torch.full(shape, 5.0, device="cuda"), colors=torch.full((3, 3, 37, 70), 5.0, device="cuda"))
    eager = outputs()
    hip.cloud_normals_raw(t_points, t_mask, t_poses, 1, half, **eager)                              # loads the code object
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    out = outputs()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            hip.cloud_normals_raw(t_points, t_mask, t_poses, 1, half, **out)
    for _ in range(2):
        for o in out.values():
            o.fill_(9)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(out[k], eager[k]) for k in out)
        check({k: out[KEY[k]].cpu().numpy() for k in OUTPUTS}, want)


# ------------------------------------------------------------------------------------------------ g2v_cloud_compact_normals
def compact(points, normals, colors, mask, cap=None, record_offset=0, records=True):
    """the raw entry point into a sentinel-filled record buffer at byte offset record_offset, with CANARY_ROWS rows after the capacity,
    from a junk-filled workspace: (records uint8 [cap + CANARY_ROWS, 27], counts int32 [N])"""
    n, h, w = points.shape[:3]
    t = [dev(points), dev(normals), dev(colors), dev(mask)]
    before = [x.clone() for x in t]
    if cap is None:
        cap = n * h * w
    room = cap + CANARY_ROWS
    store = torch.full((room * 27 + 8,), 0xEE, dtype=torch.uint8, device="cuda")
    rec = store[record_offset:record_offset + room * 27].view(room, 27)
    counts = torch.full((n,), -3, dtype=torch.int32, device="cuda")
    nbytes = hip.cloud_compact_normals_workspace(n, h, w)
    assert nbytes > 0
    ws = torch.full(((nbytes + 7) // 8,), 0x0123456789ABCDEF, dtype=torch.int64, device="cuda")     # junk: needs no initialisation
    rcode = hip.lib().g2v_cloud_compact_normals(hip._p(t[0]), hip._p(t[1]), hip._p(t[2]), hip._p(t[3]), n, h, w, hip._p(rec) if records else None,
                                                cap if records else 0, hip._p(counts), hip._p(ws), nbytes, hip._stream())
    assert rcode == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(t, before))
    assert bool((store[:record_offset] == 0xEE).all()) and bool((store[record_offset + room * 27:] == 0xEE).all())
    return rec.cpu().numpy(), counts.cpu().numpy()


def check_records(got, counts, want, mask, cap):
    assert np.array_equal(counts, (np.asarray(mask) != 0).reshape(len(counts), -1).sum(1)), counts.tolist()   # the true numbers, whatever the capacity
    written = min(len(want), cap)
    assert np.array_equal(got[:written], want[:written])
    assert (got[written:] == 0xEE).all()                                                            # nothing past the count or the capacity


@pytest.mark.parametrize("record_offset", [0, 1, 2, 3])
def test_records_equal_the_reference_packer_at_every_alignment(record_offset):
    for shape in ((1, 1, 1), (1, 9, 33), (3, 37, 70), (2, 65, 129)):
        points, colors, _, poses = scene_of(shape)
        for name in ("ones", "keep50", "hole", "last_row_and_column", "depth_edge"):
            mask = mask_of(shape, name)
            normals = nc.rule(points, mask, poses)["normals"]
            want = nc.records(points, normals, colors, mask)
            got, counts = compact(points, normals, colors, mask, record_offset=record_offset)
            check_records(got, counts, want, mask, shape[0] * shape[1] * shape[2])


def test_the_normal_is_copied_bit_for_bit():
    shape = (2, 3, 3)
    points, colors, _, _ = scene_of(shape)
    normals = np.random.default_rng(1).standard_normal(shape + (3,)).astype(np.float32)
    normals[0, 0, 0] = (-0.0, 0.0, -0.0)
    normals[0, 0, 1] = (np.nan, np.inf, -np.inf)
    normals[0, 0, 2] = np.array([0x7fc00123, 0xffc00001, 0x00000001], np.uint32).view(np.float32)  # NaN payloads, a denormal
    mask = np.ones(shape, np.uint8)
    got, counts = compact(points, normals, colors, mask)
    assert np.array_equal(got[:18], nc.records(points, normals, colors, mask)) and counts.tolist() == [9, 9]


@pytest.mark.parametrize("record_offset", [0, 3])
def test_a_capacity_below_the_count(record_offset):
    shape = (3, 37, 70)
    points, colors, _, poses = scene_of(shape)
    mask = mask_of(shape, "keep90")
    normals = nc.rule(points, mask, poses)["normals"]
    want = nc.records(points, normals, colors, mask)
    M = len(want)
    assert M > 5000
    for cap in (0, 1, 2, 700, M // 2, M - 1, M, M + 5):
        got, counts = compact(points, normals, colors, mask, cap=cap, record_offset=record_offset)
        check_records(got, counts, want, mask, cap)
    got, counts = compact(points, normals, colors, mask, records=False)                            # max_records = 0 with records NULL only counts
    check_records(got, counts, want, mask, 0)


def test_an_all_zero_mask_and_the_large_view():
    for shape in ((3, 37, 70), BIG):
        points, colors, _, poses = scene_of(shape)
        got, counts = compact(points, np.zeros(shape + (3,), np.float32), colors, np.zeros(shape, np.uint8))
        assert counts.tolist() == [0] * shape[0] and (got == 0xEE).all()
    points, colors, _, poses = scene_of(BIG)                                                        # 524 blocks: more than one pass of the scan
    for name in ("keep50", "depth_edge", "ones"):
        mask = mask_of(BIG, name)
        normals = nc.rule(points, mask, poses)["normals"]
        want = nc.records(points, normals, colors, mask)
        got, counts = compact(points, normals, colors, mask, record_offset=1)
        check_records(got, counts, want, mask, BIG[0] * BIG[1] * BIG[2])


def test_the_wrapper_counts_first_and_allocates_the_exact_size():
    shape = (2, 65, 129)
    points, colors, _, poses = scene_of(shape)
    mask = mask_of(shape, "depth_edge")
    r = hip.cloud_normals(dev(points), dev(mask), dev(poses))
    want = nc.records(points, nc.rule(points, mask, poses)["normals"], colors, mask)
    for m in (dev(mask), dev(mask).view(torch.bool)):
        records, counts = hip.cloud_compact_normals(dev(points), r["normals"], dev(colors), m)
        assert tuple(records.shape) == (len(want), 27) and records.is_contiguous() and np.array_equal(records.cpu().numpy(), want)
        assert counts.cpu().tolist() == mask.reshape(2, -1).sum(1).tolist()
    plain, plain_counts = hip.cloud_compact(dev(points), dev(colors), dev(mask))                    # g2v_cloud_compact: the same pixels, the same order
    assert torch.equal(plain[:, :12], records[:, :12]) and torch.equal(plain[:, 12:], records[:, 24:]) and torch.equal(plain_counts, counts)
    empty, counts = hip.cloud_compact_normals(dev(points), r["normals"], dev(colors), dev(np.zeros(shape, np.uint8)))
    assert tuple(empty.shape) == (0, 27) and counts.cpu().tolist() == [0, 0]
