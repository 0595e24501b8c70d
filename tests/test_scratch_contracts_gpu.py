"""GPU: every entry point of include/g2vlm_hip.h that borrows memory from the caller, held to what the header says about that
memory (tests/scratch_check.py has the table, the Arena and the staged runner; DESIGN.md 6v the reading audit behind it).

(a) exact, guarded, dirty.  The entry point runs once on the wrapper's ordinary scratch - that run is held to its owning check
    module's reference, as the existing tests hold it - and then on an Arena payload of EXACTLY the queried size at EXACTLY the
    demanded alignment under zeros, ones, leftover (and 0xFF for the fp32 workspaces of the attention kernels): every output
    equals the ordinary run bit for bit and both 64 KiB guards are intact.  zero_once rows get their ticket words zeroed and
    everything behind them poisoned.
(b) carried over.  One scratch for a whole sequence of shapes: large split -> small split -> no split -> large split for the
    ticket kernels (every launch equals the same launch on fresh scratch, the ticket words are all zero after every launch);
    big -> small -> big through one buffer for the uninit_ok kernels, the small launch writing nothing past its own size.
(c) the export chain mask -> intrinsics -> consistency -> voxel -> compaction with ONE poisoned payload as every workspace.

Every assertion is bit equality, an intact guard, an all-zero ticket region or the owning module's own bound: no tolerance is
introduced here.  The kernels are all run-to-run bit-identical (their own tests' "two runs give identical bytes"), except that the
skinny GEMM's result depends on (S, KS), which depends on the workspace size: it is compared bit for bit where g2v_gemm_route
reports the same split and with gemm_check's bound otherwise."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import cloud_check  # noqa: E402
import consistency_check as cc  # noqa: E402
import decode_check as D  # noqa: E402
import gemm_check as G  # noqa: E402
import imageop_check as I  # noqa: E402
import mesh_check  # noqa: E402
import nn_check  # noqa: E402
import normals_check  # noqa: E402
import render_check as rc  # noqa: E402
import scratch_check as sc  # noqa: E402
import voxel_check  # noqa: E402
from scratch_check import Arena, CONTRACTS  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
COVERED = set()                                              # entry points a test of this module ran under every admissible pattern


@pytest.fixture(scope="module")
def hip():
    from g2vlm_amd import hip as h
    h.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return h


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def sync():
    torch.cuda.synchronize()


def exact(name, nbytes, run, want, zero=(), leftover=None, fp32=False, what=""):
    """(a) for one launch: every admissible pattern, in order; nothing may be left unrun"""
    stages = sc.staged(name, nbytes, run, want, sc.patterns_for(name, fp32), zero=zero, leftover=leftover, sync=sync)
    sc.assert_staged(name, stages, what)
    assert all(s.status in ("ok", "not applicable") for s in stages), (name, what, stages)
    assert [s.pattern for s in stages if s.status == "ok"][:2] == ["zeros", "ones"], (name, what, stages)
    COVERED.add(name)
    return stages


def big_small_big(name, cases, what=""):
    """(b) for an uninit_ok entry point: cases = [(nbytes, run, want)] of the big and the small shape.  One poisoned buffer of the
    big size serves big, small (in its first bytes), big; the small launch leaves everything past its own size alone."""
    (nb, run_b, want_b), (ns, run_s, want_s) = cases
    assert ns <= nb and CONTRACTS[name].kind == "uninit_ok"
    arena = Arena(nb, CONTRACTS[name].align, DEV).fill("ones")

    class Head:                                              # the small launch sees the first ns bytes of the same payload
        nbytes, align, ptr = ns, arena.align, arena.ptr

        @staticmethod
        def payload(dtype=U8):
            return arena.head(ns, dtype)
    for step, (view, run, want, keep) in enumerate(((arena, run_b, want_b, None), (Head, run_s, want_s, ns), (arena, run_b, want_b, None))):
        snap = arena.snapshot() if keep is not None else None
        got = run(view)
        sync()
        diff = sc.first_difference(got, want)
        assert diff is None, f"{name} {what} step {step} of big -> small -> big: {diff}"
        arena.check(**(dict(keep_from=keep, snapshot=snap) if keep is not None else {}))


# =============================================================================================== the point-cloud families
CLOUD_SHAPES = [(1, 1, 1), (1, 32, 32), (1, 32, 33), (3, 37, 70), (1, 513, 512)]   # 1024 / 1056 pixels: on the block and past it; 257 blocks
ids = lambda s: "x".join(map(str, s))                        # noqa: E731
_SCENES = {}
VOXEL, MAX_EDGE, RTOL = 0.11, 0.35, 0.03


def scene(shape):
    """consistency_check's scene of that shape with render_check's colours and a random mask, on the host and on the device"""
    if shape not in _SCENES:
        n, h, w = shape
        s = cc.scene(n, h, w, seed=n + h + w)
        s["colors"] = rc.scene_colors(n, h, w, seed=h)
        s["mask"] = cc.random_mask(shape, seed=w, keep=0.8)
        s["origin"] = voxel_check.default_origin(s["points"], s["mask"], VOXEL).tolist()
        s["d"] = {k: dev(s[k]) for k in ("points", "local", "poses", "K", "colors", "mask")}
        _SCENES[shape] = s
    return _SCENES[shape]


def eq(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.tobytes() == want.astype(got.dtype).tobytes(), what


class Cloud:
    """One entry point of the cloud family at one shape: size(), run(workspace tensor or None) -> tuple, reference(outputs)."""

    def __init__(self, hip, shape):
        self.hip, self.shape, self.s = hip, shape, scene(shape)
        self.d = self.s["d"]

    def launch(self, arena):
        return self.run(arena.payload(U8))


class Compact(Cloud):
    name = "g2v_cloud_compact"

    def size(self):
        return self.hip.cloud_compact_workspace(*self.shape)

    def run(self, ws):
        return self.hip.cloud_compact(self.d["points"], self.d["colors"], self.d["mask"], workspace=ws)

    def reference(self, out):
        want, counts = cloud_check.pack_records(self.s["points"], self.s["colors"], self.s["mask"])
        eq(out[0], want, "records")
        assert out[1].cpu().tolist() == counts.tolist()


class CompactNormals(Cloud):
    name = "g2v_cloud_compact_normals"

    def __init__(self, hip, shape):
        super().__init__(hip, shape)
        self.normals = hip.cloud_normals(self.d["points"], self.d["mask"], self.d["poses"])["normals"]

    def size(self):
        return self.hip.cloud_compact_normals_workspace(*self.shape)

    def run(self, ws):
        return self.hip.cloud_compact_normals(self.d["points"], self.normals, self.d["colors"], self.d["mask"], workspace=ws)

    def reference(self, out):
        eq(out[0], normals_check.records(self.s["points"], self.normals.cpu().numpy(), self.s["colors"], self.s["mask"]), "records")
        assert out[1].cpu().tolist() == (self.s["mask"] != 0).reshape(self.shape[0], -1).sum(1).tolist()


class Intrinsics(Cloud):
    name = "g2v_intrinsics_lsq"

    def size(self):
        return self.hip.intrinsics_lsq_workspace(*self.shape)

    def run(self, ws):
        return self.hip.intrinsics_lsq(self.d["local"], self.d["mask"], workspace=ws)

    def reference(self, out):
        from test_cloud_gpu import check_K                   # the owning test's comparison: 4 fp32 ulp against fp64 lstsq
        ref, used = cloud_check.fit_intrinsics(self.s["local"], self.s["mask"])
        assert out[1].cpu().tolist() == used.tolist()
        check_K(out[0].cpu().numpy(), ref, self.shape[1], self.shape[2])


class Mesh(Cloud):
    """g2v_cloud_mesh with `used` and `vertex_of` left to the workspace: every region of it is in use"""
    name = "g2v_cloud_mesh"

    def __init__(self, hip, shape):
        super().__init__(hip, shape)
        self.want = mesh_check.rule(self.s["points"], self.s["mask"], MAX_EDGE)
        self.nf = len(self.want["faces"])

    def size(self):
        return self.hip.cloud_mesh_workspace(*self.shape)

    def run(self, ws):
        counts = torch.full((self.shape[0], 2), -7, dtype=I32, device=DEV)
        faces = torch.full((self.nf, 3), -7, dtype=I32, device=DEV)
        rec = torch.full((self.nf, 13), 0x5A, dtype=U8, device=DEV)
        self.hip.cloud_mesh_raw(self.d["points"], self.d["mask"], MAX_EDGE, counts, None, None, faces, rec, workspace=ws)
        return counts, faces, rec

    def reference(self, out):
        eq(out[0], self.want["counts"], "counts")
        eq(out[1], self.want["faces"], "faces")
        eq(out[2], self.want["face_records"], "face records")


class VoxelAssign(Cloud):
    name = "g2v_voxel_assign"

    def size(self):
        return self.hip.voxel_assign_workspace(*self.shape)

    def run(self, ws):
        voxel_of, stats = self.hip.voxel_assign(self.d["points"], self.d["mask"], VOXEL, self.s["origin"], workspace=ws)
        return voxel_of, torch.tensor(stats, dtype=I32)

    def reference(self, out):
        want = voxel_check.downsample(self.s["points"], self.s["colors"], self.s["mask"], VOXEL, self.s["origin"])
        eq(out[0], want["voxel_of"], "voxel_of")
        assert out[1].tolist() == want["stats"]


class VoxelReduce(Cloud):
    name = "g2v_voxel_reduce"

    def __init__(self, hip, shape):
        super().__init__(hip, shape)
        self.voxel_of, stats = hip.voxel_assign(self.d["points"], self.d["mask"], VOXEL, self.s["origin"])
        self.M = stats[0]

    def size(self):
        return self.hip.voxel_reduce_workspace(self.M)

    def run(self, ws):
        return self.hip.voxel_reduce(self.d["points"], self.d["colors"], self.voxel_of, self.M, VOXEL, self.s["origin"], workspace=ws)

    def reference(self, out):
        want = voxel_check.downsample(self.s["points"], self.s["colors"], self.s["mask"], VOXEL, self.s["origin"])
        assert self.M == want["stats"][0]
        for g, k in zip(out, ("records", "counts", "points", "colors")):
            eq(g, want[k], k)


class Consistency(Cloud):
    name = "g2v_cloud_consistency"

    def size(self):
        return self.hip.cloud_consistency_workspace(*self.shape)

    def run(self, ws):
        d = self.d
        return self.hip.cloud_consistency(d["points"], d["local"], d["mask"], d["poses"], d["K"], RTOL, 1, 0, pairs=True, workspace=ws)

    def reference(self, out):
        s = self.s
        want = cc.rule(s["points"], s["local"], s["poses"], s["K"], s["mask"], RTOL, min_agree=1, max_in_front=0)
        for g, k in zip(out, ("agree", "in_front", "mask_out", "pairs")):
            eq(g, want[k].astype(np.uint8) if k == "mask_out" else want[k], k)


CLOUD_FAMILY = [Compact, CompactNormals, Intrinsics, Mesh, VoxelAssign, VoxelReduce, Consistency]
SMALLER = {(1, 32, 32): (1, 1, 1), (1, 32, 33): (1, 32, 32), (3, 37, 70): (1, 32, 33), (1, 513, 512): (3, 37, 70)}   # the `leftover` shape


def leftover_of(small):
    def go(arena):
        n = small.size()
        assert n <= arena.nbytes, (n, arena.nbytes)
        small.run(arena.head(n))
    return go


@pytest.mark.parametrize("shape", CLOUD_SHAPES, ids=ids)
@pytest.mark.parametrize("family", CLOUD_FAMILY, ids=lambda f: f.name)
def test_cloud_entry_points_on_exact_guarded_dirty_workspaces(hip, family, shape):
    f = family(hip, shape)
    want = f.run(None)
    sync()
    f.reference(want)
    left = None
    if shape in SMALLER:
        small = family(hip, SMALLER[shape])
        if 0 < small.size() <= f.size():
            left = leftover_of(small)
    exact(f.name, f.size(), f.launch, want, leftover=left, what=ids(shape))


@pytest.mark.parametrize("family", CLOUD_FAMILY, ids=lambda f: f.name)
def test_cloud_entry_points_big_small_big_through_one_buffer(hip, family):
    big, small = family(hip, (3, 37, 70)), family(hip, (1, 32, 33))
    cases = []
    for f in (big, small):
        want = f.run(None)
        sync()
        cases.append((f.size(), f.launch, want))
    big_small_big(big.name, cases)


RENDER_SHAPES = [(1, 1, 1), (2, 9, 13), (3, 37, 70)]         # (M, OH, OW)


class Render(Cloud):
    name = "g2v_cloud_render"

    def __init__(self, hip, target):
        super().__init__(hip, (3, 37, 70))
        self.M, self.OH, self.OW = target
        self.poses, self.K = rc.targets(self.s, *target)
        self.skip = np.array([m % 4 - 1 for m in range(self.M)], np.int32)

    def size(self):
        return self.hip.cloud_render_workspace(self.M, self.OH, self.OW)

    def run(self, ws):
        d = self.d
        return self.hip.cloud_render(d["points"], d["colors"], d["mask"], dev(self.poses), dev(self.K), (self.OH, self.OW), 1, 0x102030,
                                     dev(self.skip), workspace=ws)

    def reference(self, out):
        s = self.s
        want = rc.rule(s["points"], s["colors"], s["mask"], self.poses, self.K, self.skip, self.OH, self.OW, 1, 0x102030)
        eq(out[0], want["color"], "color")
        eq(out[1].view(I32), want["depth"].view(np.int32), "depth")
        eq(out[2], want["index"], "index")


@pytest.mark.parametrize("target", RENDER_SHAPES, ids=ids)
def test_render_on_exact_guarded_dirty_workspaces(hip, target):
    f = Render(hip, target)
    want = f.run(None)
    sync()
    f.reference(want)
    i = RENDER_SHAPES.index(target)
    exact(f.name, f.size(), f.launch, want, leftover=leftover_of(Render(hip, RENDER_SHAPES[i - 1])) if i else None, what=ids(target))


def test_render_big_small_big_through_one_buffer(hip):
    cases = []
    for t in (RENDER_SHAPES[2], RENDER_SHAPES[1]):
        f = Render(hip, t)
        want = f.run(None)
        sync()
        cases.append((f.size(), f.launch, want))
    big_small_big("g2v_cloud_render", cases)


NN_SHAPES = [(1, 1), (255, 1025), (5000, 3000)]              # (Nq, Nt)


class NN:
    name = "g2v_cloud_nn"

    def __init__(self, hip, counts, path):
        self.hip, (self.nq, self.nt), self.path = hip, counts, path
        rng = np.random.default_rng(self.nq + self.nt)
        self.T = rng.standard_normal((self.nt, 3)).astype(np.float32)
        self.Q = (rng.standard_normal((self.nq, 3)) * 1.3).astype(np.float32)
        self.tm, self.qm = (rng.random(self.nt) < 0.9).astype(np.uint8), (rng.random(self.nq) < 0.9).astype(np.uint8)
        if self.nt > 4:
            self.T[3] = np.nan
            self.Q[min(2, self.nq - 1), 1] = np.inf
        self.dv = [dev(x) for x in (self.Q, self.T, self.qm, self.tm)]
        self.flags = dict(brute=hip.NN_BRUTE, grid=hip.NN_GRID)[path]

    def size(self):
        return self.hip.cloud_nn_workspace(self.nq, self.nt)

    def run(self, ws):
        Q, T, qm, tm = self.dv
        return self.hip.cloud_nn(Q, T, 2.5, qm, tm, flags=self.flags, workspace=ws)

    def launch(self, arena):
        return self.run(arena.payload(U8))

    def reference(self, out):
        want = nn_check.rule(self.Q, self.T, 2.5, self.qm, self.tm)
        eq(out[0], want["index"], "index")
        eq(out[1].view(I32), want["sq_distance"].view(np.int32), "sq_distance")
        eq(out[2], want["stats"], "stats")


@pytest.mark.parametrize("path", ["brute", "grid"])
@pytest.mark.parametrize("counts", NN_SHAPES, ids=ids)
def test_nn_on_exact_guarded_dirty_workspaces(hip, counts, path):
    f = NN(hip, counts, path)
    want = f.run(None)
    sync()
    f.reference(want)
    i = NN_SHAPES.index(counts)
    left = leftover_of(NN(hip, NN_SHAPES[i - 1], "grid" if path == "brute" else "brute")) if i else None   # the OTHER path's leavings
    exact(f.name, f.size(), f.launch, want, leftover=left, what=f"{ids(counts)} {path}")


@pytest.mark.parametrize("path", ["brute", "grid"])
def test_nn_big_small_big_through_one_buffer(hip, path):
    cases = []
    for c in (NN_SHAPES[2], NN_SHAPES[1]):
        f = NN(hip, c, path)
        want = f.run(None)
        sync()
        cases.append((f.size(), f.launch, want))
    big_small_big("g2v_cloud_nn", cases, path)


def test_export_chain_with_one_poisoned_payload_as_every_workspace(hip, tmp_path, monkeypatch):
    """(c) mask -> intrinsics -> consistency -> voxel bounds / assign / reduce -> counts, as save_point_cloud_masked(point_cloud_mask(
    min_views=...), voxel_size=...) runs them back to back, with every workspace the SAME `ones` payload, sized for the largest:
    the PLY bytes are those of the ordinary chain."""
    from g2vlm_amd import g2vlm_utils as U
    shape = (3, 37, 70)
    s = scene(shape)
    d = s["d"]
    pred = dict(points=d["points"][None], local_points=d["local"][None], images=d["colors"][None], camera_poses=d["poses"][None])

    def chain(path):
        mask = U.point_cloud_mask(pred, edge_rtol=0.03, min_views=1, max_in_front=1)
        info = U.save_point_cloud_masked(pred, str(path), mask, verbose=False, voxel_size=VOXEL)
        sync()
        return open(path, "rb").read(), info
    want, info = chain(tmp_path / "ordinary.ply")
    assert info["num_points"] > 0 and info["num_input_points"] > info["num_points"]
    sizes = [hip.intrinsics_lsq_workspace(*shape), hip.cloud_consistency_workspace(*shape), hip.voxel_assign_workspace(*shape),
             hip.voxel_reduce_workspace(shape[0] * shape[1] * shape[2]), hip.cloud_compact_workspace(*shape)]
    arena = Arena(max(sizes), 8, DEV).fill("ones")
    asked = []

    def one_payload(nbytes, device, tag):
        assert nbytes <= arena.nbytes, (tag, nbytes)
        asked.append(tag)
        return arena.payload(U8)
    monkeypatch.setattr(hip, "_cloud_workspace", one_payload)
    got, info2 = chain(tmp_path / "shared.ply")
    monkeypatch.undo()
    assert {"intrinsics", "consistency", "voxel_assign", "voxel_reduce", "compact"} <= set(asked), asked
    arena.check()
    assert info2 == info and got == want


# =============================================================================================== the row kernels with tickets
def tickets_are_zero(t, regions, what):
    b = t.view(U8) if t.dtype == U8 else t.reshape(-1).view(U8)
    for o, n in regions:
        assert not bool(b[o:o + n].any()), f"{what}: a ticket word in bytes [{o}, {o + n}) is not zero after the launch"


ROW_SHAPES = [(1, 151936), (3, 24577), (64, 20000), (600, 40000)]       # the split factor is 19, 4, 3, 1
_ROWS = {}


def row_case(rows, n):
    if (rows, n) not in _ROWS:
        from test_topk_gpu import make_case
        x = make_case(rows, n, n + 24, seed=rows + n)
        g = torch.Generator(device=DEV); g.manual_seed(n)
        t = torch.randint(0, n, (rows,), generator=g, device=DEV, dtype=I32)
        _ROWS[(rows, n)] = (x, t)
    return _ROWS[(rows, n)]


class TopK:
    name = "g2v_topk_rows_bf16"

    def __init__(self, hip, rows, n, k):
        self.hip, self.rows, self.n, self.k = hip, rows, n, k
        self.x, _ = row_case(rows, n)

    def size(self):
        return self.hip.topk_rows_workspace(self.rows, self.n, self.k)

    def run(self, ws):
        idx, val = self.hip.topk_rows_bf16(self.x, self.k, scratch=ws)
        return idx, val

    def launch(self, arena):
        if arena.nbytes == 0:                                # no split would be made: the entry point must not touch the pointer
            lib, x = self.hip.lib(), self.x
            idx = torch.empty((self.rows, self.k), dtype=I32, device=DEV)
            val = torch.empty((self.rows, self.k), dtype=F32, device=DEV)
            rc_ = lib.g2v_topk_rows_bf16(self.hip._p(x), self.rows, self.n, x.stride(0), self.k, self.hip._p(idx), self.hip._p(val), arena.ptr, 0,
                                         self.hip._stream())
            assert rc_ == 0
            return idx, val
        return self.run(arena.payload(I32))

    def reference(self, out):
        from test_topk_gpu import reference
        idx, bits = reference(self.x, self.k)
        assert torch.equal(out[0], idx) and torch.equal(out[1].view(I32), bits)


class LogProb:
    name = "g2v_logprob_rows_bf16"

    def __init__(self, hip, rows, n, k=None):
        import test_logprob_gpu as TL
        self.hip, self.rows, self.n = hip, rows, n
        if ("lp", rows, n) not in _ROWS:
            _ROWS[("lp", rows, n)] = TL.make_case([TL.KINDS[i % len(TL.KINDS)] for i in range(rows)], n, n + 24, seed=rows + n)
        self.x, self.t = _ROWS[("lp", rows, n)]

    def size(self):
        return self.hip.logprob_rows_workspace(self.rows, self.n)

    def run(self, ws):
        lse = torch.empty(self.rows, dtype=F32, device=DEV)
        rank = torch.empty(self.rows, dtype=I32, device=DEV)
        return self.hip.logprob_rows_bf16(self.x, self.t, lse, rank, scratch=ws), lse, rank

    def raw(self, ptr):
        """the C entry point with no scratch bytes: one workgroup per row"""
        lib, x, h = self.hip.lib(), self.x, self.hip
        out, lse = torch.empty(self.rows, dtype=F32, device=DEV), torch.empty(self.rows, dtype=F32, device=DEV)
        rank = torch.empty(self.rows, dtype=I32, device=DEV)
        assert lib.g2v_logprob_rows_bf16(h._p(x), self.rows, self.n, x.stride(0), h._p(self.t), h._p(out), h._p(lse), h._p(rank), ptr, 0,
                                         h._stream()) == 0
        return out, lse, rank

    def launch(self, arena):
        if arena.nbytes == 0:                                # no split would be made: the entry point must not touch the pointer
            return self.raw(arena.ptr)
        return self.run(arena.payload(I32))

    def reference(self, out):
        """The owning test's check against fp64 (its bound), and the header's own promise: a row's results do not depend on the
        launch, so the one-workgroup-per-row launch without scratch gives the same bits."""
        from test_logprob_gpu import check
        check(self.hip, self.x, self.t, f"scratch {self.rows}x{self.n}")
        alone = self.raw(None)
        sync()
        assert sc.first_difference(out, alone) is None, sc.first_difference(out, alone)


def ticket_case(cls, hip, rows, n, k):
    f = cls(hip, rows, n, k)
    want = f.run(None)
    sync()
    return f, want


@pytest.mark.parametrize("rows,n", ROW_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("cls,k", [(TopK, 1), (TopK, 32), (LogProb, None)], ids=["topk1", "topk32", "logprob"])
def test_row_kernels_on_exact_guarded_dirty_scratch(hip, cls, k, rows, n):
    f, want = ticket_case(cls, hip, rows, n, k)
    f.reference(want)
    nbytes = f.size()
    zero = CONTRACTS[f.name].tickets(nbytes)
    i = ROW_SHAPES.index((rows, n))
    left = None
    if nbytes and i:                                         # another shape's partial lists, left in the first bytes that it needs
        other = cls(hip, *ROW_SHAPES[i - 1], k)
        if 0 < other.size() <= nbytes:
            left = lambda arena: other.run(arena.head(other.size(), I32))     # noqa: E731
    exact(f.name, nbytes, f.launch, want, zero=zero, leftover=left, what=f"{rows}x{n} k={k}")


@pytest.mark.parametrize("cls,k", [(TopK, 1), (TopK, 32), (LogProb, None)], ids=["topk1", "topk32", "logprob"])
def test_row_kernels_carry_one_scratch_through_every_split(hip, cls, k):
    """large split -> small split -> no split -> large split on ONE scratch, zeroed once: every launch equals the same launch on
    fresh scratch and leaves the 512 ticket words zero."""
    seq = [ROW_SHAPES[0], ROW_SHAPES[2], ROW_SHAPES[3], ROW_SHAPES[1], ROW_SHAPES[0]]
    cases = [ticket_case(cls, hip, r, n, k) for r, n in seq]
    nbytes = max(f.size() for f, _ in cases)
    name = cases[0][0].name
    arena = Arena(nbytes, 4, DEV).fill("ones", zero=CONTRACTS[name].tickets(nbytes))
    for step, (f, want) in enumerate(cases):
        got = f.run(arena.payload(I32))
        sync()
        assert sc.first_difference(got, want) is None, (name, step, seq[step], sc.first_difference(got, want))
        tickets_are_zero(arena.payload(), CONTRACTS[name].tickets(nbytes), f"{name} step {step} {seq[step]}")
        arena.check()


ARGMAX_N = [65535, 65536, 151936]                            # one workgroup per row below 65536, 64 from there on
ARGMAX_ROWS = [1, 5, 64]


def argmax_inputs(rows, n):
    g = torch.Generator(device=DEV); g.manual_seed(rows * 7 + n)
    x = torch.randn((rows, n + 8), generator=g, device=DEV).bfloat16()
    x[:, n:] = float("inf")                                  # the pad columns must never win
    return x[:, :n]


def argmax_runs(hip, entry, x, seed=0x1234567890ABCDEF, T=0.7):
    rows = x.shape[0]

    def run(arena):
        out = torch.full((rows,), -1, dtype=I32, device=DEV)
        scr = arena.payload(I32) if arena is not None else torch.zeros(rows * 129, dtype=I32, device=DEV)
        if entry == "g2v_argmax_bf16":
            hip.lib().g2v_argmax_bf16(hip._p(x), x.shape[1], hip._p(out), hip._p(scr), hip._stream())
        elif entry == "g2v_argmax_rows_bf16":
            hip.argmax_rows_bf16(x, out, scr)
        else:
            hip.sample_rows_bf16(x, out, scr, hip.make_rng(seed, T, DEV))
        return (out,)
    return run


def argmax_reference(entry, x, out, seed=0x1234567890ABCDEF, T=0.7):
    got = out[0].cpu().tolist()
    if entry == "g2v_sample_rows_bf16":
        from test_imageops_fp64_gpu import sample_ok         # the owning test's comparison of a Gumbel-max draw
        xc = x.float().cpu().numpy()
        for r, gtok in enumerate(got):
            assert 0 <= gtok < x.shape[1] and sample_ok(xc[r], float(np.float32(1.0 / T)), seed, 0, r, gtok), (r, gtok)
    else:
        assert got == I.argmax_ref(x).tolist()


ARGMAX_CASES = [(e, r, n) for e in ("g2v_argmax_bf16", "g2v_argmax_rows_bf16", "g2v_sample_rows_bf16") for r in ARGMAX_ROWS for n in ARGMAX_N
                if r == 1 or e != "g2v_argmax_bf16"]          # g2v_argmax_bf16 takes one row


@pytest.mark.parametrize("entry,rows,n", ARGMAX_CASES, ids=lambda v: str(v))
def test_argmax_and_sample_on_exact_guarded_dirty_scratch(hip, entry, rows, n):
    x = argmax_inputs(rows, n)
    run = argmax_runs(hip, entry, x)
    want = run(None)
    sync()
    argmax_reference(entry, x, want)
    other = argmax_runs(hip, entry, argmax_inputs(rows, ARGMAX_N[ARGMAX_N.index(n) - 1]))       # the other workgroup count's leavings
    exact(entry, rows * 129 * 4, run, want, zero=CONTRACTS[entry].tickets(rows), leftover=lambda a: other(a), what=f"{rows}x{n}")


@pytest.mark.parametrize("entry", ["g2v_argmax_bf16", "g2v_argmax_rows_bf16", "g2v_sample_rows_bf16"])
def test_argmax_and_sample_carry_one_scratch_through_every_shape(hip, entry):
    """64 workgroups per row -> one -> 64, and 64 rows -> 5 -> 1 -> 64 rows, on ONE scratch zeroed once: every launch equals the
    launch on fresh scratch and every row's ticket word is zero afterwards."""
    many = 1 if entry == "g2v_argmax_bf16" else 64
    seq = [(many, 151936), (min(many, 5), 65535), (1, 65536), (many, 65535), (many, 151936)]
    arena = Arena(many * 129 * 4, 4, DEV).fill("ones", zero=CONTRACTS[entry].tickets(many))

    class Head:
        def __init__(self, rows):
            self.rows = rows

        def payload(self, dtype):
            return arena.head(self.rows * 129 * 4, dtype)
    for step, (rows, n) in enumerate(seq):
        x = argmax_inputs(rows, n)
        run = argmax_runs(hip, entry, x)
        want = run(None)
        got = run(Head(rows))
        sync()
        assert sc.first_difference(got, want) is None, (entry, step, rows, n)
        tickets_are_zero(arena.payload(), CONTRACTS[entry].tickets(many), f"{entry} step {step}")
        arena.check()


# =============================================================================================== decode attention
HQ, HKV, CAP = 12, 2, 512
DECODE_LENS = {1: [[1], [64], [65], [449]], 3: [[1, 64, 65], [449, 65, 64]]}
SCALE = 128 ** -0.5


def gen1_step(hip, lens, seed):
    from test_decode_fp64_gpu import make_step
    return make_step(hip, lens, HQ, HKV, seed, max_len=CAP)


def gen1_reference(s, out):
    """every slot against fp64 attention under the owning test's comparison (assert_bf16_close, ulps = 1.01)"""
    from test_decode_fp64_gpu import assert_bf16_close
    qc, kc, vc = s["qn"].cpu(), s["k_ref"].cpu(), s["v_ref"].cpu()
    for z, n in enumerate(s["lens"]):
        want = D.attention64(qc[z].view(HQ, 128), kc[z, :n], vc[z, :n], HKV)
        assert_bf16_close(out[z].view(HQ, 128), want.bfloat16(), ulps=1.01)


GEN1 = ["g2v_decode_attn", "g2v_decode_attn_dyn", "g2v_decode_attn_batch", "g2v_decode_attn_fused"]


def gen1_case(hip, entry, lens, seed):
    """(nbytes, run(arena or None), reference) of one first-generation entry point on one step"""
    s = gen1_step(hip, lens, seed)
    B, rows = len(lens), s["rows"]
    qn, k, v = s["qn"], s["k_ref"], s["v_ref"]
    one = entry in ("g2v_decode_attn", "g2v_decode_attn_dyn")
    if entry == "g2v_decode_attn":
        nbytes = hip.decode_attn_workspace(lens[0], HQ)
    elif entry == "g2v_decode_attn_dyn":
        nbytes = hip.decode_attn_workspace(CAP, HQ)
    else:
        nbytes = B * hip.decode_attn_workspace(CAP, HQ)

    def run(arena):
        ws = arena.payload(F32) if arena is not None else torch.empty(nbytes // 4, dtype=F32, device=DEV)
        out = D.nan_bf16(B, HQ * 128)
        if entry == "g2v_decode_attn":
            hip.decode_attn(qn[0].view(HQ, 128), k[0], v[0], out.view(HQ, 128), lens[0], HQ, HKV, SCALE, ws)
        elif entry == "g2v_decode_attn_dyn":
            hip.decode_attn_dyn(qn[0].view(HQ, 128), k[0], v[0], out.view(HQ, 128), s["ld"][:1], CAP, HQ, HKV, SCALE, ws)
        elif entry == "g2v_decode_attn_batch":
            hip.decode_attn_batch(qn, k, v, out, s["ld"], rows, CAP, HQ, HKV, SCALE, ws)
        else:
            kc, vc = s["kc"].clone(), s["vc"].clone()        # the step's own cache: the new rows are appended by this call
            hip.decode_attn_fused(s["qkv"], s["qw"], s["kw"], 1e-6, 1, s["cos"], s["sin"], kc, vc, out, s["ld"], rows, CAP, HQ, HKV, SCALE, ws)
            return out, kc, vc
        return (out,)
    assert not one or B == 1
    return nbytes, run, lambda out: gen1_reference(s, out[0])


def decode_cases(entry):
    return [(B, lens) for B in ((1,) if entry in ("g2v_decode_attn", "g2v_decode_attn_dyn") else (1, 3)) for lens in DECODE_LENS[B]]


@pytest.mark.parametrize("entry", GEN1)
def test_first_generation_decode_attention_on_exact_guarded_dirty_workspaces(hip, entry):
    prev = None
    for i, (B, lens) in enumerate(decode_cases(entry)):
        nbytes, run, reference = gen1_case(hip, entry, lens, seed=40 + i)
        want = run(None)
        sync()
        reference(want)
        left = None
        if prev is not None and prev[0] <= nbytes:
            left = (lambda p: lambda arena: p[1](_Head(arena, p[0])))(prev)
        exact(entry, nbytes, run, want, leftover=left, fp32=True, what=f"B {B} lens {lens}")
        prev = (nbytes, run)


class _Head:
    """the first nbytes of an arena's payload as a workspace of its own"""

    def __init__(self, arena, nbytes):
        self.arena, self.nbytes = arena, nbytes

    def payload(self, dtype=U8):
        return self.arena.head(self.nbytes, dtype)


def pg_case(hip, kind, lens, seed):
    """(name, nbytes, run, reference) for g2v_decode_attn_pg / _pg_kv8 on one step of capacity 512"""
    B = len(lens)
    nbytes = hip.decode_attn_pg_workspace(HQ, HKV, B)
    if kind == "pg":
        import test_decode_fp64_gpu as T
        base = T.make_step(hip, lens, HQ, HKV, seed, max_len=CAP)

        def run(arena):
            s = dict(base, kc=base["kc"].clone(), vc=base["vc"].clone())
            out = T.run_pg(hip, s, HQ, HKV, ws=None if arena is None else arena.payload(F32))
            return out, s["kc"], s["vc"]

        def reference(out):
            assert torch.equal(T.bits(out[1]), T.bits(base["k_ref"])) and torch.equal(T.bits(out[2]), T.bits(base["v_ref"]))
            T.check_against_fp64("attn_pg scratch", base, out[0], HQ, HKV)
        return "g2v_decode_attn_pg", nbytes, run, reference
    import test_kv8_gpu as T8
    base = T8.make_step(hip, lens, HQ, HKV, seed, cap=CAP)

    def run8(arena):
        s = dict(base, **{n: base[n].clone() for n in ("kc", "vc", "ks", "vs")})
        out = T8.run_kv8(hip, s, HQ, HKV, ws=None if arena is None else arena.payload(F32))
        return out, s["kc"], s["vc"], s["ks"], s["vs"]

    def reference8(out):
        """the owning test's whole check (appended codes and scales, fp64 attention over the dequantised cache, the bf16 kernel) of
        this very step: its make_step at this capacity, and its launch's output must be the ordinary run's"""
        seen, make, launch = [], T8.make_step, T8.run_kv8
        T8.make_step = lambda h, ln, hq, hkv, sd: make(h, ln, hq, hkv, sd, cap=CAP)
        T8.run_kv8 = lambda *a, **k: seen.append(launch(*a, **k)) or seen[-1]
        try:
            T8.check_step(hip, lens, HQ, HKV, seed)
        finally:
            T8.make_step, T8.run_kv8 = make, launch
        assert len(seen) == 1 and sc.same_bits(seen[0], out[0])
    return "g2v_decode_attn_pg_kv8", nbytes, run8, reference8


@pytest.mark.parametrize("kind", ["pg", "pg_kv8"])
def test_persistent_grid_decode_attention_on_exact_guarded_dirty_workspaces(hip, kind):
    prev = None
    for i, (B, lens) in enumerate(decode_cases("pg")):
        name, nbytes, run, reference = pg_case(hip, kind, lens, seed=60 + i)
        want = run(None)
        sync()
        reference(want)
        left = (lambda p: lambda arena: p[1](_Head(arena, p[0])))(prev) if prev is not None and prev[0] <= nbytes else None
        exact(name, nbytes, run, want, leftover=left, fp32=True, what=f"B {B} lens {lens}")
        prev = (nbytes, run)


PREFIX, SUFFIXES, SMAX = 300, [1, 65], 320                   # a prefix of 300 rows, suffixes of 1 and 65 in the owning test's 320-row blocks


def shared_case(hip, B, seed, monkeypatch):
    import test_shared_prefix_gpu as TS
    monkeypatch.setattr(TS, "SUFFIX", SUFFIXES)          # the suffix lengths the owning test's make_step deals out
    assert TS.SMAX == SMAX
    base = TS.make_step(hip, B, PREFIX, HQ, HKV, seed, smax=SMAX)
    nbytes = hip.decode_attn_shared_workspace(HQ, HKV, B, PREFIX, SMAX)

    def run(arena):
        s = dict(base, ks=base["ks"].clone(), vs=base["vs"].clone())
        out = torch.full((B, HQ * 128), float("nan"), dtype=torch.bfloat16, device=DEV)
        ws = arena.payload(F32) if arena is not None else torch.empty(nbytes // 4, dtype=F32, device=DEV)
        hip.decode_attn_shared(s["qkv"], s["qw"], s["kw"], 1e-6, 1, s["cos"], s["sin"], s["kp"], s["vp"], PREFIX, s["ks"], s["vs"], s["ld"],
                               SMAX, SMAX, HQ, HKV, SCALE, out, ws)
        return out, s["ks"], s["vs"]
    return TS, nbytes, run


@pytest.mark.parametrize("B", [1, 3])
def test_shared_prefix_decode_attention_on_exact_guarded_dirty_workspaces(hip, B, monkeypatch):
    TS, nbytes, run = shared_case(hip, B, PREFIX + 7 * B + HQ, monkeypatch)
    TS.check_shared(hip, HQ, HKV, B, PREFIX)                 # the owning test's check of this step (it derives the same seed)
    want = run(None)
    sync()
    assert torch.isfinite(want[0].float()).all()
    exact("g2v_decode_attn_shared", nbytes, run, want, fp32=True, what=f"B {B}",
          leftover=(lambda arena: shared_case(hip, 1, 5, monkeypatch)[2](_Head(arena, hip.decode_attn_shared_workspace(HQ, HKV, 1, PREFIX, SMAX))))
          if B > 1 else None)


@pytest.mark.parametrize("entry", ["g2v_decode_attn_batch", "g2v_decode_attn_fused", "pg", "pg_kv8", "shared"])
def test_decode_attention_big_small_big_through_one_buffer(hip, entry, monkeypatch):
    cases = []
    for lens in ([449, 65, 64], [65]):
        if entry in ("pg", "pg_kv8"):
            name, nbytes, run, _ = pg_case(hip, entry, lens, seed=81)
        elif entry == "shared":
            name = "g2v_decode_attn_shared"
            _, nbytes, run = shared_case(hip, len(lens), 82, monkeypatch)
        else:
            name = entry
            nbytes, run, _ = gen1_case(hip, entry, lens, seed=83)
        want = run(None)
        sync()
        cases.append((nbytes, run, want))
    big_small_big(name, cases)


def test_length_by_value_decode_attention_big_small_big_through_one_buffer(hip):
    for entry in ("g2v_decode_attn", "g2v_decode_attn_dyn"):
        cases = []
        for lens in ([449], [65]):
            nbytes, run, _ = gen1_case(hip, entry, lens, seed=84)
            want = run(None)
            sync()
            cases.append((nbytes, run, want))
        if entry == "g2v_decode_attn":
            assert cases[1][0] < cases[0][0]
        big_small_big(entry, cases)


# =============================================================================================== flash attention
def flash_inputs(Lq, tot, seed):
    import flash_profile_check as FP
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    r = lambda *shape: torch.randn(shape, generator=g, device=DEV)     # noqa: E731
    return FP.padded_inputs(Lq, tot, 12, 2, 128, r(Lq, 12 * 128), r(tot, 2 * 128), r(tot, 2 * 128))


def flash_plans(hip):
    """name -> (windows, plan, attn form): the smallest plans with partial slots at tile_rows 128 and 256, one with fewer slots, one
    with none, and the two-phase plan of a view-sharded rank (test_c4_rank_phases' windows at a small size)."""
    import flash_profile_check as FP
    Lq, tot, r0 = 150, 700, 200
    whole = [(FP.Q0, Lq, FP.K0, tot, False)]
    phases = [(FP.Q0, Lq, FP.K0 + r0, Lq, False, 0), (FP.Q0, Lq, FP.K0, r0, False, 1), (FP.Q0, Lq, FP.K0 + r0 + Lq, tot - r0 - Lq, False, 1)]
    mk = lambda w, mb, tr: hip.make_attn_plan(w, 12, DEV, max_blocks=mb, tile_rows=tr)     # noqa: E731
    # slots at these sizes (the host's schedule): 128-row items 50 / 22 / 8 / 0 at max_blocks 29 / 13 / 23 / 7, 256-row items 8 and 12
    plans = {"128 mb23": (whole, mk(whole, 23, 128), 1), "256 mb11": (whole, mk(whole, 11, 256), 1), "256 mb7 8w": (whole, mk(whole, 7, 256), 0),
             "128 mb29": (whole, mk(whole, 29, 128), 1), "128 mb13": (whole, mk(whole, 13, 128), 1), "128 none": (whole, mk(whole, 7, 128), 1),
             "256 phases": (phases, mk(phases, None, 256), 1)}
    slots = {n: p[1].n_slots for n, p in plans.items()}
    assert slots["128 mb29"] > slots["128 mb13"] > slots["128 mb23"] > 0 == slots["128 none"] and slots["256 mb11"] > 0, slots
    assert slots["256 phases"] > 0 and len(plans["256 phases"][1].phases) == 2 and slots["256 mb7 8w"] > 0, slots
    return (Lq, tot), plans


def flash_run(hip, q, k, v, windows, plan, form, ws, phase_by_phase=False):
    import flash_profile_check as FP
    owner = hip.scratch_owner(torch.cuda.current_device())
    saved = plan._by_owner.get(owner)
    if ws is not None:
        plan._by_owner[owner] = ws                           # the payload in place of plan.ws(owner)'s own tensor
    try:
        with FP.attn_form(hip, form):
            return (FP.launch(hip, q, k, v, plan, 12, 2, 128, windows, q.shape[0], 12 * 128 + 36, phase_by_phase=phase_by_phase).clone(),)
    finally:
        if saved is None:
            plan._by_owner.pop(owner, None)
        else:
            plan._by_owner[owner] = saved


def test_flash_attention_on_exact_guarded_dirty_workspaces(hip):
    import flash_profile_check as FP
    from test_attention_gpu import Errors, check_bounds
    (Lq, tot), plans = flash_plans(hip)
    q, k, v = flash_inputs(Lq, tot, seed=9)
    small = plans["128 mb23"]
    for name, (windows, plan, form) in plans.items():
        want = flash_run(hip, q, k, v, windows, plan, form, None)
        sync()
        check_bounds(Errors(want[0], FP.ref_fp64(q, k, v, windows, 12, 2, 128), 12, 128), 128, f"scratch {name}")
        nbytes = int(hip.lib().g2v_flash_attn_workspace(plan.n_slots))
        run = lambda arena, a=(windows, plan, form): flash_run(hip, q, k, v, *a, arena.payload(F32), phase_by_phase=len(a[1].phases) > 1)   # noqa: E731
        left = None
        if plan is not small[1] and 0 < small[1].n_slots * 256 * 130 * 4 <= nbytes:
            left = lambda arena: flash_run(hip, q, k, v, *small, arena.head(small[1].n_slots * 256 * 130 * 4, F32))     # noqa: E731
        if nbytes:
            exact("g2v_flash_attn", nbytes, run, want, leftover=left, fp32=True, what=name)


def test_flash_attention_plans_share_one_workspace(hip):
    """One workspace, sized for the plan with the most slots, serves that plan, a plan with fewer slots, a plan with none, the
    two-phase plan launched phase by phase, and the first again: every launch equals its launch on its own workspace."""
    (Lq, tot), plans = flash_plans(hip)
    q, k, v = flash_inputs(Lq, tot, seed=10)
    seq = ["128 mb29", "128 mb13", "128 none", "256 phases", "256 mb11", "128 mb29"]
    nbytes = max(int(hip.lib().g2v_flash_attn_workspace(plans[n][1].n_slots)) for n in seq)
    arena = Arena(nbytes, 16, DEV).fill("nan")
    for step, name in enumerate(seq):
        windows, plan, form = plans[name]
        want = flash_run(hip, q, k, v, windows, plan, form, None)
        got = flash_run(hip, q, k, v, windows, plan, form, arena.payload(F32), phase_by_phase=len(plan.phases) > 1)
        sync()
        assert sc.first_difference(got, want) is None, (step, name)
        arena.check()


# =============================================================================================== the skinny GEMM's K split
GEMM_SHAPES = [(8, 1536, 8960), (40, 1536, 4096), (8, 256, 640)]        # the first two split K across workgroups, the third does not
GEMM_BYTES = [64 << 10, 1 << 20, 8 << 20]


def gemm_launch(hip, shape, seed):
    from test_gemm_fp64_gpu import Launch
    M, N, K = shape
    return Launch(hip, G.EPI_BF16, [M], N, K, lda_pad=64, seed=seed)


@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=ids)
def test_skinny_gemm_on_exact_guarded_dirty_workspaces(hip, shape):
    L = gemm_launch(hip, shape, seed=7)
    route0 = L.route()
    L.run()
    L.check("skinny", (route0[1], 16), f"scratch {shape} ordinary {route0}")
    want = (L.output(),)
    big = 8 << 20
    assert route0[0] == "skinny" and (route0[3] > 1) == (shape != GEMM_SHAPES[2]), route0
    for nbytes in GEMM_BYTES:
        route = L.route(ws=torch.zeros(nbytes // 4, dtype=I32, device=DEV))
        assert nbytes > (64 << 10) or route[3] == 1, route    # nothing but tickets fits: the split stays inside the workgroup

        def run(arena):
            L.run(ws=arena.payload(I32))
            if route[2:] != route0[2:]:                       # another (S, KS): another summation order, the owning module's bound
                L.check("skinny", (route[1], 16), f"scratch {shape} ws {nbytes} {route}")
                return want
            return (L.output(),)

        def other(arena):                                     # another shape's tickets (reset) and partials
            gemm_launch(hip, GEMM_SHAPES[1] if shape == GEMM_SHAPES[0] else GEMM_SHAPES[0], seed=8).run(ws=arena.payload(I32))
        stages = exact("g2v_gemm_bf16", nbytes, run, want, zero=CONTRACTS["g2v_gemm_bf16"].tickets(nbytes), leftover=other,
                       what=f"{shape} ws {nbytes} route {route}")
        assert len(stages) == 3 and big >= nbytes


def test_skinny_gemm_carries_one_workspace_through_every_split(hip):
    """large split -> small split -> no split -> large split on ONE workspace zeroed once: equal to the launch on a fresh
    workspace of the same size, and the 64 KiB of tickets all zero after every launch."""
    nbytes = 1 << 20
    arena = Arena(nbytes, 4, DEV).fill("ones", zero=CONTRACTS["g2v_gemm_bf16"].tickets(nbytes))
    seq = [GEMM_SHAPES[0], GEMM_SHAPES[1], GEMM_SHAPES[2], GEMM_SHAPES[0]]
    splits = []
    for step, shape in enumerate(seq):
        L = gemm_launch(hip, shape, seed=20 + step)
        fresh = torch.zeros(nbytes // 4, dtype=I32, device=DEV)
        splits.append(L.route(ws=fresh)[3])
        L.run(ws=fresh)
        L.check("skinny", (L.route(ws=fresh)[1], 16), f"carry {shape}")
        want = L.output()
        L.run(ws=arena.payload(I32))
        assert sc.same_bits(L.output(), want), (step, shape)
        tickets_are_zero(arena.payload(), CONTRACTS["g2v_gemm_bf16"].tickets(nbytes), f"gemm step {step} {shape}")
        arena.check()
    assert splits[0] > 1 and splits[1] > 1 and splits[2] == 1, splits


# =============================================================================================== the resize's staging buffer
def test_lanczos_tmp_is_exact_guarded_and_dirty(hip):
    """g2v_lanczos_resize_u8's tmp u8 [N, Hin, Wout, 3] through the C entry point: the wrapper's own run is PIL's resize (bit-exact,
    tests/test_imageops_fp64_gpu.py holds it to that), the payload runs equal it."""
    from PIL import Image
    from g2vlm_amd import host
    N, H, W, OH, OW = 2, 37, 53, 28, 42
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    want = hip.lanczos_resize_u8(dev(frames), OH, OW)
    sync()
    for i in range(N):
        assert np.array_equal(want[i].cpu().numpy(), np.asarray(Image.fromarray(frames[i]).resize((OW, OH), Image.LANCZOS)))
    tabs = [tuple(hip.h2d(t, torch.device(DEV)) for t in host.lanczos_tables(a, b)) for a, b in ((W, OW), (H, OH))]
    src = dev(frames)

    def run(arena):
        out = torch.empty((N, OH, OW, 3), dtype=U8, device=DEV)
        (bh, kh), (bv, kv) = tabs
        rc_ = hip.lib().g2v_lanczos_resize_u8(hip._p(src), N, H, W, hip._p(out), OH, OW, arena.ptr, hip._p(bh), hip._p(kh), kh.shape[1],
                                              hip._p(bv), hip._p(kv), kv.shape[1], hip._stream())
        assert rc_ == 0
        return (out,)
    exact("g2v_lanczos_resize_u8", N * H * OW * 3, run, (want,), leftover=lambda a: a.payload()[::3].fill_(0xEE), what="2x37x53 -> 28x42")


# =============================================================================================== nothing left out
def test_every_row_of_the_table_was_run(hip):
    """runs last in this module: with the whole module selected, every entry point of CONTRACTS went through exact()"""
    if len(COVERED) < 3:                                     # a selection (-k) of this module: nothing to say
        return
    assert sorted(COVERED) == sorted(CONTRACTS), sorted(set(CONTRACTS) - COVERED)
