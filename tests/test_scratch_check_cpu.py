"""CPU (no GPU): tests/scratch_check.py itself - the table of scratch contracts against include/g2vlm_hip.h, the Arena against
planted faults on CPU tensors, and the workspace queries of the built library against the closed forms the header states.

1. CONTRACTS has exactly the entry points of the header that take a workspace, scratch or tmp argument (g2v_gemm_bf16 takes its
   workspace in g2v_gemm_desc): a kernel cannot be added without a row.
2. The Arena: a write one byte behind the payload, and one byte in front of it, are each reported at that offset; the payload
   has the exact size at exactly the demanded alignment; a planted kernel that reads a word before writing it changes its output
   under `ones` and not under `zeros`, and the staged runner then leaves the more hostile patterns alone.
3. The size queries (pure host calls) against the header's formulas over a sweep of small shapes."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import scratch_check as sc  # noqa: E402
from g2vlm_amd import hip  # noqa: E402


# ------------------------------------------------------------------------------------------------ 1. the table
def test_contracts_cover_exactly_the_scratch_taking_entry_points_of_the_header():
    found = sc.header_scratch_entry_points()
    assert len(found) >= 24 and "g2v_cloud_nn" in found and "g2v_lanczos_resize_u8" in found and found["g2v_gemm_bf16"] == "g2v_gemm_desc"
    assert "g2v_gemm_route" not in found and "g2v_cloud_normals" not in found and "g2v_cloud_mask" not in found
    assert sorted(sc.CONTRACTS) == sorted(found), (sorted(set(found) - set(sc.CONTRACTS)), sorted(set(sc.CONTRACTS) - set(found)))
    for name, via in found.items():
        assert sc.CONTRACTS[name].via_struct == via, name


def test_every_row_is_complete_and_its_query_is_exported():
    protos = sc.header_entry_points()
    for name, c in sc.CONTRACTS.items():
        assert c.kind in ("uninit_ok", "zero_once") and c.align in (1, 4, 8, 16) and c.size_doc, name
        assert (c.kind == "zero_once") == (c.ticket_doc is not None), name
        if c.query is not None:
            assert c.query in protos and c.query in hip.EXPORTS, (name, c.query)
        assert "nan" not in sc.patterns_for(name) and ("nan" in sc.patterns_for(name, fp32=True)) == (c.kind == "uninit_ok" and c.dtype == torch.float32)
    assert sc.patterns_for("g2v_cloud_nn") == ("zeros", "ones", "leftover")
    assert sc.patterns_for("g2v_decode_attn_pg", fp32=True) == sc.PATTERNS
    # the ticket words the header documents
    assert sc.CONTRACTS["g2v_argmax_rows_bf16"].tickets(3) == [(0, 4), (516, 4), (1032, 4)]
    assert sc.CONTRACTS["g2v_topk_rows_bf16"].tickets(4096) == [(0, 2048)] and sc.CONTRACTS["g2v_logprob_rows_bf16"].tickets(0) == []
    assert sc.CONTRACTS["g2v_gemm_bf16"].tickets(1 << 20) == [(0, 65536)]


# ------------------------------------------------------------------------------------------------ 2. the Arena
@pytest.mark.parametrize("align", [1, 4, 8, 16])
@pytest.mark.parametrize("nbytes", [0, 4, 13, 72, 4100])
def test_payload_has_the_exact_size_at_exactly_the_alignment(align, nbytes):
    if nbytes % align:
        nbytes -= nbytes % align
    a = sc.Arena(nbytes, align)
    p = a.payload()
    assert p.numel() == nbytes and p.dtype == torch.uint8
    assert a.ptr % align == 0 and a.ptr % (2 * align) != 0
    if nbytes:
        assert p.data_ptr() == a.ptr
    assert a.off >= sc.GUARD_BYTES and a.buf.numel() - (a.off + nbytes) >= sc.GUARD_BYTES
    assert a.damage() is None
    a.check()
    if align >= 4 and nbytes:
        assert a.payload(torch.int32).numel() == nbytes // 4 and a.payload(torch.int32).data_ptr() == a.ptr


def test_a_write_one_byte_past_or_before_the_payload_is_reported_at_its_offset():
    for align, nbytes in ((4, 60), (16, 1040), (8, 0)):
        a = sc.Arena(nbytes, align).fill("zeros")
        a.buf[a.off + nbytes] = 0                            # one byte past
        d = a.damage()
        assert d is not None and f"payload offset {nbytes} " in d and "1 bytes damaged" in d, d
        with pytest.raises(AssertionError, match=f"payload offset {nbytes} "):
            a.check()
        a = sc.Arena(nbytes, align).fill("ones")
        a.buf[a.off - 1] = 7                                 # one byte before
        d = a.damage()
        assert d is not None and "payload offset -1 " in d and "is 0x07" in d, d
        a = sc.Arena(nbytes, align).fill("nan")              # the far ends of both guards
        a.buf[0] = 1
        assert "payload offset %d " % -a.off in a.damage()
        a = sc.Arena(nbytes, align)
        a.buf[-1] = 1
        assert "payload offset %d " % (a.buf.numel() - 1 - a.off) in a.damage()


def test_fill_patterns_and_ticket_words():
    a = sc.Arena(24, 4).fill("ones")
    assert a.payload(torch.int32).tolist() == [1] * 6
    a.fill("ones", zero=[(0, 8)])
    assert a.payload(torch.int32).tolist() == [0, 0, 1, 1, 1, 1]
    a.fill("nan", zero=[(4, 4)])
    assert a.payload(torch.int32).tolist() == [-1, 0, -1, -1, -1, -1] and bool(torch.isnan(a.payload(torch.float32)[0]))
    a.fill("leftover")
    assert a.payload(torch.int32).tolist() == [-1, 0, -1, -1, -1, -1]
    a.fill("zeros")
    assert a.payload(torch.int32).tolist() == [0] * 6 and a.damage() is None
    with pytest.raises(AssertionError):
        a.fill("zeros", zero=[(20, 8)])                      # a ticket region that leaves the payload is a bug of the table
    odd = sc.Arena(7, 1).fill("ones")
    assert odd.payload().tolist() == [1, 0, 0, 0, 1, 0, 0]


def test_a_small_launch_inside_a_big_buffer_must_leave_the_rest_alone():
    a = sc.Arena(64, 8).fill("ones")
    snap = a.snapshot()
    a.head(16, torch.int32).fill_(5)                         # the small launch's own 16 bytes
    assert a.damage(keep_from=16, snapshot=snap) is None
    a.payload()[16] = 9                                      # ... and one byte more
    d = a.damage(keep_from=16, snapshot=snap)
    assert d is not None and "payload offset 16 " in d and "was 0x01, is 0x09" in d


def _planted(reads_before_writing):
    """a 'kernel' with a 4-word int32 workspace: it sums x through word 0; the faulty one forgets to clear the word first"""
    x = torch.arange(1, 9, dtype=torch.int32)

    def run(arena):
        w = arena.payload(torch.int32)
        if not reads_before_writing:
            w[0] = 0
        for v in x.tolist():
            w[0] += v
        w[1] = w[0] * 2
        return (w[:2].clone(),)
    return run


def test_pattern_staging_means_something():
    want = (torch.tensor([36, 72], dtype=torch.int32),)
    good = sc.staged("g2v_cloud_compact", 16, _planted(False), want, sc.patterns_for("g2v_cloud_compact"), device="cpu")
    assert [(s.pattern, s.status) for s in good] == [("zeros", "ok"), ("ones", "ok"), ("leftover", "not applicable")]
    sc.assert_staged("g2v_cloud_compact", good)
    bad = sc.staged("g2v_cloud_compact", 16, _planted(True), want, sc.PATTERNS, device="cpu", leftover=lambda a: None)
    assert [(s.pattern, s.status) for s in bad] == [("zeros", "ok"), ("ones", "FAILED"), ("leftover", "not run"), ("nan", "not run")]
    assert "ones failed first" in bad[2].detail and "output 0" in bad[1].detail
    with pytest.raises(AssertionError, match="ones: FAILED"):
        sc.assert_staged("g2v_cloud_compact", bad)

    def overrun(arena):                                      # right answer, one word too far
        arena.buf[arena.off + 16:arena.off + 20] = 0
        return want
    over = sc.staged("g2v_cloud_compact", 16, overrun, want, ("zeros", "ones"), device="cpu")
    assert over[0].status == "FAILED" and "payload offset 16 " in over[0].detail and over[1].status == "not run"


def test_leftover_runs_the_other_shape_first_and_keeps_the_tickets_it_reset():
    seen = []

    def other(arena):
        seen.append(arena.payload(torch.int32).tolist())
        arena.head(8, torch.int32).fill_(3)

    def run(arena):
        seen.append(arena.payload(torch.int32).tolist())
        return ()
    st = sc.staged("g2v_topk_rows_bf16", 16, run, (), ("leftover",), zero=[(0, 4)], leftover=other, device="cpu")
    assert st == [sc.Stage("leftover", "ok", "")] and seen == [[0, 1, 1, 1], [3, 3, 1, 1]]


def test_same_bits_tells_nan_payloads_and_signed_zeros_apart():
    a = torch.tensor([0.0, float("nan")])
    b = a.clone()
    assert sc.same_bits(a, b) and sc.first_difference((a, None), (b, None)) is None
    b[0] = -0.0
    assert not sc.same_bits(a, b) and "output 0: 1 bytes differ, the first at byte 3" in sc.first_difference((a,), (b,))
    c = a.clone().view(torch.int32)
    c[1] ^= 1
    assert not sc.same_bits(a, c.view(torch.float32)) and not sc.same_bits(a, a.double()) and not sc.same_bits(a, None)


# ------------------------------------------------------------------------------------------------ 3. the size queries
@pytest.fixture(scope="module")
def lib():
    from g2vlm_amd import build
    lib = C.CDLL(build.build())
    for name in sorted({c.query for c in sc.CONTRACTS.values() if c.query}):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = hip._SIGS[name]
    return lib


SHAPES = [(1, 1, 1), (1, 32, 32), (1, 32, 33), (2, 9, 13), (3, 37, 70), (1, 513, 512), (5, 1, 1025), (2, 518, 518)]


def _cells(nt):                                              # the largest G with G^3 <= 2 Nt, in [1, 256]
    g = 1
    while g < 256 and (g + 1) ** 3 <= 2 * nt:
        g += 1
    return g ** 3


def test_queries_equal_the_formulas_the_header_states(lib):
    for nq in (0, 1, 255, 5000):
        for nt in (0, 1, 3, 4, 13, 1025, 3000, 70000):
            g3 = _cells(nt)
            assert lib.g2v_cloud_nn_workspace(nq, nt) == 256 + 24 * nt + 8 * nq + 4 * (g3 + 1) + 4 * -(-g3 // 1024), (nq, nt)
    for n, h, w in SHAPES:
        blocks = -(-(h * w) // 1024)
        assert lib.g2v_cloud_render_workspace(n, h, w) == 8 * n * h * w
        assert lib.g2v_cloud_consistency_workspace(n, h, w) == 4 * n * h * w
        assert lib.g2v_cloud_compact_normals_workspace(n, h, w) == 8 * n * blocks          # "8 N ceil(H W / 1024)"
        assert lib.g2v_cloud_compact_workspace(n, h, w) == 8 * n * blocks
    for m in (1, 2, 1000, 262656):
        assert lib.g2v_voxel_reduce_workspace(m) == 64 * m
    assert lib.g2v_voxel_reduce_workspace(0) == 0 and lib.g2v_cloud_render_workspace(0, 4, 4) == 0
    assert lib.g2v_cloud_consistency_workspace(257, 4, 4) == 0 and lib.g2v_cloud_nn_workspace(-1, 4) == 0


def test_queries_whose_layout_the_sources_state(lib):
    """No closed form in the header: the sums are the source files' own comments (CONTRACTS' size_doc), restated here so that a
    change of a layout has to be made in two places."""
    for n, h, w in SHAPES:
        p, blocks = n * h * w, -(-(h * w) // 1024)
        slots = 2
        while slots < 2 * p:
            slots *= 2
        assert lib.g2v_voxel_assign_workspace(n, h, w) == 12 * slots + 4 * p + 8 * -(-p // 1024) + p
        assert lib.g2v_cloud_mesh_workspace(n, h, w) == 16 * n * blocks + 6 * p
        assert lib.g2v_intrinsics_lsq_workspace(n, h, w) == 72 * n * min(64, blocks)
    for lk in (1, 64, 65, 449, 512):
        assert lib.g2v_decode_attn_workspace(lk, 12) == 12 * -(-lk // 64) * 130 * 4
    for hq, hkv, b in ((12, 2, 1), (12, 2, 3), (28, 4, 1), (4, 4, 2)):
        assert lib.g2v_decode_attn_pg_workspace(hq, hkv, b) == b * hq * min(128, 256 // hkv) * 130 * 4
        assert lib.g2v_decode_attn_shared_workspace(hq, hkv, b, 300, 65) == b * hq * 128 * 130 * 4
    for slots in (0, 1, 7):
        assert lib.g2v_flash_attn_workspace(slots) == slots * 256 * 130 * 4
    for rows, n, split in ((1, 151936, 19), (3, 24577, 4), (64, 20000, 3), (600, 40000, 1)):
        chunks = -(-n // 8192)
        assert min(chunks, 1 if rows >= 512 else -(-512 // rows)) == split
        assert lib.g2v_logprob_rows_workspace(rows, n) == (4 * (512 + rows * chunks * 3) if split > 1 else 0)
        for k in (1, 32):
            assert lib.g2v_topk_rows_workspace(rows, n, k) == (4 * (512 + rows * split * 2 * k) if split > 1 else 0)
