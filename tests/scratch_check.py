"""What the kernels borrow from the caller - workspaces, ticket words, staging buffers - held to what include/g2vlm_hip.h says
about it.  No tests here; tests/test_scratch_check_cpu.py checks this module, tests/test_scratch_contracts_gpu.py uses it.

Arena      one allocation [guard | payload | guard]: the payload has exactly the bytes the entry point asks for and starts at
           exactly the alignment it demands (address % align == 0, address % 2 align != 0), so a workspace formula that is a word
           short, or a last vector store that runs over, lands in a guard - memory the test owns - and check() names the offset.
PATTERNS   what the payload holds before the launch, from benign to hostile: zeros, ones (every int32 word 1: not zero, but
           still a valid index, count and flag wherever it is read by mistake), leftover (what a launch of another shape left),
           nan (0xFF bytes; fp32 workspaces only).
CONTRACTS  one row per entry point of the header with a workspace, scratch or tmp argument: the class of its promise
           (uninit_ok: any contents; zero_once: ticket words zero before the first launch, reset by every launch), the size
           query, the alignment and where the tickets live.
staged()   the patterns applied to one launch in that order; the first that fails ends the run, the more hostile ones are
           reported as not run.  A read-before-write that `ones` shows is fixed from the code, never probed with wilder values.
"""
import collections
import os
import re

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "g2vlm_hip.h")

GUARD_BYTES = 64 << 10
GUARD_BYTE = 0xA5
PATTERNS = ("zeros", "ones", "leftover", "nan")              # benign -> hostile
_SLACK = 64                                                  # room to move the payload to its exact alignment


class Arena:
    """[guard | payload | guard] in one uint8 allocation on `device`."""

    def __init__(self, nbytes, align=4, device="cpu", guard=GUARD_BYTES):
        assert align in (1, 2, 4, 8, 16) and nbytes >= 0 and guard >= GUARD_BYTES
        self.nbytes, self.align = int(nbytes), align
        self.buf = torch.full((guard + _SLACK + self.nbytes + guard,), GUARD_BYTE, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        off = guard + (-(base + guard)) % align
        if (base + off) % (2 * align) == 0:                  # no more alignment than the contract gives
            off += align
        self.off = off
        assert self.ptr % align == 0 and self.ptr % (2 * align) != 0 and off + self.nbytes + guard <= self.buf.numel()

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def payload(self, dtype=torch.uint8):
        """the view to pass: exactly nbytes, as `dtype` (its size must divide nbytes and the alignment)"""
        size = torch.empty((), dtype=dtype).element_size()
        assert self.nbytes % size == 0 and self.align % size == 0, (self.nbytes, self.align, dtype)
        return self.buf[self.off:self.off + self.nbytes].view(dtype)

    def head(self, nbytes, dtype=torch.uint8):
        """the first nbytes of the payload: a smaller launch's workspace inside this one"""
        assert 0 <= nbytes <= self.nbytes
        return self.buf[self.off:self.off + nbytes].view(dtype)

    def fill(self, pattern, zero=()):
        """the payload under `pattern`; then the byte ranges `zero` = [(offset, bytes), ...] (ticket words) set to 0.
        `leftover` leaves the payload as it is: the caller has run another shape on it."""
        p = self.payload()
        if pattern == "zeros":
            p.zero_()
        elif pattern == "ones":
            p.copy_(torch.tensor([1, 0, 0, 0], dtype=torch.uint8).repeat((self.nbytes + 3) // 4)[:self.nbytes])
        elif pattern == "nan":
            p.fill_(0xFF)
        else:
            assert pattern == "leftover", pattern
        for o, n in zero:
            assert 0 <= o and o + n <= self.nbytes, ("ticket region outside the payload", o, n, self.nbytes)
            p[o:o + n].zero_()
        return self

    def damage(self, keep_from=None, snapshot=None):
        """None, or a description of the first damaged guard byte (offset relative to the payload: < 0 in front of it,
        >= nbytes behind it).  With snapshot (a clone of buf) and keep_from, payload bytes [keep_from, nbytes) count as guard
        too: a launch that was given only the first keep_from bytes must have left them as the snapshot has them."""
        parts = [(0, self.off, None), (self.off + self.nbytes, self.buf.numel(), None)]
        if snapshot is not None:
            parts.insert(1, (self.off + keep_from, self.off + self.nbytes, snapshot))
        for lo, hi, ref in parts:
            got = self.buf[lo:hi]
            bad = (got != GUARD_BYTE) if ref is None else (got != ref[lo:hi])
            if bool(bad.any()):
                i = int(torch.nonzero(bad)[0])
                want = GUARD_BYTE if ref is None else int(ref[lo + i])
                return (f"byte at payload offset {lo + i - self.off} (payload of {self.nbytes} bytes, {self.align}-byte aligned) "
                        f"was {want:#04x}, is {int(got[i]):#04x}; {int(bad.sum())} bytes damaged in this part")
        return None

    def check(self, **kw):
        d = self.damage(**kw)
        assert d is None, "write outside the workspace: " + d

    def snapshot(self):
        return self.buf.clone()


def same_bits(a, b):
    """bit equality of two tensors (NaN payloads and signed zeros included)"""
    if a is None or b is None:
        return a is None and b is None
    if a.dtype != b.dtype or tuple(a.shape) != tuple(b.shape):
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def first_difference(got, want):
    """None, or which output differs first and where"""
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if not same_bits(g, w):
            if g is None or w is None or g.dtype != w.dtype or tuple(g.shape) != tuple(w.shape):
                return f"output {i}: {None if g is None else (g.dtype, tuple(g.shape))} against {None if w is None else (w.dtype, tuple(w.shape))}"
            gb, wb = g.contiguous().reshape(-1).view(torch.uint8), w.contiguous().reshape(-1).view(torch.uint8)
            bad = torch.nonzero(gb != wb)
            return f"output {i}: {bad.numel()} bytes differ, the first at byte {int(bad[0])}"
    return None


# ------------------------------------------------------------------------------------------------------------- the contracts
Contract = collections.namedtuple("Contract", "kind query align dtype tickets ticket_doc size_doc via_struct")
Contract.__new__.__defaults__ = (None,)


def _no_tickets(*a, **k):
    return []


def _argmax_tickets(rows=1):
    return [(129 * 4 * r, 4) for r in range(rows)]            # word 0 of every row's 129-word slab


def _row_tickets(nbytes):
    return [(0, min(nbytes, 512 * 4))] if nbytes else []      # one word per row, 512 rows at most, at the head


def _gemm_tickets(nbytes):
    return [(0, min(nbytes, 64 << 10))]


def _uninit(query, align, dtype, size_doc):
    return Contract("uninit_ok", query, align, dtype, _no_tickets, None, size_doc)


F32, I32, U8, I64 = torch.float32, torch.int32, torch.uint8, torch.int64

CONTRACTS = {
    # ---- zero once, tickets reset themselves
    "g2v_gemm_bf16": Contract("zero_once", None, 4, I32, _gemm_tickets, "the first 64 KiB (one int32 per column group)",
                              "desc.workspace_bytes, the caller's choice", "g2v_gemm_desc"),
    "g2v_argmax_bf16": Contract("zero_once", None, 4, I32, _argmax_tickets, "word 0 of int32[129]", "int32[129]"),
    "g2v_argmax_rows_bf16": Contract("zero_once", None, 4, I32, _argmax_tickets, "word 0 of int32[129] per row", "int32[rows * 129]"),
    "g2v_sample_rows_bf16": Contract("zero_once", None, 4, I32, _argmax_tickets, "word 0 of int32[129] per row", "int32[rows * 129]"),
    "g2v_logprob_rows_bf16": Contract("zero_once", "g2v_logprob_rows_workspace", 4, I32, _row_tickets, "the first 512 int32",
                                      "g2v_logprob_rows_workspace(rows, n)"),
    "g2v_topk_rows_bf16": Contract("zero_once", "g2v_topk_rows_workspace", 4, I32, _row_tickets, "the first 512 int32",
                                   "g2v_topk_rows_workspace(rows, n, k)"),
    # ---- any contents
    "g2v_flash_attn": _uninit("g2v_flash_attn_workspace", 16, F32, "g2v_flash_attn_workspace(n_slots)"),
    "g2v_lanczos_resize_u8": _uninit(None, 1, U8, "u8 [N, Hin, Wout, 3]"),
    "g2v_decode_attn": _uninit("g2v_decode_attn_workspace", 4, F32, "g2v_decode_attn_workspace(Lk, Hq)"),
    "g2v_decode_attn_dyn": _uninit("g2v_decode_attn_workspace", 4, F32, "g2v_decode_attn_workspace(max_len, Hq)"),
    "g2v_decode_attn_batch": _uninit("g2v_decode_attn_workspace", 4, F32, "batch * g2v_decode_attn_workspace(max_len, Hq)"),
    "g2v_decode_attn_fused": _uninit("g2v_decode_attn_workspace", 4, F32, "batch * g2v_decode_attn_workspace(max_len, Hq)"),
    "g2v_decode_attn_pg": _uninit("g2v_decode_attn_pg_workspace", 4, F32, "g2v_decode_attn_pg_workspace(Hq, Hkv, batch)"),
    "g2v_decode_attn_pg_kv8": _uninit("g2v_decode_attn_pg_workspace", 4, F32, "g2v_decode_attn_pg_workspace(Hq, Hkv, batch)"),
    "g2v_decode_attn_shared": _uninit("g2v_decode_attn_shared_workspace", 4, F32,
                                      "g2v_decode_attn_shared_workspace(Hq, Hkv, batch, prefix_len, suffix_max_len)"),
    "g2v_cloud_compact": _uninit("g2v_cloud_compact_workspace", 4, U8, "8 N ceil(H W / 1024)"),
    "g2v_intrinsics_lsq": _uninit("g2v_intrinsics_lsq_workspace", 8, U8, "72 N min(64, ceil(H W / 1024))"),
    "g2v_cloud_consistency": _uninit("g2v_cloud_consistency_workspace", 4, U8, "4 N H W"),
    "g2v_cloud_render": _uninit("g2v_cloud_render_workspace", 8, U8, "8 M OH OW"),
    "g2v_voxel_assign": _uninit("g2v_voxel_assign_workspace", 8, U8, "12 slots + 4 P + 8 ceil(P / 1024) + P, slots = the power of two >= 2 P"),
    "g2v_voxel_reduce": _uninit("g2v_voxel_reduce_workspace", 8, U8, "64 M"),
    "g2v_cloud_mesh": _uninit("g2v_cloud_mesh_workspace", 4, U8, "16 N ceil(H W / 1024) + 6 N H W"),
    "g2v_cloud_nn": _uninit("g2v_cloud_nn_workspace", 16, U8, "256 + 24 Nt + 8 Nq + 4 (G^3 + 1) + 4 ceil(G^3 / 1024)"),
    "g2v_cloud_compact_normals": _uninit("g2v_cloud_compact_normals_workspace", 4, U8, "8 N ceil(H W / 1024)"),
}


def patterns_for(name, fp32=False):
    """the patterns the contract admits, in staging order: nan only for the fp32 workspaces of the attention kernels"""
    c = CONTRACTS[name]
    return tuple(p for p in PATTERNS if p != "nan" or (fp32 and c.dtype == F32 and c.kind == "uninit_ok"))


# ------------------------------------------------------------------------------------------------------------- the header
_PROTO = re.compile(r"^(?:int64_t|int|const char\*|void)\s+(g2v_\w+)\s*\(([^;{]*?)\)\s*;", re.S | re.M)


def header_entry_points(path=HEADER):
    """{name: [parameter names]} of every prototype of the header, comments stripped"""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    out = {}
    for m in _PROTO.finditer(text):
        params = [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
        out[m.group(1)] = [re.split(r"[\s*]+", re.sub(r"\[.*\]", "", p))[-1] for p in params if p and p != "void"]
    return out


def header_scratch_entry_points(path=HEADER):
    """the entry points that take scratch: a parameter named workspace, scratch or tmp, or a descriptor struct with a
    `workspace` member (-> {name: None or the struct's name})"""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    structs = {m.group(2) for m in re.finditer(r"typedef struct\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S)
               if re.search(r"void\*\s+workspace\s*;", m.group(1))}
    out = {}
    for m in _PROTO.finditer(text):
        names = header_entry_points(path)[m.group(1)]
        if {"workspace", "scratch", "tmp"} & set(names):
            out[m.group(1)] = None
        else:
            for s in structs:
                # a launching entry point of the descriptor, not a host-only query with an output array behind it
                if re.search(r"const\s+" + s + r"\s*\*", m.group(2)) and "stream" in names:
                    out[m.group(1)] = s
    return out


# ------------------------------------------------------------------------------------------------------------- the staged runner
Stage = collections.namedtuple("Stage", "pattern status detail")


def staged(name, nbytes, run, want, patterns, zero=(), leftover=None, device="cuda", sync=None):
    """One launch under every pattern of `patterns` (a subset of PATTERNS, applied in PATTERNS' order).
    run(arena) -> tuple of output tensors; want = the ordinary run's; zero = the ticket byte ranges of a zero_once row;
    leftover(arena): runs a launch of another shape on arena.head(...) (the arena then holds `ones` overwritten by it).
    Returns the list of Stage; the first pattern with a mismatch or a damaged guard fails, the rest are not run."""
    c = CONTRACTS[name]
    assert c.kind == "uninit_ok" or zero or nbytes == 0, f"{name}: a zero_once row names its ticket words"
    order = [p for p in PATTERNS if p in patterns]
    stages = []
    for i, pat in enumerate(order):
        arena = Arena(nbytes, c.align, device)
        if pat == "leftover":
            if leftover is None:
                stages.append(Stage(pat, "not applicable", "no other shape fits this workspace"))
                continue
            arena.fill("ones", zero)
            leftover(arena)
            arena.fill("leftover", ())                       # tickets are NOT zeroed again: the launch before reset them
        else:
            arena.fill(pat, zero)
        got = run(arena)
        if sync is not None:
            sync()
        problem = first_difference(got, want)
        dmg = arena.damage()
        if dmg is not None:
            problem = (problem + "; " if problem else "") + "write outside the workspace: " + dmg
        if problem:
            stages.append(Stage(pat, "FAILED", problem))
            stages += [Stage(p, "not run", f"{pat} failed first") for p in order[i + 1:]]
            break
        stages.append(Stage(pat, "ok", ""))
    return stages


def assert_staged(name, stages, what=""):
    bad = [s for s in stages if s.status == "FAILED"]
    assert not bad, f"{name} {what}: " + "; ".join(f"[{s.pattern}: {s.status}{' - ' + s.detail if s.detail else ''}]" for s in stages)
