"""ctypes binding of libg2vlm_hip.so (include/g2vlm_hip.h) + thin torch-tensor front ends.

PyTorch is plumbing here: device memory (tensors), streams, and nothing else.  Every compute
call below lands in a hand-written gfx950 kernel.  There is NO fallback: if the library is
missing or a call fails, this module raises.
"""
import ctypes as C
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("G2V_LIB_PATH") or os.path.join(_HERE, "lib", "libg2vlm_hip.so")   # override: experiment builds only

EPI_BF16, EPI_GELU, EPI_QUICKGELU, EPI_SWIGLU, EPI_RES_F32, EPI_RES_BF16 = range(6)
GAMMA_ROUND_BF16 = 1
FORCE_SMALL_TILE = 2
SUPERTILE = 4
FORCE_BIG_TILE = 8
FORCE_8P = 16
P8_H192, P8_H128, P8_H256, P8_TWO_BARRIER, P8_H288, P8_H224, P8_H160 = 128, 256, 512, 1024, 4096, 8192, 16384   # A/B only
P8_PIPELINED = 32768                                        # A/B only: round 1's main loop instead of the staggered two-barrier one
P8_FOUR_WAVES = 65536       # force gemm_4w.hip (four waves, one per SIMD, 128-column wave tiles); without a flag the launcher picks by shape class
P8_EIGHT_WAVES = 131072     # force gemm_8p.hip's staggered eight-wave loop (round 2's default)
P8_NO_ROW_SKIP = 262144     # A/B only: wave rows without a valid row run their MFMAs anyway
F32, BF16 = 0, 1
NO_CAUSAL = 2 ** 30
_DEBUG_GEMM_FLAGS = int(os.environ.get("G2V_GEMM_FLAGS", "0"))     # A/B experiments only (tools/, tests -k ...)


class GemmGroup(C.Structure):
    _fields_ = [("A", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("C", C.c_void_p),
                ("res", C.c_void_p), ("gamma", C.c_void_p), ("M", C.c_int32), ("_pad", C.c_int32)]


class GemmDesc(C.Structure):
    _fields_ = [("g", GemmGroup * 2), ("ngroups", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("lda", C.c_int32), ("ldc", C.c_int32), ("ldres", C.c_int32), ("epilogue", C.c_int32),
                ("flags", C.c_int32), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


_P, _I, _F, _L, _D = C.c_void_p, C.c_int, C.c_float, C.c_int64, C.c_double
_SIGS = {
    "g2v_version": ([], C.c_int),
    "g2v_arch": ([], C.c_char_p),
    "g2v_gemm_bf16": ([C.POINTER(GemmDesc), _P], C.c_int),
    "g2v_gemm_route": ([C.POINTER(GemmDesc), C.POINTER(C.c_int32 * 4)], C.c_int),
    "g2v_gemm_f32": ([_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P], C.c_int),
    "g2v_layernorm": ([_P, _I, _I, _P, _P, _F, _P, _I, _I, _I, _I, _P], C.c_int),
    "g2v_rmsnorm": ([_P, _I, _P, _P, _I, _F, _P, _I, _I, _I, _I, _P], C.c_int),
    "g2v_mrope_table": ([_P, _I, _P, _P, _P, _P], C.c_int),
    "g2v_qknorm_mrope_cache": ([_P, _I, _I, _I, _P, _P, _P, _P, _I, _F, _I, _P, _P, _P, _P, _P, _P, _P], C.c_int),
    "g2v_flash_attn": ([_P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _F, _P, _P, _I, _P, _I, _I, _P, _P], C.c_int),
    "g2v_flash_attn_workspace": ([_I], C.c_int64),
    "g2v_debug_attn_form": ([_I], C.c_int),
    "g2v_rope2d": ([_P, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P], C.c_int),
    "g2v_rope_vision": ([_P, _I, _I, _I, _I, _P, _P, _P], C.c_int),
    "g2v_im2col14": ([_P, _I, _I, _I, _P, _I, _P], C.c_int),
    "g2v_dino_preprocess": ([_P, _I, _I, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _P, _P], C.c_int),
    "g2v_dino_assemble": ([_P, _P, _P, _P, _P, _I, _I, _I, _P], C.c_int),
    "g2v_im2col_patch": ([_P, _I, _I, _I, _I, _P, _I, _P], C.c_int),
    "g2v_qwen_patchify_u8": ([_P, _I, _I, _I, C.POINTER(C.c_float), C.POINTER(C.c_float), _P, _I, _P], C.c_int),
    "g2v_vit_assemble": ([_P, _P, _P, _P, _I, _I, _I, _I, _P], C.c_int),
    "g2v_gather_rows_f32": ([_P, _I, _P, _P, _I, _I, _I, _P], C.c_int),
    "g2v_scatter_rows_f32": ([_P, _I, _P, _P, _I, _I, _I, _P], C.c_int),
    "g2v_cast_f32_bf16": ([_P, _P, _L, _P], C.c_int),
    "g2v_cast_bf16_f32": ([_P, _P, _L, _P], C.c_int),
    "g2v_pts_epilogue": ([_P, _I, _I, _I, _I, _P, _P, _P, _P], C.c_int),
    "g2v_pixel_shuffle14": ([_P, _I, _I, _I, _I, _P, _P], C.c_int),
    "g2v_lanczos_resize_u8": ([_P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _I, _P, _P, _I, _P], C.c_int),
    "g2v_pts_epilogue_ps": ([_P, _I, _I, _I, _I, _I, _P, _P, _P, _P], C.c_int),
    "g2v_pixel_shuffle": ([_P, _I, _I, _I, _I, _I, _P, _P], C.c_int),
    "g2v_camera_tail": ([_P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P], C.c_int),
    "g2v_argmax_bf16": ([_P, _I, _P, _P, _P], C.c_int),
    "g2v_gemv_bf16": ([_P, _P, _P, _P, _P, _I, _I, _P], C.c_int),
    "g2v_decode_attn_workspace": ([_I, _I], C.c_int64),
    "g2v_gemv_rmsnorm_bf16": ([_P, _P, _F, _P, _P, _P, _I, _I, _P], C.c_int),
    "g2v_gemv_swiglu_bf16": ([_P, _P, _P, _I, _I, _P], C.c_int),
    "g2v_gemv_rmsnorm_swiglu_bf16": ([_P, _P, _F, _P, _P, _I, _I, _P], C.c_int),
    "g2v_decode_attn": ([_P, _P, _P, _P, _I, _I, _I, _F, _P, _P], C.c_int),
    "g2v_swiglu_bf16": ([_P, _P, _I, _P], C.c_int),
    "g2v_decode_attn_dyn": ([_P, _P, _P, _P, _P, _I, _I, _I, _F, _P, _P], C.c_int),
    "g2v_decode_advance": ([_P, _P, _P, _P], C.c_int),
    "g2v_decode_attn_batch": ([_P, _P, _P, _P, _P, _I, _L, _I, _I, _I, _F, _P, _P], C.c_int),
    "g2v_decode_advance_batch": ([_P, _P, _P, _I, _P], C.c_int),
    "g2v_decode_attn_fused": ([_P, _P, _P, _F, _I, _P, _P, _P, _P, _P, _P, _I, _L, _I, _I, _I, _F, _P, _P], C.c_int),
    "g2v_argmax_rows_bf16": ([_P, _I, _I, _L, _P, _P, _P], C.c_int),
    "g2v_gemv_pg": ([_P, _P, _F, _P, _P, _P, _P, _I, _I, _I, _P], C.c_int),
    "g2v_gemv_pg_batch": ([_P, _P, _F, _P, _P, _P, _P, _I, _I, _I, _I, _P], C.c_int),
    "g2v_decode_attn_pg_workspace": ([_I, _I, _I], C.c_int64),
    "g2v_decode_attn_pg": ([_P, _P, _P, _F, _I, _P, _P, _P, _P, _P, _P, _I, _L, _I, _I, _I, _F, _P, _P], C.c_int),
    "g2v_sample_rows_bf16": ([_P, _I, _I, _L, _P, _P, _P, _P], C.c_int),
    "g2v_decode_attn_shared_workspace": ([_I, _I, _I, _I, _I], C.c_int64),
    "g2v_decode_attn_shared": ([_P, _P, _P, _F, _I, _P, _P, _P, _P, _I, _P, _P, _P, _I, _L, _I, _I, _I, _F, _P, _P, _P], C.c_int),
    "g2v_gemv_pg_fp8": ([_P, _P, _F, _P, _P, _P, _P, _P, _I, _I, _I, _P], C.c_int),
    "g2v_gemv_pg_batch_fp8": ([_P, _P, _F, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P], C.c_int),
    "g2v_gemv_pg_route": ([_I, _I, _I, _I, _I, _I, C.POINTER(C.c_int32 * 4)], C.c_int),
    "g2v_kv_quant_e4m3": ([_P, _L, _I, _P, _P, _P], C.c_int),
    "g2v_kv_dequant_e4m3": ([_P, _P, _L, _I, _P, _P], C.c_int),
    "g2v_decode_attn_pg_kv8": ([_P, _P, _P, _F, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _L, _I, _I, _I, _F, _P, _P], C.c_int),
    "g2v_logprob_rows_workspace": ([_I, _I], C.c_int64),
    "g2v_logprob_rows_bf16": ([_P, _I, _I, _L, _P, _P, _P, _P, _P, _L, _P], C.c_int),
    "g2v_topk_rows_workspace": ([_I, _I, _I], C.c_int64),
    "g2v_topk_rows_bf16": ([_P, _I, _I, _L, _I, _P, _P, _P, _L, _P], C.c_int),
    "g2v_cloud_mask": ([_P, _P, _P, _I, _I, _I, _I, _F, _F, _F, _P, _P], C.c_int),
    "g2v_cloud_compact_workspace": ([_I, _I, _I], C.c_int64),
    "g2v_cloud_compact": ([_P, _P, _P, _I, _I, _I, _P, _L, _P, _P, _L, _P], C.c_int),
    "g2v_intrinsics_lsq_workspace": ([_I, _I, _I], C.c_int64),
    "g2v_intrinsics_lsq": ([_P, _P, _I, _I, _I, _P, _P, _P, _L, _P], C.c_int),
    "g2v_cloud_consistency_workspace": ([_I, _I, _I], C.c_int64),
    "g2v_cloud_consistency": ([_P, _P, _P, _P, _P, _I, _I, _I, _F, _I, _I, _P, _P, _P, _P, _P, _L, _P], C.c_int),
    "g2v_cloud_render_workspace": ([_I, _I, _I], C.c_int64),
    "g2v_cloud_render": ([_P, _P, _P, _I, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _L, _P], C.c_int),
    "g2v_cloud_mesh_workspace": ([_I, _I, _I], C.c_int64),
    "g2v_cloud_mesh": ([_P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _P, _L, _P, _P, _L, _P], C.c_int),
    "g2v_cloud_nn_workspace": ([_L, _L], C.c_int64),
    "g2v_cloud_nn": ([_P, _P, _L, _P, _P, _L, _F, _I, _P, _P, _P, _P, _L, _P], C.c_int),
    "g2v_cloud_normals": ([_P, _P, _P, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P], C.c_int),
    "g2v_cloud_compact_normals_workspace": ([_I, _I, _I], C.c_int64),
    "g2v_cloud_compact_normals": ([_P, _P, _P, _P, _I, _I, _I, _P, _L, _P, _P, _L, _P], C.c_int),
    "g2v_voxel_bounds": ([_P, _P, _I, _I, _I, _P, _P], C.c_int),
    "g2v_voxel_assign_workspace": ([_I, _I, _I], C.c_int64),
    "g2v_voxel_assign": ([_P, _P, _I, _I, _I, _D, _D, _D, _D, _P, _P, _P, _L, _P], C.c_int),
    "g2v_voxel_reduce_workspace": ([_L], C.c_int64),
    "g2v_voxel_reduce": ([_P, _P, _P, _I, _I, _I, _D, _D, _D, _D, _L, _P, _P, _P, _P, _P, _L, _I, _P], C.c_int),
}
EXPORTS = tuple(_SIGS)

_lib = None


def lib():
    """Load the shared library (once).  Raises if it has not been built — no CPU fallback exists."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -m g2vlm_amd.build` (hipcc, gfx950). "
                               "g2vlm_amd has no CPU fallback.")
        _lib = C.CDLL(LIB_PATH)
        for name, (args, res) in _SIGS.items():
            fn = getattr(_lib, name)
            fn.argtypes, fn.restype = args, res
        # the kernels are written for one architecture (wave64 MFMA shapes, LDS-DMA, and cross-workgroup hand-offs that lean on
        # its sc1 write-through / L2-bypass behaviour, csrc/gemm_skinny.hip): refuse any other device instead of misbehaving
        if torch.cuda.is_available():
            want = _lib.g2v_arch().decode()
            have = getattr(torch.cuda.get_device_properties(torch.cuda.current_device()), "gcnArchName", "")
            if have and not have.split(":")[0] == want:
                _lib = None
                raise RuntimeError(f"libg2vlm_hip.so is built for {want}; this device is {have}")
        if os.environ.get("G2V_ATTN_FORM"):                   # A/B experiments only (tools/bench_ab_env.sh): 0 = the 8 x 32 attention form
            _lib.g2v_debug_attn_form(int(os.environ["G2V_ATTN_FORM"]))
    return _lib


class HipError(RuntimeError):
    pass


def _ck(rc, what):
    if rc != 0:
        raise HipError(f"{what} failed with code {rc}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream on the current device (the raw getter is ~20x cheaper than building a
    torch.cuda.Stream object per launch: 8 us x ~800 launches per scene otherwise)."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    assert t.is_cuda, "libg2vlm_hip takes device pointers only"
    return C.c_void_p(t.data_ptr())


def _rowmajor(t):
    assert t.dim() == 2 and t.stride(1) == 1, "row-major 2-D view expected"
    return t.stride(0)


# ------------------------------------------------------------------------------------------ GEMM
def h2d(t, device, dtype=None, resident=False):
    """Host -> device copy that never blocks the host: the tensor is staged through pinned memory (torch's caching host
    allocator keeps the staging buffers alive until the copy has run) and copied with non_blocking=True.  A pageable
    `.to(device)` is a stream-wide sync point whose wake-up costs milliseconds while the GPU is busy: 174 of them cost a
    C5 step 0.45 s of GPU idle time."""
    if t.is_cuda:
        return t.to(dtype) if dtype is not None else t
    if dtype is not None:
        t = t.to(dtype)
    if torch.device(device).type != "cuda":
        return t.to(device)
    out = t.contiguous().pin_memory().to(device, non_blocking=True)
    if resident:
        # a table that is cached and may later be read by kernels on OTHER streams (attention plans, memoised indices): make
        # sure the upload has landed before anyone can see the cache entry.  Paid once per table, never in steady state.
        torch.cuda.current_stream(out.device).synchronize()
    return out


def scratch_owner(device_index):
    """Owner of a piece of multi-launch kernel scratch: (device, raw stream, host thread).

    Scratch that lives across launches (the attention's partial slots between its forward and combine launches, the skinny
    GEMM's K-split tickets, the argmax ticket) is only safe to share between launches that the stream orders ONE CALL AFTER
    THE OTHER.  Two streams break that, and so do two host threads enqueueing on one stream: ctypes releases the GIL inside a
    call, so thread B's forward can land between thread A's forward and A's combine (round 2's red GPU run: 8 rank threads
    of the sharding simulation shared one plan's slots).  Keyed by all three, every (stream, thread) pair owns its scratch."""
    return (device_index, int(torch._C._cuda_getCurrentRawStream(device_index)), threading.get_ident())


_gemm_ws = {}


GEMM_WS_WORDS = 2 << 20                                     # 8 MiB of int32: covers every skinny shape of the path


def _gemm_workspace(device):
    """Scratch of the skinny GEMM's cross-workgroup K split, one per scratch_owner (device, stream, host thread) so that
    launches that can overlap or interleave never share tickets: zeroed once, tickets self-reset."""
    key = scratch_owner(device.index)
    ws = _gemm_ws.get(key)
    if ws is None:
        ws = _gemm_ws[key] = torch.zeros(GEMM_WS_WORDS, dtype=torch.int32, device=device)
    return ws


def gemm_bf16(groups, N, K, epilogue, out_ld, lda=None, ldres=0, flags=0, ws=None):
    """groups: list (<=2) of dicts {A, W, bias, C, res, gamma, M}; tensors are bf16 except res/gamma/C per epilogue."""
    _ck(lib().g2v_gemm_bf16(C.byref(_gemm_desc(groups, N, K, epilogue, out_ld, lda, ldres, flags, ws)), _stream()), "g2v_gemm_bf16")


GEMM_FORMS = {1: "128x128", 2: "big", 3: "8p", 4: "4w", 5: "skinny"}


def gemm_route(groups, N, K, epilogue, out_ld, lda=None, ldres=0, flags=0, ws=None):
    """What gemm_bf16 with the same arguments launches, without launching: (form name, tile height, S, KS), S / KS = the
    skinny kernel's K split inside / across workgroups (1 for the tiled forms)."""
    out = (C.c_int32 * 4)()
    _ck(lib().g2v_gemm_route(C.byref(_gemm_desc(groups, N, K, epilogue, out_ld, lda, ldres, flags, ws)), C.byref(out)),
        "g2v_gemm_route")
    return GEMM_FORMS[out[0]], out[1], out[2], out[3]


def _gemm_desc(groups, N, K, epilogue, out_ld, lda, ldres, flags, ws):
    d = GemmDesc()
    flags |= _DEBUG_GEMM_FLAGS
    d.ngroups, d.N, d.K, d.epilogue, d.flags = len(groups), N, K, epilogue, flags
    d.lda = lda if lda is not None else K
    d.ldc, d.ldres = out_ld, ldres
    if max(int(g["M"]) for g in groups) <= 64:
        # skinny path: scratch for its cross-workgroup K split.  `ws` (int32, zeroed once) when the caller owns one - a
        # captured decode step must not allocate - else the per-(device, stream) default
        if ws is None:
            ws = _gemm_workspace(groups[0]["A"].device)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
    for i, g in enumerate(groups):
        gg = d.g[i]
        gg.A, gg.W, gg.bias, gg.C = _p(g["A"]), _p(g["W"]), _p(g.get("bias")), _p(g["C"])
        gg.res, gg.gamma, gg.M = _p(g.get("res")), _p(g.get("gamma")), int(g["M"])
    return d


def linear(x, w, bias=None, epilogue=EPI_BF16, out=None, res=None, gamma=None, flags=0, ws=None):
    """Single-problem convenience wrapper.  x bf16 [M,K] (row-major view), w bf16 [N,K]."""
    M, K = x.shape
    N = w.shape[0]
    n_out = N // 2 if epilogue == EPI_SWIGLU else N
    if out is None:
        dt = torch.float32 if epilogue == EPI_RES_F32 else torch.bfloat16
        out = torch.empty((M, n_out), dtype=dt, device=x.device)
    gemm_bf16([dict(A=x, W=w, bias=bias, C=out, res=res, gamma=gamma, M=M)], N, K, epilogue,
              out_ld=_rowmajor(out), lda=_rowmajor(x), ldres=_rowmajor(res) if res is not None else 0, flags=flags, ws=ws)
    return out


def gemm_f32(x, w, bias=None, relu=False, res=None, out=None):
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    _ck(lib().g2v_gemm_f32(_p(x), _p(w), _p(bias), _p(out), _p(res), M, N, K, _rowmajor(x), _rowmajor(out),
                           _rowmajor(res) if res is not None else 0, int(relu), _stream()), "g2v_gemm_f32")
    return out


# ----------------------------------------------------------------------------------------- norms
def _dt(t):
    return BF16 if t.dtype == torch.bfloat16 else F32


def layernorm(x, w, b, eps, out_dtype=torch.bfloat16, out=None):
    M, Cc = x.shape
    if out is None:
        out = torch.empty((M, Cc), dtype=out_dtype, device=x.device)
    _ck(lib().g2v_layernorm(_p(x), _dt(x), _rowmajor(x), _p(w), _p(b), eps, _p(out), _dt(out), _rowmajor(out), M, Cc,
                            _stream()), "g2v_layernorm")
    return out


def rmsnorm(x, w_lo, w_hi, split, eps, out_dtype=torch.bfloat16, out=None):
    M, Cc = x.shape
    if out is None:
        out = torch.empty((M, Cc), dtype=out_dtype, device=x.device)
    _ck(lib().g2v_rmsnorm(_p(x), _rowmajor(x), _p(w_lo), _p(w_hi), int(split), eps, _p(out), _dt(out), _rowmajor(out),
                          M, Cc, _stream()), "g2v_rmsnorm")
    return out


def mrope_table(pos_i32, inv_freq):
    L = pos_i32.shape[1]
    cos = torch.empty((L, 128), dtype=torch.float32, device=pos_i32.device)
    sin = torch.empty_like(cos)
    _ck(lib().g2v_mrope_table(_p(pos_i32), L, _p(inv_freq), _p(cos), _p(sin), _stream()), "g2v_mrope_table")
    return cos, sin


def qknorm_mrope_cache(qkv, Hq, Hkv, qw_lo, qw_hi, kw_lo, kw_hi, split, eps, und_rounding, cos, sin, q_out, k_cache,
                       v_cache, kv_rows):
    L = qkv.shape[0]
    _ck(lib().g2v_qknorm_mrope_cache(_p(qkv), L, Hq, Hkv, _p(qw_lo), _p(qw_hi), _p(kw_lo), _p(kw_hi), int(split), eps,
                                     int(und_rounding), _p(cos), _p(sin), _p(q_out), _p(k_cache), _p(v_cache),
                                     _p(kv_rows), _stream()), "g2v_qknorm_mrope_cache")


# ------------------------------------------------------------------------------------- attention
class AttnSeg(C.Structure):
    _fields_ = [("desc", C.c_int32), ("head", C.c_int32), ("kt0", C.c_int32), ("kt1", C.c_int32), ("slot", C.c_int32),
                ("_pad", C.c_int32 * 3)]


class AttnPlan:
    """Device-side schedule of one attention shape (see attn.hip): tile descriptors, per-phase segment tables, the merge
    table and the partial-result workspace."""

    def __init__(self, tiles, n_tiles, phases, comb, n_comb, n_slots, tile_rows, device):
        self.tiles, self.n_tiles, self.phases = tiles, n_tiles, phases          # phases: list of (segs, seg_ptr, n_blocks)
        self.comb, self.n_comb, self.n_slots, self.tile_rows = comb, n_comb, n_slots, tile_rows
        self.n_blocks = max((p[2] for p in phases), default=0)
        self.n_split = n_comb                                                    # (name kept for the tests' introspection)
        self.ws_words = max(4, int(lib().g2v_flash_attn_workspace(n_slots)) // 4)
        self.device = device
        self._by_owner = {}

    def ws(self, owner):
        """Partial-result scratch of the launches `owner` (hip.scratch_owner: device, stream, host thread) issues: the slots
        are written by the forward launch(es) and read by the combine, so launches of one plan that overlap on two streams
        (scenes issued on two streams) or interleave from two host threads on one stream must not share them."""
        w = self._by_owner.get(owner)
        if w is None:
            w = self._by_owner[owner] = torch.empty(self.ws_words, dtype=torch.float32, device=self.device)
        return w


def _schedule_items(items, n_blocks, align_short_items, n_desc_tiles):
    """items: list of (desc, head, nkt) in launch order.  Returns per-block lists of (item index, kt0, kt1).

    Whole items first: with equal items and few left over (n_items = q n_blocks + r, r <= n_blocks / 8) every workgroup takes
    q whole items and the r left-over items are cut into s pieces each, one piece per workgroup of an evenly spread
    subset, s just large enough that a piece is <= 2 % of a workgroup's work: few partial slots, balance within 2 %.
    Otherwise the (item, KV tile) units are cut into n_blocks equal ranges (stream-K; for short items the cuts are
    snapped to item boundaries when that costs less balance than the partials cost traffic)."""
    import bisect
    n_items = len(items)
    per_block = [[] for _ in range(n_blocks)]
    sizes = [it[2] for it in items]
    U = sum(sizes)
    if n_items == 0 or U == 0:
        return per_block
    equal = min(sizes) == max(sizes)
    q, r = divmod(n_items, n_blocks)
    if equal and q >= 1 and 8 * r <= n_blocks:
        K0 = sizes[0]
        for bq in range(n_blocks):
            for i in range(bq * q, (bq + 1) * q):
                per_block[bq].append((i, 0, K0))
        if r:
            s_ = 1
            while s_ * q < 50 and 2 * s_ * r <= n_blocks and 2 * s_ <= K0:
                s_ *= 2
            for li in range(r):
                i = q * n_blocks + li
                for pc in range(s_):
                    kt0, kt1 = pc * K0 // s_, (pc + 1) * K0 // s_
                    if kt1 > kt0:
                        per_block[((li * s_ + pc) * n_blocks) // (r * s_)].append((i, kt0, kt1))
        return per_block
    prefix = [0]
    for n in sizes:
        prefix.append(prefix[-1] + n)
    bounds = [bq * U // n_blocks for bq in range(n_blocks + 1)]
    if align_short_items and U // max(1, n_items) < 48 and n_items >= 2 * n_blocks:
        for bq in range(1, n_blocks):
            jx = bisect.bisect_left(prefix, bounds[bq])
            lo_, hi_ = prefix[max(0, jx - 1)], prefix[min(jx, len(prefix) - 1)]
            bounds[bq] = lo_ if bounds[bq] - lo_ <= hi_ - bounds[bq] else hi_
        for bq in range(1, n_blocks + 1):
            bounds[bq] = max(bounds[bq], bounds[bq - 1])
    for bq in range(n_blocks):
        u, u_end = bounds[bq], bounds[bq + 1]
        while u < u_end:
            i = bisect.bisect_right(prefix, u) - 1
            kt0 = u - prefix[i]
            kt1 = min(sizes[i], kt0 + (u_end - u))
            per_block[bq].append((i, kt0, kt1))
            u += kt1 - kt0
    return per_block


def make_attn_plan(windows, Hq, device, max_blocks=None, tile_rows=128, align_short_items=True):
    """windows: list of (q_start, q_len, k_start, k_len, causal[, phase]).  One descriptor per tile_rows-row query tile of
    every window.  Windows with the same query rows and disjoint KV ranges (the view-sharded prefill: local K/V block in
    phase 0, the other ranks' blocks in phase 1) are merged by the combine pass that follows the LAST phase; every phase is
    its own launch (flash_attn(..., phase=i)), so a collective can run between them.
    A causal window needs k_len >= q_len: the mask is bottom-right aligned, so with fewer keys than queries the first
    q_len - k_len rows see no key at all (their output would be left unwritten, or 0 x 1/0 inside a mixed tile)."""
    rows, desc_nkt, desc_phase, out_tiles = [], [], [], {}
    for win in windows:
        qs, ql, ks, kl, causal = win[:5]
        ph = win[5] if len(win) > 5 else 0
        if causal and kl < ql:
            raise ValueError(f"causal attention window {tuple(win)}: k_len {kl} < q_len {ql} leaves {ql - kl} query rows without a key")
        shift = (kl - ql) if causal else NO_CAUSAL
        for t0 in range(0, ql, tile_rows):
            qr = min(tile_rows, ql - t0)
            k_need = min(kl, t0 + qr - 1 + shift + 1)
            if k_need <= 0:
                continue
            out_tiles.setdefault((qs + t0, qr), []).append(len(rows))
            rows.append([qs + t0, qr, ks, kl, shift, qs, 0, 0])
            desc_nkt.append((k_need + 63) // 64)
            desc_phase.append(ph)
    n_tiles = len(rows)
    n_phases = max(desc_phase, default=0) + 1
    if max_blocks is None:
        max_blocks = 512 if tile_rows == 128 else 256          # resident workgroups: 2 (4-wave) or 1 (8-wave) per CU
    # ---- schedule every phase
    pieces = {}                                                # (desc, head) -> list of [phase, block, position, kt0, kt1]
    phase_blocks = []
    for ph in range(n_phases):
        descs = [d for d in range(n_tiles) if desc_phase[d] == ph]
        items = [(d, h, desc_nkt[d]) for h in range(Hq) for d in descs]
        U = sum(it[2] for it in items)
        # more workgroups than items is fine (a 731-row ViT prefill has 36 items but 8 000 KV tiles: 36 CUs would do all the
        # work); keep at least ~8 KV tiles per workgroup so the per-segment prologue / partial write stays amortised
        n_blocks = max(1, min(max_blocks, max(len(items), U // 8))) if items else 0
        per_block = _schedule_items(items, n_blocks, align_short_items, len(descs)) if items else []
        for bq, lst in enumerate(per_block):
            for pos, (i, kt0, kt1) in enumerate(lst):
                pieces.setdefault((items[i][0], items[i][1]), []).append([ph, bq, pos, kt0, kt1])
        phase_blocks.append((n_blocks, per_block, items))
    # ---- slots: an output tile (query rows, head) whose work is ONE segment over ONE descriptor is written directly
    comb, slot_of, n_slots = [], {}, 0
    for (q0, qr), descs in out_tiles.items():
        for h in range(Hq):
            pcs = [(d, pc) for d in descs for pc in pieces.get((d, h), [])]
            if len(pcs) == 1 and pcs[0][1][3] == 0 and pcs[0][1][4] == desc_nkt[pcs[0][0]]:
                slot_of[(pcs[0][0], h, 0)] = -1
                continue
            comb += [descs[0], h, n_slots, len(pcs)]
            for d, pc in pcs:
                slot_of[(d, h, pc[3])] = n_slots
                n_slots += 1
    phases = []
    for ph, (n_blocks, per_block, items) in enumerate(phase_blocks):
        segs = (AttnSeg * max(1, sum(len(x) for x in per_block)))()
        ptr, k = [0], 0
        for lst in per_block:
            for (i, kt0, kt1) in lst:
                d, h = items[i][0], items[i][1]
                sg = segs[k]
                sg.desc, sg.head, sg.kt0, sg.kt1, sg.slot = d, h, kt0, kt1, slot_of[(d, h, kt0)]
                k += 1
            ptr.append(k)
        seg_t = torch.frombuffer(bytearray(bytes(segs)), dtype=torch.int32).clone()
        phases.append((h2d(seg_t, device, resident=True), h2d(torch.tensor(ptr, dtype=torch.int32), device, resident=True), n_blocks))
    tiles = h2d(torch.tensor(rows, dtype=torch.int32).reshape(-1, 8), device, resident=True)
    comb_t = h2d(torch.tensor(comb if comb else [0, 0, 0, 0], dtype=torch.int32), device, resident=True)
    return AttnPlan(tiles, n_tiles, phases, comb_t, len(comb) // 4, n_slots, tile_rows, device)


def flash_attn(q, k, v, out, plan, Hq, Hkv, D, scale=None, phase=None):
    """q [Lq, >=Hq*D] / k,v [Lk, >=Hkv*D] bf16 row-major views (strides in elements); out [Lq, Hq*D] bf16.
    phase=None: every phase of the plan, then the merge; phase=i: that launch only (the merge follows the last one)."""
    scale = scale if scale is not None else D ** -0.5
    ws = plan.ws(scratch_owner(q.device.index))
    last = len(plan.phases) - 1
    for i in (range(len(plan.phases)) if phase is None else (phase,)):
        segs, seg_ptr, n_blocks = plan.phases[i]
        n_comb = plan.n_comb if i == last else 0
        _ck(lib().g2v_flash_attn(_p(q), _rowmajor(q), _p(k), _rowmajor(k), _p(v), _rowmajor(v), _p(out), _rowmajor(out),
                                 _p(plan.tiles), plan.n_tiles, Hq, Hkv, D, scale, _p(segs), _p(seg_ptr), n_blocks, _p(plan.comb), n_comb,
                                 plan.tile_rows, _p(ws), _stream()), "g2v_flash_attn")
    return out


def rope2d(x, col0, n_heads, D, cos, sin, pos, P):
    _ck(lib().g2v_rope2d(_p(x), _rowmajor(x), x.shape[0], col0, n_heads, D, _p(cos), _p(sin), _p(pos), P, _stream()),
        "g2v_rope2d")


def rope_vision(x, n_heads, D, cos, sin):
    _ck(lib().g2v_rope_vision(_p(x), _rowmajor(x), x.shape[0], n_heads, D, _p(cos), _p(sin), _stream()), "g2v_rope_vision")


# ------------------------------------------------------------------------------------- data movers
def im2col14(img, Kpad=640):
    N, _, H, W = img.shape
    out = torch.empty((N * (H // 14) * (W // 14), Kpad), dtype=torch.bfloat16, device=img.device)
    _ck(lib().g2v_im2col14(_p(img), N, H, W, _p(out), Kpad, _stream()), "g2v_im2col14")
    return out


def dino_preprocess(frames, mean, std, want_orig=True):
    """frames: uint8 [N,H,W,3] or fp32 [N,3,H,W] in [0,1], on the device -> (normalised fp32 [N,3,H,W], original fp32
    [N,3,H,W] or None); see g2v_dino_preprocess."""
    u8 = frames.dtype == torch.uint8
    if u8:
        N, H, W, _ = frames.shape
    else:
        assert frames.dtype == torch.float32
        N, _, H, W = frames.shape
    frames = frames.contiguous()
    norm = torch.empty((N, 3, H, W), dtype=torch.float32, device=frames.device)
    orig = torch.empty_like(norm) if want_orig else None      # a copy, as the reference's .clone() (g2vlm.py:952)
    m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    _ck(lib().g2v_dino_preprocess(_p(frames), int(u8), N, H, W, m3, s3, _p(norm), _p(orig), _stream()),
        "g2v_dino_preprocess")
    return norm, orig


def dino_assemble(patch, cls, regs, pos, N, P):
    Cc = patch.shape[1]
    x = torch.empty((N * (P + 5), Cc), dtype=torch.float32, device=patch.device)
    _ck(lib().g2v_dino_assemble(_p(patch), _p(cls), _p(regs), _p(pos), _p(x), N, P, Cc, _stream()), "g2v_dino_assemble")
    return x


def im2col_patch(img, patch, Kpad):
    N, _, H, W = img.shape
    out = torch.empty((N * (H // patch) * (W // patch), Kpad), dtype=torch.bfloat16, device=img.device)
    _ck(lib().g2v_im2col_patch(_p(img), N, H, W, patch, _p(out), Kpad, _stream()), "g2v_im2col_patch")
    return out


def vit_assemble(patch, cls, regs, N, P, R):
    Cc = patch.shape[1]
    x = torch.empty((N * (P + 1 + R), Cc), dtype=torch.float32, device=patch.device)
    _ck(lib().g2v_vit_assemble(_p(patch), _p(cls), _p(regs), _p(x), N, P, R, Cc, _stream()), "g2v_vit_assemble")
    return x


def qwen_patchify_u8(frames_u8, mean, std, Kpad):
    """frames_u8 uint8 [F,H,W,3] on the device -> bf16 [T, Kpad] patch matrix (see g2v_qwen_patchify_u8)."""
    Fn, H, W, _ = frames_u8.shape
    out = torch.empty((((Fn + 1) // 2) * (H // 14) * (W // 14), Kpad), dtype=torch.bfloat16, device=frames_u8.device)
    m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    _ck(lib().g2v_qwen_patchify_u8(_p(frames_u8), Fn, H, W, m3, s3, _p(out), Kpad, _stream()), "g2v_qwen_patchify_u8")
    return out


def gather_rows(src, idx_i32, out):
    _ck(lib().g2v_gather_rows_f32(_p(src), _rowmajor(src), _p(idx_i32), _p(out), _rowmajor(out), idx_i32.numel(),
                                  src.shape[1], _stream()), "g2v_gather_rows_f32")
    return out


def scatter_rows(src, idx_i32, out):
    _ck(lib().g2v_scatter_rows_f32(_p(src), _rowmajor(src), _p(idx_i32), _p(out), _rowmajor(out), idx_i32.numel(),
                                   src.shape[1], _stream()), "g2v_scatter_rows_f32")
    return out


def cast_bf16(x):
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _ck(lib().g2v_cast_f32_bf16(_p(x), _p(out), x.numel(), _stream()), "g2v_cast_f32_bf16")
    return out


def cast_f32(x):
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _ck(lib().g2v_cast_bf16_f32(_p(x), _p(out), x.numel(), _stream()), "g2v_cast_bf16_f32")
    return out


_LANCZOS_DEV = {}


def lanczos_resize_u8(frames, out_h, out_w):
    """PIL's LANCZOS resize of uint8 RGB frames [N, H, W, 3] on the device, bit-exact (g2v_lanczos_resize_u8); the tap
    tables come from host.lanczos_tables and stay resident per (device, in size, out size)."""
    from . import host
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3 and frames.is_contiguous()
    N, H, W, _ = frames.shape
    if (H, W) == (out_h, out_w):
        return frames.clone()                                # Image.resize returns a copy when the size is unchanged
    tabs = []
    for n_in, n_out in ((W, out_w), (H, out_h)):
        key = (frames.device, n_in, n_out)
        if n_in != n_out and key not in _LANCZOS_DEV:
            b, k = host.lanczos_tables(n_in, n_out)
            _LANCZOS_DEV[key] = (h2d(b, frames.device, resident=True), h2d(k, frames.device, resident=True), k.shape[1])
        tabs.append(_LANCZOS_DEV.get(key, (None, None, 0)) if n_in != n_out else (None, None, 0))
    out = torch.empty((N, out_h, out_w, 3), dtype=torch.uint8, device=frames.device)
    tmp = torch.empty((N, H, out_w, 3), dtype=torch.uint8, device=frames.device) if (W != out_w and H != out_h) else None
    (bh, kh, nh), (bv, kv, nv) = tabs
    _ck(lib().g2v_lanczos_resize_u8(_p(frames), N, H, W, _p(out), out_h, out_w, _p(tmp), _p(bh), _p(kh), nh, _p(bv), _p(kv), nv, _stream()),
        "g2v_lanczos_resize_u8")
    return out


def pts_epilogue(feat, N, H, W, mode, pose=None, patch=14):
    assert feat.shape == (N * (H // patch) * (W // patch), 3 * patch * patch) and feat.dtype == torch.float32
    out = torch.empty((N, H, W, 3), dtype=torch.float32, device=feat.device)
    out2 = torch.empty_like(out) if mode == 1 else None
    _ck(lib().g2v_pts_epilogue_ps(_p(feat), N, H, W, patch, mode, _p(pose), _p(out), _p(out2), _stream()), "g2v_pts_epilogue_ps")
    return out, out2


def pixel_shuffle(feat, N, H, W, C_, patch=14):
    assert feat.shape == (N * (H // patch) * (W // patch), C_ * patch * patch) and feat.dtype == torch.float32
    out = torch.empty((N, H, W, C_), dtype=torch.float32, device=feat.device)
    _ck(lib().g2v_pixel_shuffle(_p(feat), N, H, W, C_, patch, _p(out), _stream()), "g2v_pixel_shuffle")
    return out


def pixel_shuffle14(feat, N, H, W, C_):
    return pixel_shuffle(feat, N, H, W, C_, 14)


def camera_tail(feat, N, P, w0, b0, w1, b1, wt, bt, wr, br):
    pose = torch.empty((N, 4, 4), dtype=torch.float32, device=feat.device)
    _ck(lib().g2v_camera_tail(_p(feat), N, P, _p(w0), _p(b0), _p(w1), _p(b1), _p(wt), _p(bt), _p(wr), _p(br), _p(pose),
                              _stream()), "g2v_camera_tail")
    return pose


_argmax_scratch = {}


def argmax_bf16(x, out, scratch=None):
    if scratch is None:
        # one ticket word per scratch_owner: two streams (or two host threads) reducing at once must not share it
        key = scratch_owner(x.device.index)
        scratch = _argmax_scratch.get(key)
        if scratch is None:
            scratch = _argmax_scratch[key] = torch.zeros(129, dtype=torch.int32, device=x.device)
    _ck(lib().g2v_argmax_bf16(_p(x), x.numel(), _p(out), _p(scratch), _stream()), "g2v_argmax_bf16")
    return out


# ------------------------------------------------------------------------------------------ decode
def gemv_bf16(x, w, bias=None, out=None, res=None):
    """y = bf16(w[N,K] . x[K] + bias); res (f32, in place) += y if given, else out (bf16) = y."""
    N, K = w.shape
    _ck(lib().g2v_gemv_bf16(_p(x), _p(w), _p(bias), _p(out), _p(res), N, K, _stream()), "g2v_gemv_bf16")
    return res if res is not None else out


def gemv_rmsnorm_bf16(x_f32, norm_w, eps, w, bias, out):
    """out = bf16(W . bf16(rmsnorm(x_f32)) + bias): input norm fused into the weight-streaming GEMV."""
    N, K = w.shape
    _ck(lib().g2v_gemv_rmsnorm_bf16(_p(x_f32), _p(norm_w), eps, _p(w), _p(bias), _p(out), N, K, _stream()), "g2v_gemv_rmsnorm_bf16")
    return out


def gemv_rmsnorm_swiglu_bf16(x_f32, norm_w, eps, w_gu, act_out):
    """act_out bf16[F] = SwiGLU(W_gu . bf16(rmsnorm(x_f32))): norm, gate/up GEMV and activation in one launch."""
    N2, K = w_gu.shape
    _ck(lib().g2v_gemv_rmsnorm_swiglu_bf16(_p(x_f32), _p(norm_w), eps, _p(w_gu), _p(act_out), N2, K, _stream()),
        "g2v_gemv_rmsnorm_swiglu_bf16")
    return act_out


def gemv_swiglu_bf16(gu, w, res):
    """res (f32, in place) += bf16(W . swiglu(gu)): activation fused into the down-projection GEMV."""
    N, K = w.shape
    _ck(lib().g2v_gemv_swiglu_bf16(_p(gu), _p(w), _p(res), N, K, _stream()), "g2v_gemv_swiglu_bf16")
    return res


def gemv_pg(x, w, norm_w=None, eps=0.0, bias=None, out=None, res=None, act=False):
    """Persistent-grid GEMV of the decode step (g2v_gemv_pg): y = w[N,K] . x with the fused RMSNorm / SwiGLU / residual forms."""
    N, K = w.shape
    _ck(lib().g2v_gemv_pg(_p(x), _p(norm_w), float(eps), _p(w), _p(bias), _p(out), _p(res), N, K, int(act), _stream()), "g2v_gemv_pg")
    return res if res is not None else out


def gemv_pg_batch(x, w, norm_w=None, eps=0.0, bias=None, out=None, res=None, act=False):
    """g2v_gemv_pg_batch: Y[B,N] = x[B,K] . w[N,K]^T for B <= 8 decode rows, weights streamed once; fused forms as gemv_pg."""
    N, K = w.shape
    B = x.shape[0]
    assert x.dim() == 2 and x.shape[1] == K and x.is_contiguous() and (x.dtype == torch.float32) == (norm_w is not None)
    tgt = res if res is not None else out
    assert tgt.is_contiguous() and tgt.shape == (B, N // 2 if act else N)
    _ck(lib().g2v_gemv_pg_batch(_p(x), _p(norm_w), float(eps), _p(w), _p(bias), _p(out), _p(res), B, N, K, int(act), _stream()),
        "g2v_gemv_pg_batch")
    return tgt


def gemv_pg_route(B, N, K, act=False, norm=False, fp8=False):
    """What gemv_pg / gemv_pg_fp8 (B == 0) or gemv_pg_batch / gemv_pg_batch_fp8 (B = 1..8 rows) launch for a [N, K] weight,
    without a device: (form, threads per block, RB, KCH) with form 1 = gemv_pg*, 2 = gemv_pgb*, 3 = gemv_pgk* kernels (form 3:
    RB is the kernel's R and KCH its CW in bf16, S in e4m3).  Raises HipError where the entry point refuses the shape."""
    out = (C.c_int32 * 4)()
    _ck(lib().g2v_gemv_pg_route(int(B), int(N), int(K), int(act), int(norm), int(fp8), C.byref(out)), "g2v_gemv_pg_route")
    return tuple(out)


def gemv_pg_fp8(x, wq, wscale, norm_w=None, eps=0.0, bias=None, out=None, res=None, act=False):
    """g2v_gemv_pg_fp8: gemv_pg with the weight as e4m3 codes wq uint8 [N,K] and one power-of-two scale per row wscale f32 [N]
    (g2vlm_amd.quant.quantize_rows_e4m3); the result is gemv_pg's on dequantize_rows(wq, wscale) up to the fp32 summation order."""
    N, K = wq.shape
    assert wq.dtype == torch.uint8 and wq.is_contiguous() and wscale.dtype == torch.float32 and wscale.shape == (N,)
    _ck(lib().g2v_gemv_pg_fp8(_p(x), _p(norm_w), float(eps), _p(wq), _p(wscale), _p(bias), _p(out), _p(res), N, K, int(act), _stream()),
        "g2v_gemv_pg_fp8")
    return res if res is not None else out


def gemv_pg_batch_fp8(x, wq, wscale, norm_w=None, eps=0.0, bias=None, out=None, res=None, act=False):
    """g2v_gemv_pg_batch_fp8: gemv_pg_batch (B <= 8 rows, weights streamed once) with e4m3 weights as gemv_pg_fp8."""
    N, K = wq.shape
    B = x.shape[0]
    assert wq.dtype == torch.uint8 and wq.is_contiguous() and wscale.dtype == torch.float32 and wscale.shape == (N,)
    assert x.dim() == 2 and x.shape[1] == K and x.is_contiguous() and (x.dtype == torch.float32) == (norm_w is not None)
    tgt = res if res is not None else out
    assert tgt.is_contiguous() and tgt.shape == (B, N // 2 if act else N)
    _ck(lib().g2v_gemv_pg_batch_fp8(_p(x), _p(norm_w), float(eps), _p(wq), _p(wscale), _p(bias), _p(out), _p(res), B, N, K, int(act),
                                    _stream()), "g2v_gemv_pg_batch_fp8")
    return tgt


def decode_attn_pg_workspace(Hq, Hkv, batch=1):
    return int(lib().g2v_decode_attn_pg_workspace(Hq, Hkv, batch))


def decode_attn_pg(qkv, qw, kw, eps, und_rounding, cos, sin, k_cache, v_cache, out, len_dev, scene_rows, max_len, Hq, Hkv, scale,
                   workspace):
    """g2v_decode_attn_pg: as decode_attn_fused, on a grid of 256 equal shares of the max_len cache rows per scene."""
    _ck(lib().g2v_decode_attn_pg(_p(qkv), _p(qw), _p(kw), eps, int(und_rounding), _p(cos), _p(sin), _p(k_cache), _p(v_cache), _p(out),
                                 _p(len_dev), qkv.shape[0], int(scene_rows), int(max_len), Hq, Hkv, scale, _p(workspace), _stream()),
        "g2v_decode_attn_pg")
    return out


def kv_quant_e4m3(src, codes, scales):
    """g2v_kv_quant_e4m3: src bf16 [rows, Hkv, 128] -> codes uint8 [rows, Hkv, 128] and scales f32 [rows, Hkv], both written in
    place: g2vlm_amd.quant.quantize_rows_e4m3 on the rows viewed as [rows * Hkv, 128]."""
    rows, Hkv, D = src.shape
    assert D == 128 and src.dtype == torch.bfloat16 and codes.dtype == torch.uint8 and scales.dtype == torch.float32
    assert src.is_contiguous() and codes.is_contiguous() and scales.is_contiguous()
    assert codes.shape == src.shape and scales.shape == (rows, Hkv)
    if rows:
        _ck(lib().g2v_kv_quant_e4m3(_p(src), rows, Hkv, _p(codes), _p(scales), _stream()), "g2v_kv_quant_e4m3")
    return codes, scales


def kv_dequant_e4m3(codes, scales, out=None):
    """g2v_kv_dequant_e4m3: codes uint8 [rows, Hkv, 128], scales f32 [rows, Hkv] -> bf16 [rows, Hkv, 128] = codes * scales, exact."""
    rows, Hkv, D = codes.shape
    if out is None:
        out = torch.empty(codes.shape, dtype=torch.bfloat16, device=codes.device)
    assert D == 128 and out.dtype == torch.bfloat16 and codes.dtype == torch.uint8 and scales.dtype == torch.float32
    assert out.is_contiguous() and codes.is_contiguous() and scales.is_contiguous()
    assert out.shape == codes.shape and scales.shape == (rows, Hkv)
    if rows:
        _ck(lib().g2v_kv_dequant_e4m3(_p(codes), _p(scales), rows, Hkv, _p(out), _stream()), "g2v_kv_dequant_e4m3")
    return out


def decode_attn_pg_kv8(qkv, qw, kw, eps, und_rounding, cos, sin, k_codes, v_codes, k_scale, v_scale, out, len_dev, scene_rows, max_len,
                       Hq, Hkv, scale, workspace):
    """g2v_decode_attn_pg_kv8: decode_attn_pg over an e4m3 cache (codes uint8 [B, scene_rows, Hkv, 128], scales f32
    [B, scene_rows, Hkv]); the new token's K / V rows are appended quantised and attended to as their dequantised values."""
    assert k_codes.dtype == torch.uint8 and v_codes.dtype == torch.uint8 and k_scale.dtype == torch.float32 and v_scale.dtype == torch.float32
    _ck(lib().g2v_decode_attn_pg_kv8(_p(qkv), _p(qw), _p(kw), eps, int(und_rounding), _p(cos), _p(sin), _p(k_codes), _p(v_codes),
                                     _p(k_scale), _p(v_scale), _p(out), _p(len_dev), qkv.shape[0], int(scene_rows), int(max_len), Hq, Hkv,
                                     scale, _p(workspace), _stream()),
        "g2v_decode_attn_pg_kv8")
    return out


def decode_attn_shared_workspace(Hq, Hkv, batch, prefix_len, suffix_max_len):
    return int(lib().g2v_decode_attn_shared_workspace(Hq, Hkv, batch, prefix_len, suffix_max_len))


def decode_attn_shared(qkv, qw, kw, eps, und_rounding, cos, sin, k_prefix, v_prefix, prefix_len, k_suffix, v_suffix, suffix_len_dev,
                       suffix_rows, suffix_max_len, Hq, Hkv, scale, out, workspace):
    """g2v_decode_attn_shared: decode_attn_pg for B slots over one shared, read-only prefix [0, prefix_len) of
    k_prefix / v_prefix plus a suffix block per slot (k_suffix / v_suffix [B, suffix_rows, Hkv, 128], lengths on the device,
    the new token included); the prefix rows are read once per column group of slots, not once per slot."""
    _ck(lib().g2v_decode_attn_shared(_p(qkv), _p(qw), _p(kw), eps, int(und_rounding), _p(cos), _p(sin), _p(k_prefix), _p(v_prefix),
                                     int(prefix_len), _p(k_suffix), _p(v_suffix), _p(suffix_len_dev), qkv.shape[0], int(suffix_rows),
                                     int(suffix_max_len), Hq, Hkv, scale, _p(out), _p(workspace), _stream()),
        "g2v_decode_attn_shared")
    return out


def decode_attn_workspace(Lk, Hq):
    return int(lib().g2v_decode_attn_workspace(Lk, Hq))


def decode_attn(q, k_cache, v_cache, out, Lk, Hq, Hkv, scale, workspace):
    _ck(lib().g2v_decode_attn(_p(q), _p(k_cache), _p(v_cache), _p(out), Lk, Hq, Hkv, scale, _p(workspace), _stream()),
        "g2v_decode_attn")
    return out


def decode_attn_dyn(q, k_cache, v_cache, out, len_dev, max_len, Hq, Hkv, scale, workspace):
    _ck(lib().g2v_decode_attn_dyn(_p(q), _p(k_cache), _p(v_cache), _p(out), _p(len_dev), max_len, Hq, Hkv, scale,
                                  _p(workspace), _stream()), "g2v_decode_attn_dyn")
    return out


def decode_advance(pos3, row, length):
    _ck(lib().g2v_decode_advance(_p(pos3), _p(row), _p(length), _stream()), "g2v_decode_advance")


def decode_attn_batch(q, k_cache, v_cache, out, len_dev, scene_rows, max_len, Hq, Hkv, scale, workspace):
    """q / out [B, Hq*128]; caches [B, scene_rows, Hkv, 128]; len_dev int32 [B]."""
    _ck(lib().g2v_decode_attn_batch(_p(q), _p(k_cache), _p(v_cache), _p(out), _p(len_dev), q.shape[0], int(scene_rows), max_len, Hq,
                                    Hkv, scale, _p(workspace), _stream()), "g2v_decode_attn_batch")
    return out


def decode_attn_fused(qkv, qw, kw, eps, und_rounding, cos, sin, k_cache, v_cache, out, len_dev, scene_rows, max_len, Hq, Hkv, scale,
                      workspace):
    """Attention of one decode step with q/k-norm, mRoPE and the cache append folded in.  qkv [B, (Hq+2Hkv)*128] raw."""
    _ck(lib().g2v_decode_attn_fused(_p(qkv), _p(qw), _p(kw), eps, int(und_rounding), _p(cos), _p(sin), _p(k_cache), _p(v_cache),
                                    _p(out), _p(len_dev), qkv.shape[0], int(scene_rows), max_len, Hq, Hkv, scale, _p(workspace),
                                    _stream()), "g2v_decode_attn_fused")
    return out


def decode_advance_batch(pos3, row, length):
    _ck(lib().g2v_decode_advance_batch(_p(pos3), _p(row), _p(length), row.numel(), _stream()), "g2v_decode_advance_batch")


def argmax_rows_bf16(x, out, scratch):
    """x bf16 [rows, n] (row stride >= n); out int32 [rows]; scratch int32 [rows*129] zeroed once."""
    _ck(lib().g2v_argmax_rows_bf16(_p(x), x.shape[0], x.shape[1], _rowmajor(x), _p(out), _p(scratch), _stream()), "g2v_argmax_rows_bf16")
    return out


def make_rng(seed, temperature, device):
    """Device-side sampler state of g2v_sample_rows_bf16: int32[4] = {seed lo, seed hi, step = 0, float bits of 1 / T}."""
    import struct
    if not temperature > 0:
        raise ValueError("temperature must be > 0")
    seed = int(seed) & (2 ** 64 - 1)
    to_i32 = lambda v: v - (1 << 32) if v >= (1 << 31) else v     # noqa: E731
    words = [to_i32(seed & 0xffffffff), to_i32(seed >> 32), 0, struct.unpack("<i", struct.pack("<f", 1.0 / float(temperature)))[0]]
    return h2d(torch.tensor(words, dtype=torch.int32), device)


def sample_rows_bf16(x, out, scratch, rng):
    """x bf16 [rows, n]: out[r] ~ softmax(x[r] / T) (reference g2vlm.py:1119-1122); advances rng's step word."""
    if x.dim() == 1:
        x = x.view(1, -1)
    _ck(lib().g2v_sample_rows_bf16(_p(x), x.shape[0], x.shape[1], _rowmajor(x), _p(out), _p(scratch), _p(rng), _stream()),
        "g2v_sample_rows_bf16")
    return out


_logprob_scratch = {}
LOGPROB_WS_WORDS = 1 << 16


def logprob_rows_workspace(rows, n):
    """Bytes of scratch with which g2v_logprob_rows_bf16 deals the rows of a [rows, n] launch out to several workgroups each
    (0: it would not)."""
    return int(lib().g2v_logprob_rows_workspace(int(rows), int(n)))


def logprob_rows_bf16(logits, targets, lse=None, rank=None, out=None, scratch=None):
    """out[r] = log_softmax(logits[r].float(), -1)[targets[r]] (g2v_logprob_rows_bf16): logits bf16 [rows, n] (row stride >= n),
    targets int32 [rows]; lse fp32 [rows] / rank int32 [rows], when given, receive the row's logsumexp and the target's rank
    (0: the argmax).  A target outside [0, n) gives NaN and rank -1.  Returns out (fp32 [rows], allocated when None).
    scratch: int32, zeroed once, >= logprob_rows_workspace(rows, n) bytes when the caller owns one (a captured graph must not
    allocate); else one per scratch_owner, as the argmax ticket.  The results do not depend on it.
    A row whose entries are all -inf gives -inf for both (torch: NaN)."""
    rows, n = logits.shape
    assert logits.dtype == torch.bfloat16 and targets.dtype == torch.int32 and targets.numel() == rows and targets.is_contiguous()
    if out is None:
        out = torch.empty(rows, dtype=torch.float32, device=logits.device)
    assert out.dtype == torch.float32 and out.numel() == rows and out.is_contiguous()
    assert lse is None or (lse.dtype == torch.float32 and lse.numel() == rows and lse.is_contiguous())
    assert rank is None or (rank.dtype == torch.int32 and rank.numel() == rows and rank.is_contiguous())
    if scratch is None and logprob_rows_workspace(rows, n):
        # one per scratch_owner, allocated once at a fixed size and never replaced (a captured graph keeps its pointer): 256 KiB
        # cover 511 rows of the 151 936-entry vocabulary (118 KB); a launch that would need more gets none and runs one
        # workgroup per row, which gives the same bits
        key = scratch_owner(logits.device.index)
        scratch = _logprob_scratch.get(key)
        if scratch is None:
            scratch = _logprob_scratch[key] = torch.zeros(LOGPROB_WS_WORDS, dtype=torch.int32, device=logits.device)
    _ck(lib().g2v_logprob_rows_bf16(_p(logits), rows, n, _rowmajor(logits), _p(targets), _p(out), _p(lse), _p(rank), _p(scratch),
                                    scratch.numel() * 4 if scratch is not None else 0, _stream()), "g2v_logprob_rows_bf16")
    return out


_topk_scratch = {}
TOPK_MAX = 32                                               # G2V_TOPK_MAX
TOPK_WS_WORDS = 1 << 17                                     # 512 KiB: every split launch (< 512 rows, k <= 32) fits


def topk_rows_workspace(rows, n, k):
    """Bytes of scratch with which g2v_topk_rows_bf16 deals the rows of a [rows, n] launch out to several workgroups each
    (0: it would not)."""
    return int(lib().g2v_topk_rows_workspace(int(rows), int(n), int(k)))


def topk_rows_bf16(logits, k, out_idx=None, out_val=None, scratch=None):
    """The first k entries of every row of bf16 logits [rows, n] (row stride >= n) in argmax_rows_bf16's order - larger first,
    -0 == +0, NaN on top, equal values by ascending index (g2v_topk_rows_bf16): returns (idx int32 [rows, k], val fp32
    [rows, k]), allocated when None; idx[:, 0] is the argmax, val the selected elements themselves.  k > n leaves index -1 /
    value NaN behind the n entries.  1 <= k <= 32.
    scratch: int32, zeroed once, >= topk_rows_workspace(rows, n, k) bytes when the caller owns one (a captured graph must not
    allocate); else one per scratch_owner, as logprob_rows_bf16's.  The results do not depend on it."""
    rows, n = logits.shape
    k = int(k)
    assert logits.dtype == torch.bfloat16
    if not 1 <= k <= TOPK_MAX:
        raise ValueError(f"topk_rows_bf16: k = {k}, 1..{TOPK_MAX}")
    if out_idx is None:
        out_idx = torch.empty((rows, k), dtype=torch.int32, device=logits.device)
    if out_val is None:
        out_val = torch.empty((rows, k), dtype=torch.float32, device=logits.device)
    assert out_idx.dtype == torch.int32 and tuple(out_idx.shape) == (rows, k) and out_idx.is_contiguous()
    assert out_val.dtype == torch.float32 and tuple(out_val.shape) == (rows, k) and out_val.is_contiguous()
    if scratch is None and topk_rows_workspace(rows, n, k):
        key = scratch_owner(logits.device.index)
        scratch = _topk_scratch.get(key)
        if scratch is None:
            scratch = _topk_scratch[key] = torch.zeros(TOPK_WS_WORDS, dtype=torch.int32, device=logits.device)
    _ck(lib().g2v_topk_rows_bf16(_p(logits), rows, n, _rowmajor(logits), k, _p(out_idx), _p(out_val), _p(scratch),
                                 scratch.numel() * 4 if scratch is not None else 0, _stream()), "g2v_topk_rows_bf16")
    return out_idx, out_val


# ------------------------------------------------------------------------------------------ point-cloud export (csrc/cloud.hip)
CLOUD_FINITE, CLOUD_CONF, CLOUD_EDGE_ATOL, CLOUD_EDGE_RTOL = 1, 2, 4, 8       # G2V_CLOUD_*
_cloud_ws = {}


def _cloud_workspace(nbytes, device, tag):
    """Scratch of the compaction's block counts / the fit's partial sums: one per scratch_owner and use, grown when a launch
    needs more (it carries nothing from one call to the next and needs no zeroing)."""
    key = scratch_owner(device.index) + (tag,)
    ws = _cloud_ws.get(key)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = _cloud_ws[key] = torch.empty(max((nbytes + 7) // 8, 1), dtype=torch.int64, device=device)
    return ws


def _workspace_arg(workspace, nbytes, device, tag):
    """(workspace, the bytes to pass for it): the caller's own, or the scratch owner's buffer for `tag`, grown to nbytes."""
    if workspace is None:
        workspace = _cloud_workspace(nbytes, device, tag)
    return workspace, workspace.numel() * workspace.element_size()


def _nhw3(t, what):
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[3] == 3 and t.is_contiguous(), f"{what}: fp32 [N,H,W,3], contiguous"
    return tuple(t.shape[:3])


def _mask_u8(mask, shape, what="mask", optional=False):
    """mask as uint8 of `shape` (a bool mask is viewed, not copied); None passes where optional (all pixels / points)."""
    if mask is None and optional:
        return None
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    dims = "[N,H,W]" if len(shape) == 3 else str(list(shape))
    assert mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == tuple(shape) and mask.is_contiguous(), f"{what}: uint8 {dims}"
    return mask


def _colors_n3hw(colors, N, H, W):
    assert colors.is_cuda and colors.dtype == torch.float32 and tuple(colors.shape) == (N, 3, H, W) and colors.is_contiguous(), \
        "colors: fp32 [N,3,H,W], contiguous"


def cloud_mask(points=None, local=None, conf=None, conf_logit_min=0.0, edge_atol=None, edge_rtol=None, finite=True, out=None):
    """Keep mask uint8 [N,H,W] of recon's pointmaps (g2v_cloud_mask): 1 where every enabled test passes.
    finite: the three coordinates of points fp32 [N,H,W,3] are finite.  conf fp32 [N,H,W] given: conf > conf_logit_min as an
    fp32 compare (logits; NaN fails).  edge_atol / edge_rtol given: not an edge of local[..., 2] under the reference's
    depth_edge rule (3x3 window; local fp32 [N,H,W,3])."""
    flags = (CLOUD_FINITE if finite else 0) | (CLOUD_CONF if conf is not None else 0) | \
        (CLOUD_EDGE_ATOL if edge_atol is not None else 0) | (CLOUD_EDGE_RTOL if edge_rtol is not None else 0)
    edge = flags & (CLOUD_EDGE_ATOL | CLOUD_EDGE_RTOL)
    shapes = []
    if finite:
        shapes.append(_nhw3(points, "points"))
    if edge:
        shapes.append(_nhw3(local, "local"))
    if conf is not None:
        assert conf.is_cuda and conf.dtype == torch.float32 and conf.dim() == 3 and conf.is_contiguous(), "conf: fp32 [N,H,W], contiguous"
        shapes.append(tuple(conf.shape))
    assert shapes, "cloud_mask: no test enabled and no input to take the shape from"
    assert all(s == shapes[0] for s in shapes), f"cloud_mask: inputs disagree on [N,H,W]: {shapes}"
    N, H, W = shapes[0]
    dev = (points if finite else local if edge else conf).device
    if out is None:
        out = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (N, H, W) and out.is_contiguous()
    _ck(lib().g2v_cloud_mask(_p(points) if finite else None, _p(local) if edge else None, _p(conf), N, H, W, flags, float(conf_logit_min),
                             float(edge_atol or 0.0), float(edge_rtol or 0.0), _p(out), _stream()), "g2v_cloud_mask")
    return out


def cloud_compact_workspace(N, H, W):
    return int(lib().g2v_cloud_compact_workspace(int(N), int(H), int(W)))


def cloud_compact(points, colors, mask, workspace=None):
    """The pixels mask keeps as packed PLY records (g2v_cloud_compact): points fp32 [N,H,W,3], colors fp32 [N,3,H,W] in [0,1],
    mask uint8 or bool [N,H,W] -> (records uint8 [M,15] = <f4 x,y,z + u1 r,g,b in view-major, row-major order, counts int32
    [N]).  Synchronous: the total M is read back once to size the result (a view of a buffer of N*H*W records)."""
    N, H, W = _nhw3(points, "points")
    _colors_n3hw(colors, N, H, W)
    mask = _mask_u8(mask, (N, H, W))
    workspace, ws_bytes = _workspace_arg(workspace, cloud_compact_workspace(N, H, W), points.device, "compact")
    cap = N * H * W
    records = torch.empty((cap, 15), dtype=torch.uint8, device=points.device)
    counts = torch.empty(N, dtype=torch.int32, device=points.device)
    _ck(lib().g2v_cloud_compact(_p(points), _p(colors), _p(mask), N, H, W, _p(records), cap, _p(counts), _p(workspace),
                                ws_bytes, _stream()), "g2v_cloud_compact")
    m = int(counts.sum(dtype=torch.int64).item())
    return records[:m], counts


def cloud_counts(points, colors, mask, workspace=None):
    """counts int32 [N] of cloud_compact alone: g2v_cloud_compact with room for no record (it then only counts)."""
    N, H, W = _nhw3(points, "points")
    mask = _mask_u8(mask, (N, H, W))
    workspace, ws_bytes = _workspace_arg(workspace, cloud_compact_workspace(N, H, W), points.device, "compact")
    counts = torch.empty(N, dtype=torch.int32, device=points.device)
    _ck(lib().g2v_cloud_compact(_p(points), _p(colors), _p(mask), N, H, W, None, 0, _p(counts), _p(workspace),
                                ws_bytes, _stream()), "g2v_cloud_compact")
    return counts


def intrinsics_lsq_workspace(N, H, W):
    return int(lib().g2v_intrinsics_lsq_workspace(int(N), int(H), int(W)))


def intrinsics_lsq(local, mask=None, workspace=None):
    """Per view the least-squares pinhole matrix of local points fp32 [N,H,W,3] (g2v_intrinsics_lsq): u = fx X/Z + cx,
    v = fy Y/Z + cy over pixel centres (x + 0.5, y + 0.5) and the pixels mask keeps (None: all) with finite X, Y, Z and Z > 0.
    Returns (K fp32 [N,3,3], used int32 [N]); entries that the pixels do not determine are NaN.  Bit-reproducible."""
    N, H, W = _nhw3(local, "local")
    mask = _mask_u8(mask, (N, H, W), optional=True)
    workspace, ws_bytes = _workspace_arg(workspace, intrinsics_lsq_workspace(N, H, W), local.device, "intrinsics")
    K = torch.empty((N, 3, 3), dtype=torch.float32, device=local.device)
    used = torch.empty(N, dtype=torch.int32, device=local.device)
    _ck(lib().g2v_intrinsics_lsq(_p(local), _p(mask), N, H, W, _p(K), _p(used), _p(workspace), ws_bytes, _stream()), "g2v_intrinsics_lsq")
    return K, used


def cloud_consistency_workspace(N, H, W):
    return int(lib().g2v_cloud_consistency_workspace(int(N), int(H), int(W)))


def cloud_consistency(points, local, mask, poses, K, depth_rtol, min_agree=0, max_in_front=-1, pairs=False, workspace=None):
    """Per pixel, in how many OTHER views its world point is confirmed / floats in front of the surface (g2v_cloud_consistency;
    include/g2vlm_hip.h has the exact rule): points, local fp32 [N,H,W,3], mask uint8 or bool [N,H,W] or None (all pixels), poses
    fp32 [N,4,4] camera-to-world, K fp32 [N,3,3], N <= 256.  Returns (agree uint8 [N,H,W], in_front uint8 [N,H,W], mask_out
    uint8 [N,H,W] = eligible and agree >= min_agree and (max_in_front < 0 or in_front <= max_in_front), pairs int32 [N,N,2] or
    None).  Bit-reproducible; no host synchronisation."""
    N, H, W = _nhw3(points, "points")
    assert _nhw3(local, "local") == (N, H, W), "local: the shape of points"
    mask = _mask_u8(mask, (N, H, W), optional=True)
    for t, shape, what in ((poses, (N, 4, 4), "poses"), (K, (N, 3, 3), "K")):
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous(), f"{what}: fp32 {list(shape)}, contiguous"
    dev = points.device
    workspace, ws_bytes = _workspace_arg(workspace, cloud_consistency_workspace(N, H, W), dev, "consistency")
    agree = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    in_front = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    mask_out = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    pair_counts = torch.empty((N, N, 2), dtype=torch.int32, device=dev) if pairs else None
    _ck(lib().g2v_cloud_consistency(_p(points), _p(local), _p(mask), _p(poses), _p(K), N, H, W, float(depth_rtol), int(min_agree),
                                    int(max_in_front), _p(agree), _p(in_front), _p(pair_counts), _p(mask_out), _p(workspace),
                                    ws_bytes, _stream()), "g2v_cloud_consistency")
    return agree, in_front, mask_out, pair_counts


# ------------------------------------------------------------------------------------------ z-buffer rendering (csrc/render.hip)
def cloud_render_workspace(M, OH, OW):
    return int(lib().g2v_cloud_render_workspace(int(M), int(OH), int(OW)))


def cloud_render(points, colors, mask, poses, K, size, radius=0, background=0, skip=None, color=True, depth=True, index=True,
                 workspace=None):
    """The cloud seen from M target cameras through a z-buffer (g2v_cloud_render; include/g2vlm_hip.h has the exact rule): points
    fp32 [N,H,W,3], colors fp32 [N,3,H,W] (None only with color=False), mask uint8 or bool [N,H,W] or None (all pixels), poses
    fp32 [M,4,4] camera-to-world and K fp32 [M,3,3] of the targets, size = (OH, OW), radius 0..8 = the half-width of a point's
    square, background 0xRRGGBB, skip int32 [M] or None = the source view left out of each target.  Returns (color uint8
    [M,OH,OW,3], depth fp32 [M,OH,OW], index int32 [M,OH,OW] = the flat source pixel or -1), None for an output switched off.
    Bit-reproducible; no host synchronisation."""
    N, H, W = _nhw3(points, "points")
    if colors is not None:
        _colors_n3hw(colors, N, H, W)
    mask = _mask_u8(mask, (N, H, W), optional=True)
    assert poses.dim() == 3, "poses: fp32 [M,4,4]"
    M, (OH, OW) = poses.shape[0], size
    for t, shape, what in ((poses, (M, 4, 4), "poses"), (K, (M, 3, 3), "K")):
        assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == shape and t.is_contiguous(), f"{what}: fp32 {list(shape)}, contiguous"
    if skip is not None:
        assert skip.is_cuda and skip.dtype == torch.int32 and tuple(skip.shape) == (M,) and skip.is_contiguous(), "skip: int32 [M]"
    dev = points.device
    workspace, ws_bytes = _workspace_arg(workspace, cloud_render_workspace(M, OH, OW), dev, "render")
    color_out = torch.empty((M, OH, OW, 3), dtype=torch.uint8, device=dev) if color else None
    depth_out = torch.empty((M, OH, OW), dtype=torch.float32, device=dev) if depth else None
    index_out = torch.empty((M, OH, OW), dtype=torch.int32, device=dev) if index else None
    _ck(lib().g2v_cloud_render(_p(points), _p(colors), _p(mask), N, H, W, _p(poses), _p(K), _p(skip), M, int(OH), int(OW), int(radius),
                               int(background), _p(color_out), _p(depth_out), _p(index_out), _p(workspace),
                               ws_bytes, _stream()), "g2v_cloud_render")
    return color_out, depth_out, index_out


# ------------------------------------------------------------------------------------------ triangle-mesh export (csrc/mesh.hip)
MESH_MAX_EDGE = 1                                           # G2V_MESH_MAX_EDGE


def cloud_mesh_workspace(N, H, W):
    return int(lib().g2v_cloud_mesh_workspace(int(N), int(H), int(W)))


def cloud_mesh_raw(points, mask, max_edge, counts, used=None, vertex_of=None, faces=None, face_records=None, workspace=None):
    """One call of g2v_cloud_mesh into the caller's tensors (no allocation but a grown workspace, no host synchronisation):
    counts int32 [N,2] always; used uint8 [N,H,W], vertex_of int32 [N,H,W], faces int32 [cap,3], face_records uint8 [cap,13] where
    given - the capacity is that of the face tensors (0 without them: the call then only counts)."""
    N, H, W = _nhw3(points, "points")
    mask = _mask_u8(mask, (N, H, W), optional=True)
    assert counts.is_cuda and counts.dtype == torch.int32 and tuple(counts.shape) == (N, 2) and counts.is_contiguous(), "counts: int32 [N,2]"
    for t, dtype, what in ((used, torch.uint8, "used"), (vertex_of, torch.int32, "vertex_of")):
        assert t is None or (t.is_cuda and t.dtype == dtype and tuple(t.shape) == (N, H, W) and t.is_contiguous()), f"{what}: {dtype} [N,H,W]"
    cap = None
    for t, dtype, width, what in ((faces, torch.int32, 3, "faces"), (face_records, torch.uint8, 13, "face_records")):
        if t is not None:
            assert t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.shape[1] == width and t.is_contiguous(), f"{what}: {dtype} [cap,{width}]"
            assert cap is None or cap == t.shape[0], "faces and face_records: one capacity"
            cap = t.shape[0]
    workspace, ws_bytes = _workspace_arg(workspace, cloud_mesh_workspace(N, H, W), points.device, "mesh")
    _ck(lib().g2v_cloud_mesh(_p(points), _p(mask), N, H, W, MESH_MAX_EDGE if max_edge is not None else 0, float(max_edge or 0.0), _p(used),
                             _p(vertex_of), _p(faces) if cap else None, _p(face_records) if cap else None, int(cap or 0), _p(counts),
                             _p(workspace), ws_bytes, _stream()), "g2v_cloud_mesh")


def cloud_mesh(points, colors, mask, max_edge=None, faces=True, face_records=True, workspace=None):
    """The image mesh of recon's pointmaps (g2v_cloud_mesh; include/g2vlm_hip.h has the exact rule): points fp32 [N,H,W,3], colors
    fp32 [N,3,H,W], mask uint8 or bool [N,H,W] or None (all pixels), max_edge = the longest edge a triangle may have (None: no
    limit).  Returns dict(vertex_records uint8 [V,15] - g2v_cloud_compact's records of the used pixels -, faces int32 [F,3],
    face_records uint8 [F,13] (None for one switched off), used uint8 [N,H,W], vertex_of int32 [N,H,W], counts int32 [N,2]).
    Two calls: the first only counts, the face outputs are then allocated at their exact size and the second call fills them (the
    worst case is 25 bytes for each of 2 N (H-1) (W-1) candidates).  Synchronous: counts are read back once, and
    size the vertex records as well."""
    N, H, W = _nhw3(points, "points")
    _colors_n3hw(colors, N, H, W)
    dev = points.device
    counts = torch.empty((N, 2), dtype=torch.int32, device=dev)
    cloud_mesh_raw(points, mask, max_edge, counts, workspace=workspace)
    nv, nf = counts.sum(0, dtype=torch.int64).tolist()
    used = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    vertex_of = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    f = torch.empty((nf, 3), dtype=torch.int32, device=dev) if faces else None
    fr = torch.empty((nf, 13), dtype=torch.uint8, device=dev) if face_records else None
    cloud_mesh_raw(points, mask, max_edge, counts, used, vertex_of, f, fr, workspace=workspace)
    vertex_records = torch.empty((nv, 15), dtype=torch.uint8, device=dev)
    per_view = torch.empty(N, dtype=torch.int32, device=dev)
    ws, ws_bytes = _workspace_arg(None, cloud_compact_workspace(N, H, W), dev, "compact")
    _ck(lib().g2v_cloud_compact(_p(points), _p(colors), _p(used), N, H, W, _p(vertex_records) if nv else None, nv, _p(per_view), _p(ws),
                                ws_bytes, _stream()), "g2v_cloud_compact")
    return dict(vertex_records=vertex_records, faces=f, face_records=fr, used=used, vertex_of=vertex_of, counts=counts)


# ------------------------------------------------------------------------------------------ surface normals (csrc/normals.hip)
NORMALS_MAX_EDGE = 1                                        # G2V_NORMALS_MAX_EDGE
NORMALS_PLAIN, NORMALS_HALO = 2, 4                          # G2V_NORMALS_PLAIN, G2V_NORMALS_HALO (A/B and tests only)
NORMALS_STEP_MAX = 8                                        # G2V_NORMALS_STEP_MAX


def cloud_normals_raw(points, mask, poses, step=1, max_edge=None, normals=None, valid=None, cos_view=None, colors=None, flags=0):
    """One call of g2v_cloud_normals into the caller's tensors (no allocation, no host synchronisation): normals fp32 [N,H,W,3],
    valid uint8 [N,H,W], cos_view fp32 [N,H,W], colors fp32 [N,3,H,W] where given - at least one.  flags: NORMALS_PLAIN /
    NORMALS_HALO force a form of the kernel."""
    N, H, W = _nhw3(points, "points")
    mask = _mask_u8(mask, (N, H, W), optional=True)
    if poses is not None:
        assert poses.is_cuda and poses.dtype == torch.float32 and tuple(poses.shape) == (N, 4, 4) and poses.is_contiguous(), \
            "poses: fp32 [N,4,4], contiguous"
    assert normals is None or _nhw3(normals, "normals") == (N, H, W), "normals: the shape of points"
    for t, dtype, what in ((valid, torch.uint8, "valid"), (cos_view, torch.float32, "cos_view")):
        assert t is None or (t.is_cuda and t.dtype == dtype and tuple(t.shape) == (N, H, W) and t.is_contiguous()), f"{what}: {dtype} [N,H,W]"
    if colors is not None:
        _colors_n3hw(colors, N, H, W)
    flags = int(flags) | (NORMALS_MAX_EDGE if max_edge is not None else 0)
    _ck(lib().g2v_cloud_normals(_p(points), _p(mask), _p(poses), N, H, W, int(step), flags, float(max_edge or 0.0), _p(normals), _p(valid),
                                _p(cos_view), _p(colors), _stream()), "g2v_cloud_normals")


def cloud_normals(points, mask, poses, step=1, max_edge=None, colors=False):
    """Image-space surface normals of recon's pointmaps (g2v_cloud_normals; include/g2vlm_hip.h has the exact rule): points fp32
    [N,H,W,3], mask uint8 or bool [N,H,W] or None (all pixels), poses fp32 [N,4,4] camera-to-world or None (the camera at the origin:
    camera-frame normals of local points), step = the distance to the four neighbours (1..8), max_edge = the longest edge to a
    neighbour that counts (None: no limit).  Returns dict(normals fp32 [N,H,W,3] = unit vectors that look at the camera, valid uint8
    [N,H,W], cos_view fp32 [N,H,W] = |cos| of the angle between the normal and the viewing ray, colors fp32 [N,3,H,W] = n / 2 + 1 / 2
    or None); everything is 0 where valid is.  Bit-reproducible; no host synchronisation."""
    N, H, W = _nhw3(points, "points")
    dev = points.device
    out = dict(normals=torch.empty((N, H, W, 3), dtype=torch.float32, device=dev), valid=torch.empty((N, H, W), dtype=torch.uint8, device=dev),
               cos_view=torch.empty((N, H, W), dtype=torch.float32, device=dev),
               colors=torch.empty((N, 3, H, W), dtype=torch.float32, device=dev) if colors else None)
    cloud_normals_raw(points, mask, poses, step, max_edge, **out)
    return out


def cloud_compact_normals_workspace(N, H, W):
    return int(lib().g2v_cloud_compact_normals_workspace(int(N), int(H), int(W)))


def cloud_compact_normals(points, normals, colors, mask, workspace=None):
    """The pixels mask keeps as packed 27-byte PLY records with normals (g2v_cloud_compact_normals): points, normals fp32 [N,H,W,3],
    colors fp32 [N,3,H,W] in [0,1], mask uint8 or bool [N,H,W] -> (records uint8 [M,27] = <f4 x,y,z + <f4 nx,ny,nz + u1 r,g,b in
    view-major, row-major order, counts int32 [N]).  Two calls: the first only counts, the records are then allocated at their exact
    size and the second call fills them.  Synchronous: the counts are read back once."""
    N, H, W = _nhw3(points, "points")
    assert _nhw3(normals, "normals") == (N, H, W), "normals: the shape of points"
    _colors_n3hw(colors, N, H, W)
    mask = _mask_u8(mask, (N, H, W))
    workspace, ws_bytes = _workspace_arg(workspace, cloud_compact_normals_workspace(N, H, W), points.device, "compact_normals")
    counts = torch.empty(N, dtype=torch.int32, device=points.device)

    def call(records, cap):
        _ck(lib().g2v_cloud_compact_normals(_p(points), _p(normals), _p(colors), _p(mask), N, H, W, _p(records) if cap else None, cap,
                                            _p(counts), _p(workspace), ws_bytes, _stream()), "g2v_cloud_compact_normals")
    call(None, 0)
    m = int(counts.sum(dtype=torch.int64).item())
    records = torch.empty((m, 27), dtype=torch.uint8, device=points.device)
    if m:
        call(records, m)
    return records, counts


# ------------------------------------------------------------------------------------------ nearest neighbour (csrc/nn.hip)
NN_BRUTE, NN_GRID = 1, 2                                   # G2V_NN_BRUTE, G2V_NN_GRID (A/B and tests only)


def cloud_nn_workspace(Nq, Nt):
    return int(lib().g2v_cloud_nn_workspace(int(Nq), int(Nt)))


def cloud_nn_raw(query, query_mask, target, target_mask, max_distance, flags, index, sq_distance, stats, workspace=None):
    """One call of g2v_cloud_nn into the caller's tensors (no allocation but a grown workspace, no host synchronisation)."""
    for t, what in ((query, "query"), (target, "target")):
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 3 and t.is_contiguous(), f"{what}: fp32 [N,3], contiguous"
    Nq, Nt = query.shape[0], target.shape[0]
    masks = [_mask_u8(query_mask, (Nq,), "query_mask", optional=True), _mask_u8(target_mask, (Nt,), "target_mask", optional=True)]
    assert index.is_cuda and index.dtype == torch.int32 and tuple(index.shape) == (Nq,) and index.is_contiguous(), "index: int32 [Nq]"
    assert sq_distance.is_cuda and sq_distance.dtype == torch.float32 and tuple(sq_distance.shape) == (Nq,) and sq_distance.is_contiguous(), \
        "sq_distance: fp32 [Nq]"
    assert stats.is_cuda and stats.dtype == torch.int32 and tuple(stats.shape) == (4,), "stats: int32 [4]"
    workspace, ws_bytes = _workspace_arg(workspace, cloud_nn_workspace(Nq, Nt), query.device, "nn")
    _ck(lib().g2v_cloud_nn(_p(query) if Nq else None, _p(masks[0]) if Nq else None, Nq, _p(target) if Nt else None,
                           _p(masks[1]) if Nt else None, Nt, float("inf") if max_distance is None else float(max_distance), int(flags),
                           _p(index) if Nq else None, _p(sq_distance) if Nq else None, _p(stats), _p(workspace),
                           ws_bytes, _stream()), "g2v_cloud_nn")


def cloud_nn(query, target, max_distance=None, query_mask=None, target_mask=None, flags=0, workspace=None):
    """For every query point the nearest target point (g2v_cloud_nn; include/g2vlm_hip.h has the exact rule): query fp32 [Nq,3],
    target fp32 [Nt,3], masks uint8 or bool [Nq] / [Nt] or None (all points), max_distance = the largest distance that counts (None:
    no limit).  Returns (index int32 [Nq] = the target or -1, sq_distance fp32 [Nq] = the fp32 squared distance or +inf, stats int32
    [4] = participating queries, participating targets, queries without / with a neighbour), on the device.  Exact: the nearest by
    the fp32 rule, ties to the lowest index; bit-reproducible; no host synchronisation.  flags: NN_BRUTE / NN_GRID force a path."""
    dev = query.device
    index = torch.empty(query.shape[0], dtype=torch.int32, device=dev)
    sq_distance = torch.empty(query.shape[0], dtype=torch.float32, device=dev)
    stats = torch.empty(4, dtype=torch.int32, device=dev)
    cloud_nn_raw(query, query_mask, target, target_mask, max_distance, flags, index, sq_distance, stats, workspace=workspace)
    return index, sq_distance, stats


# ------------------------------------------------------------------------------------------ voxel downsampling (csrc/voxel.hip)
VOXEL_NO_RUNS = 1                                          # G2V_VOXEL_NO_RUNS (A/B only)


def _voxel_inputs(points, mask):
    N, H, W = _nhw3(points, "points")
    return N, H, W, _mask_u8(mask, (N, H, W))


def voxel_bounds(points, mask):
    """(min fp64 [3], max fp64 [3], count) of the points that take part (mask != 0, finite), as python floats (g2v_voxel_bounds).
    Synchronous: one readback of seven words.  count == 0: zeros."""
    N, H, W, mask = _voxel_inputs(points, mask)
    out = torch.empty(7, dtype=torch.float32, device=points.device)
    _ck(lib().g2v_voxel_bounds(_p(points), _p(mask), N, H, W, _p(out), _stream()), "g2v_voxel_bounds")
    host = out.cpu()
    lo_hi = host[:6].double().tolist()
    return lo_hi[:3], lo_hi[3:], int(host[6:].view(torch.int32).item())


def voxel_assign_workspace(N, H, W):
    return int(lib().g2v_voxel_assign_workspace(int(N), int(H), int(W)))


def voxel_reduce_workspace(M):
    return int(lib().g2v_voxel_reduce_workspace(int(M)))


def voxel_assign(points, mask, voxel_size, origin, workspace=None):
    """The dense id of every pixel's grid cell (g2v_voxel_assign): points fp32 [N,H,W,3], mask uint8 or bool [N,H,W], voxel_size
    > 0 and origin (3 floats), both taken as fp64 -> (voxel_of int32 [N,H,W], -1 where the pixel is dropped; stats = [cells M,
    participating pixels, out-of-range pixels, status]).  Cells are numbered by first appearance in flat pixel order.
    Synchronous: the four stats are read back once."""
    N, H, W, mask = _voxel_inputs(points, mask)
    ox, oy, oz = (float(o) for o in origin)
    workspace, ws_bytes = _workspace_arg(workspace, voxel_assign_workspace(N, H, W), points.device, "voxel_assign")
    voxel_of = torch.empty((N, H, W), dtype=torch.int32, device=points.device)
    stats = torch.empty(4, dtype=torch.int32, device=points.device)
    _ck(lib().g2v_voxel_assign(_p(points), _p(mask), N, H, W, float(voxel_size), ox, oy, oz, _p(voxel_of), _p(stats), _p(workspace),
                               ws_bytes, _stream()), "g2v_voxel_assign")
    return voxel_of, stats.tolist()


def voxel_reduce(points, colors, voxel_of, M, voxel_size, origin, workspace=None, flags=0):
    """The cells' vertices (g2v_voxel_reduce): voxel_of and M = stats[0] from voxel_assign with the same points, voxel_size and
    origin; colors fp32 [N,3,H,W] -> (records uint8 [M,15] = <f4 x,y,z + u1 r,g,b, counts int32 [M], points fp32 [M,3], colors
    uint8 [M,3])."""
    N, H, W = _nhw3(points, "points")
    _colors_n3hw(colors, N, H, W)
    assert voxel_of.is_cuda and voxel_of.dtype == torch.int32 and tuple(voxel_of.shape) == (N, H, W) and voxel_of.is_contiguous(), \
        "voxel_of: int32 [N,H,W]"
    M = int(M)
    ox, oy, oz = (float(o) for o in origin)
    dev = points.device
    records = torch.empty((M, 15), dtype=torch.uint8, device=dev)
    counts = torch.empty(M, dtype=torch.int32, device=dev)
    out_points = torch.empty((M, 3), dtype=torch.float32, device=dev)
    out_colors = torch.empty((M, 3), dtype=torch.uint8, device=dev)
    workspace, ws_bytes = _workspace_arg(workspace, voxel_reduce_workspace(M), dev, "voxel_reduce")
    _ck(lib().g2v_voxel_reduce(_p(points), _p(colors), _p(voxel_of), N, H, W, float(voxel_size), ox, oy, oz, M, _p(records), _p(counts),
                               _p(out_points), _p(out_colors), _p(workspace), ws_bytes, int(flags),
                               _stream()), "g2v_voxel_reduce")
    return records, counts, out_points, out_colors


def mrope_table_into(pos_i32, inv_freq, cos, sin):
    _ck(lib().g2v_mrope_table(_p(pos_i32), pos_i32.shape[1], _p(inv_freq), _p(cos), _p(sin), _stream()), "g2v_mrope_table")


def swiglu_bf16(gu, out):
    """out[i] = bf16(bf16(silu(g[i])) * u[i]); gu holds gate/up interleaved per 16 (decode MLP)."""
    _ck(lib().g2v_swiglu_bf16(_p(gu), _p(out), out.numel(), _stream()), "g2v_swiglu_bf16")
    return out
