"""CPU (no GPU): the FP8 (e4m3) weight-only decode - the host quantiser (g2vlm_amd/quant.py), the C ABI of the two entry
points of csrc/decode_fp8.hip (every case here is refused by the argument checks, which return before any HIP call), the
build audit of that file, and the element-wise checker (tests/gemm_check.py) on an fp32 emulation of the kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_check as G  # noqa: E402

from g2vlm_amd.quant import dequantize_rows, quantize_rows_e4m3  # noqa: E402
from g2vlm_amd.weights import interleave_gate_up  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(); g.manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------ 1. quantiser
def quantiser_rows():
    """bf16 [N, 512]: Gaussian rows, rows scaled by 2^+-20, a zero row, a row with one huge outlier, peaked_lm_head rows."""
    from oracle import synth
    K = 512
    gauss = rnd(64, K, seed=1, scale=K ** -0.5)
    big, small = rnd(8, K, seed=2) * 2.0 ** 20, rnd(8, K, seed=3) * 2.0 ** -20
    zero = torch.zeros(1, K)
    outlier = rnd(1, K, seed=4, scale=0.02)
    outlier[0, 77] = 3000.0
    exact = torch.full((1, K), 0.01)
    exact[0, 5] = -448.0 * 2.0 ** -3                          # amax / 448 an exact power of two
    sd = synth.peaked_lm_head({"language_model.lm_head.weight": rnd(96, K, seed=5, scale=K ** -0.5)}, 2.0, 11)
    return torch.cat([gauss, big, small, zero, outlier, exact, sd["language_model.lm_head.weight"]]).bfloat16()


def test_quantiser_properties():
    w = quantiser_rows()
    q, s = quantize_rows_e4m3(w)
    assert q.dtype == torch.uint8 and q.shape == w.shape and s.dtype == torch.float32 and s.shape == (w.shape[0],)
    mant, _ = torch.frexp(s)
    assert bool((mant == 0.5).all()), "scales are powers of two"
    assert not bool(((q == 0x7F) | (q == 0xFF)).any()), "a NaN code"
    qa = q.view(torch.float8_e4m3fn).float().abs().amax(1)
    nz = w.float().abs().amax(1) > 0
    assert bool(nz.sum() == w.shape[0] - 1)
    assert bool(((qa[nz] >= 224) & (qa[nz] <= 448)).all()), qa[nz].min()
    assert bool((s[~nz] == 1).all()) and bool((q[~nz] == 0).all())
    # exact in bf16: the fp64 product q * scale equals its bf16 rounding
    dq = dequantize_rows(q, s)
    assert dq.dtype == torch.bfloat16
    exact = q.view(torch.float8_e4m3fn).double() * s.double()[:, None]
    assert torch.equal(dq.double(), exact)
    # the derived bound: half an ulp of a 3-bit mantissa, half the subnormal step 2^-9
    err = (dq.double() - w.double()).abs()
    bound = torch.maximum(2.0 ** -4 * w.double().abs(), 2.0 ** -10 * s.double()[:, None])
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    # representable input is lossless, even where the scale moves a binade
    q2, s2 = quantize_rows_e4m3(dq)
    assert torch.equal(dequantize_rows(q2, s2).view(torch.int16), dq.view(torch.int16))


def test_quantiser_commutes_with_gate_up_interleave_and_qkv_concat():
    g, u = rnd(64, 256, seed=7).bfloat16(), (rnd(64, 256, seed=8) * 2.0 ** 6).bfloat16()
    dq = lambda w: dequantize_rows(*quantize_rows_e4m3(w))    # noqa: E731
    assert torch.equal(dq(interleave_gate_up(g, u)), interleave_gate_up(dq(g), dq(u)))
    assert torch.equal(dq(torch.cat([g, u], 0)), torch.cat([dq(g), dq(u)], 0))


# ------------------------------------------------------------------------------------------------ 2. the C ABI
PG = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
PGB = PG[:8] + [C.c_int] + PG[8:]
NAMES = ("x", "norm_w", "eps", "Wq", "wscale", "bias", "out", "res", "B", "N", "K", "act", "stream")


@pytest.fixture(scope="module")
def lib():
    from g2vlm_amd import build
    lib = C.CDLL(build.build())
    lib.g2v_gemv_pg_fp8.argtypes, lib.g2v_gemv_pg_fp8.restype = PG, C.c_int
    lib.g2v_gemv_pg_batch_fp8.argtypes, lib.g2v_gemv_pg_batch_fp8.restype = PGB, C.c_int
    return lib


def call(lib, batched, **kw):
    """A valid argument set (the pointers are never dereferenced: every call below is refused first), with overrides."""
    a = dict(x=16, norm_w=None, eps=1e-6, Wq=16, wscale=16, bias=None, out=16, res=None, B=2, N=2048, K=1536, act=0, stream=None)
    a.update(kw)
    if batched:
        return lib.g2v_gemv_pg_batch_fp8(*[a[n] for n in NAMES])
    return lib.g2v_gemv_pg_fp8(*[a[n] for n in NAMES if n != "B"])


def test_library_exports_and_declares_the_fp8_symbols(lib):
    from g2vlm_amd import hip
    hdr = open(os.path.join(ROOT, "include", "g2vlm_hip.h")).read()
    for name in ("g2v_gemv_pg_fp8", "g2v_gemv_pg_batch_fp8"):
        assert hasattr(lib, name) and name in hip.EXPORTS
        assert re.search(r"\bint " + name + r"\(", hdr), name
    assert callable(hip.gemv_pg_fp8) and callable(hip.gemv_pg_batch_fp8)
    from g2vlm_amd import build
    assert "decode_fp8.hip" in build.SOURCES and "decode_fp8.hip" in build.RESOURCE_AUDIT


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("bad", [dict(Wq=None), dict(wscale=None), dict(x=None), dict(out=None, res=None), dict(K=1528), dict(K=1544),
                                 dict(K=0), dict(N=0), dict(K=1 << 20),
                                 dict(act=1, norm_w=16, N=2040), dict(act=1, norm_w=None, N=2048), dict(act=1, norm_w=16, res=16),
                                 dict(act=1, norm_w=16, out=None, res=16), dict(norm_w=16, K=1552), dict(norm_w=16, K=8960)])
def test_argument_errors_return_einval_without_a_device(lib, batched, bad):
    assert call(lib, batched, **bad) == -22


def test_k_limits_are_those_of_the_bf16_entry_points(lib):
    assert call(lib, False, K=9216 + 16) == -22 and call(lib, True, K=12288 + 16) == -22
    for b in (0, 9, -1, 64):
        assert call(lib, True, B=b) == -22


# ------------------------------------------------------------------------------------------------ 3. build audit
def _remarks(src):
    from g2vlm_amd import build
    build.build()
    rows, cur = [], None
    for ln in open(build.resources_path(src)).read().splitlines():
        m = re.search(r"remark:\s+(?:\S+:\d+:\d+:\s+)?(.*?)\s+\[-Rpass", ln)
        if not m:
            continue
        t = m.group(1)
        if t.startswith("Function Name:"):
            cur = {"name": t.split(":", 1)[1].strip()}
            rows.append(cur)
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    return rows


@pytest.mark.timeout(1800)
def test_every_fp8_gemv_instantiation_is_spill_free():
    if not os.path.exists(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    rows = _remarks("decode_fp8.hip")
    for pat, least in (("gemv_pg8_kernel", 12), ("gemv_pgb8_kernel", 18), ("gemv_pgk8_kernel", 3)):
        mine = [r for r in rows if pat in r["name"]]
        assert len(mine) >= least, (pat, len(mine))
        for r in mine:
            assert int(r["ScratchSize [bytes/lane]"]) == 0, r
            assert int(r["VGPRs"]) <= 256, r


@pytest.fixture(scope="module")
def fp8_asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    from g2vlm_amd import build
    out = tmp_path_factory.mktemp("asm8") / "decode_fp8.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-kernarg-preload-count=16",
           *build.FILE_FLAGS.get("decode_fp8.hip", []), "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC, "-S", "--cuda-device-only",
           os.path.join(build.CSRC, "decode_fp8.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out.read_text()


@pytest.mark.timeout(600)
def test_device_assembly_converts_in_the_valu_and_streams_16_byte_nontemporal_words(fp8_asm):
    s = fp8_asm
    names = re.findall(r"^(_Z\S*gemv_pg(?:b|k)?8_kernel\S*):", s, re.M)
    assert len(names) >= 33, len(names)
    for name in names:
        i = s.index("\n", s.index(name + ":"))
        body = s[i:s.index(".Lfunc_end", i)]
        assert "scratch_" not in body, (name, "the kernel spills")
        assert "v_cvt_scalef32_pk_bf16_fp8" in body or "v_cvt_pk_f32_fp8" in body, name
        assert "v_dot2c_f32_bf16" in body or "v_dot2_f32_bf16" in body, name
        # no byte / short loads anywhere except the 2-byte bias word; the weight stream is global_load_dwordx4 ... nt
        assert not re.search(r"global_load_(u|s)byte", body), name
        nt = [ln for ln in body.split("\n") if "global_load_dwordx4" in ln and re.search(r"\bnt\b", ln)]
        assert nt, name
        assert not [ln for ln in body.split("\n") if re.search(r"global_load_dword(x2|x3)?\s", ln) and re.search(r"\bnt\b", ln)], name


# ------------------------------------------------------------------------------------------------ 4. the checker
def lane_chunk_emulation(X, Wd):
    """fp32 emulation of the kernels' summation: a lane owns 16 consecutive k (chunks lane, lane + 64, ...), accumulates
    them in order, and the 64 lane sums are added pairwise.  X bf16 [B, K], Wd bf16 [N, K] (dequantised) -> fp32 [B, N]."""
    B, K = X.shape
    N = Wd.shape[0]
    nch = K // 16
    kch = (nch + 63) // 64
    x = torch.zeros(B, kch * 1024); x[:, :K] = X.float()
    w = torch.zeros(N, kch * 1024); w[:, :K] = Wd.float()
    x = x.view(B, kch, 64, 16).permute(2, 0, 1, 3).reshape(64, B, kch * 16)
    w = w.view(N, kch, 64, 16).permute(2, 0, 1, 3).reshape(64, N, kch * 16)
    lanes = torch.bmm(x, w.transpose(1, 2))                   # [64, B, N] fp32 lane sums
    while lanes.shape[0] > 1:
        lanes = lanes[0::2] + lanes[1::2]
    return lanes[0]


def fp8_operands(B, N, K, seed):
    X = rnd(B, K, seed=seed).bfloat16()
    q, s = quantize_rows_e4m3(rnd(N, K, seed=seed + 1, scale=K ** -0.5).bfloat16())
    return X, q, s


@pytest.mark.parametrize("B,N,K", [(1, 2048, 1536), (8, 1536, 8960), (3, 1000, 2064)])
def test_checker_accepts_the_honest_emulation(B, N, K):
    X, q, s = fp8_operands(B, N, K, seed=30)
    Wd = dequantize_rows(q, s)
    got = lane_chunk_emulation(X, Wd).bfloat16()
    chk = G.check_gemm(got, X, Wd, None, G.EPI_BF16)
    assert chk.count == 0, chk.report(what=f"honest {B}x{N}x{K}")
    assert 0.2 < chk.multi / chk.n < 0.7                      # many elements have two admissible values: see the GPU test


def test_checker_accepts_the_honest_swiglu_emulation():
    B, N, K = 8, 17920, 1536
    X, q, s = fp8_operands(B, N, K, seed=40)
    Wd = dequantize_rows(q, s)
    acc = lane_chunk_emulation(X, Wd).view(B, N // 32, 2, 16)
    g, u = acc[:, :, 0].reshape(B, N // 2).bfloat16().float(), acc[:, :, 1].reshape(B, N // 2).bfloat16().float()
    got = (torch.nn.functional.silu(g).bfloat16().float() * u).bfloat16()
    chk = G.check_gemm(got, X, Wd, None, G.EPI_SWIGLU)
    assert chk.count == 0 and chk.max_ulps <= G.ULP_BOUND[G.EPI_SWIGLU], (chk.report(what="swiglu"), chk.max_ulps)


def planted(B, N=1000, K=2064, seed=50, scale_row=17, swap_row=401):
    X, q, s = fp8_operands(B, N, K, seed)
    Wd = dequantize_rows(q, s)
    s_bad = s.clone(); s_bad[scale_row] *= 2
    q_bad = q.clone()
    # two neighbouring weight bytes of one row change places (distinct values, neither tiny)
    row = q_bad[swap_row].view(torch.float8_e4m3fn).float().abs()
    k = int(((row[:-1] - row[1:]).abs() * (row[:-1] > 64) * (row[1:] < 32)).argmax())
    q_bad[swap_row, k], q_bad[swap_row, k + 1] = q[swap_row, k + 1], q[swap_row, k]
    assert q_bad[swap_row, k] != q[swap_row, k]
    got = lane_chunk_emulation(X, dequantize_rows(q_bad, s_bad)).bfloat16()
    return G.check_gemm(got, X, Wd, None, G.EPI_BF16)


@pytest.mark.parametrize("B", [3, 8])
def test_checker_flags_a_wrong_scale_and_two_swapped_bytes_in_exactly_those_columns(B):
    chk = planted(B)
    cols = sorted(set(chk.bad.any(0).nonzero().flatten().tolist()))
    assert cols == [17, 401], cols
    assert int(chk.bad[:, 17].sum()) == B                     # a scale off by two moves every scene's output


def test_one_activation_vector_can_miss_a_byte_swap_so_batch_1_is_checked_over_eight():
    """A swapped byte pair moves one output by (w_a - w_b)(x_b - x_a): with a single activation vector the two activations
    may be close and the column stays inside its admissible set, so one vector proves nothing about byte order.  Over 8
    different vectors the column is caught.  The GPU tests therefore always drive the batch-1 kernel with 8 different
    activation vectors.  A scale off by two is caught for every vector."""
    chk = planted(8)
    assert int(chk.bad[:, 17].sum()) == 8
    assert 1 <= int(chk.bad[:, 401].sum()) <= 8
