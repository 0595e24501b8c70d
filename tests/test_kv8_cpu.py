"""CPU (no GPU): the FP8 (e4m3) KV cache of the decode step (Engine.decode_kv = "fp8", csrc/decode_kv8.hip).

1. The encoding: g2vlm_amd/quant.py applied to cache rows viewed as [rows * Hkv, 128] - what g2v_kv_quant_e4m3 must reproduce.
2. The C ABI: the three symbols are exported and declared, argument errors come back as -22 before anything touches a device,
   the decode_kv setter refuses what it must.
3. The step program in FP8-KV mode, traced as tests/test_decode_program_cpu.py traces the other modes.
4. The build remarks of decode_kv8.hip: no scratch, at most 256 VGPRs.
5. The accuracy bound tests/test_kv8_gpu.py uses: fp64 attention over dequant(quant(K, V)) against fp64 attention over K, V.
"""
import ctypes as C
import os
import re
import shutil
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import dims as D  # noqa: E402

from g2vlm_amd import hip  # noqa: E402
from g2vlm_amd.engine import Engine  # noqa: E402
from g2vlm_amd.quant import dequantize_rows, quantize_rows_e4m3  # noqa: E402
from test_decode_program_cpu import LAYERS, Recorder, TinyWeights, filled_cache  # noqa: E402

KV8_CALLS = ("kv_quant_e4m3", "kv_dequant_e4m3", "decode_attn_pg_kv8")


# ------------------------------------------------------------------------------------------------ 1. the encoding
def magnitude_rows(Hkv, seed=0):
    """Cache rows [rows, Hkv, 128] bf16 whose (row, head) amax runs from 2^-20 to 3e4, plus the edge rows: all zero, amax = 448 x
    2^k (amax / scale exactly 448: the largest code), amax = 224 x 2^k (mantissa 1.75, the last amax that keeps the smaller
    exponent) and the next bf16 above it, 225 x 2^k (the first amax that takes the larger one)."""
    g = torch.Generator(); g.manual_seed(seed)
    mags = [2.0 ** -20, 2.0 ** -13, 3e-3, 0.07, 1.0, 5.5, 448.0, 1000.0, 30080.0]   # 30080: the first bf16 above 3e4
    rows = [torch.randn((Hkv, 128), generator=g) * m / 4 for m in mags]
    for r, m in zip(rows, mags):
        r[:, 5] = m                                        # pin the amax of every head
        r.clamp_(-m, m)
    rows.append(torch.zeros(Hkv, 128))
    for top in (448.0, 224.0, 225.0):
        for k in (-9, 0, 3):
            r = torch.randn((Hkv, 128), generator=g).clamp_(-1, 1) * top * 2.0 ** k * 0.5
            r[:, 77] = -top * 2.0 ** k
            rows.append(r)
    return torch.stack(rows).to(torch.bfloat16)


@pytest.mark.parametrize("Hkv", [2, 1])
def test_the_row_quantiser_on_cache_rows(Hkv):
    x = magnitude_rows(Hkv)
    flat = x.view(-1, 128)
    q, s = quantize_rows_e4m3(flat)
    assert q.shape == flat.shape and s.shape == (flat.shape[0],) and q.dtype == torch.uint8 and s.dtype == torch.float32
    assert not ((q & 0x7F) == 0x7F).any()                       # no NaN code
    amax = flat.float().abs().amax(dim=1)
    assert float(amax.min()) == 0.0 and float(amax[amax > 0].min()) <= 2.0 ** -20 and float(amax.max()) >= 3e4
    zero = amax == 0
    assert zero.any() and (s[zero] == 1).all() and (q[zero] == 0).all()
    m, e = torch.frexp(s)
    assert (m == 0.5).all()                                  # powers of two
    ratio = amax[~zero] / s[~zero]
    assert (ratio > 224).all() and (ratio <= 448).all()
    # the edge rows: 448 x 2^k and 224 x 2^k both land on the largest code (the ceiling keeps the smaller exponent up to and
    # including mantissa 1.75), 225 x 2^k is the first amax on the larger scale
    n = flat.shape[0] // Hkv
    edge = ratio.view(-1, Hkv)[-9:]
    assert (edge[:6] == 448).all() and (edge[6:] == 225).all(), edge
    assert n == 19
    # value-level round trip: dequant(quant(dequant(quant(x)))) == dequant(quant(x)), and dequantised values are bf16
    dq = dequantize_rows(q, s)
    q2, s2 = quantize_rows_e4m3(dq)
    assert torch.equal(dequantize_rows(q2, s2), dq)
    assert torch.equal((q.view(torch.float8_e4m3fn).float() * s[:, None]).to(torch.bfloat16).float(), q.view(torch.float8_e4m3fn).float() * s[:, None])
    # the scale from the float's bits, as the kernel computes it: amax = m 2^E, exponent E - 8 if m <= 1.75 else E - 7
    bits = amax[~zero].view(torch.int32)
    E, mant = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    e_s = torch.clamp(E - torch.where(mant <= 0x600000, 8, 7), min=1)
    assert torch.equal((e_s << 23).to(torch.int32).view(torch.float32), s[~zero])


# ------------------------------------------------------------------------------------------------ 2. the C ABI and the setter
P, I, L, F = C.c_void_p, C.c_int, C.c_int64, C.c_float
ATTN_NAMES = ("qkv", "qw", "kw", "eps", "und", "cos", "sin", "kc", "vc", "ks", "vs", "out", "len", "batch", "scene_rows", "max_len", "Hq", "Hkv",
              "scale", "ws", "stream")


@pytest.fixture(scope="module")
def lib():
    from g2vlm_amd import build
    lib = C.CDLL(build.build())
    lib.g2v_kv_quant_e4m3.argtypes, lib.g2v_kv_quant_e4m3.restype = [P, L, I, P, P, P], I
    lib.g2v_kv_dequant_e4m3.argtypes, lib.g2v_kv_dequant_e4m3.restype = [P, P, L, I, P, P], I
    lib.g2v_decode_attn_pg_kv8.argtypes = [P, P, P, F, I, P, P, P, P, P, P, P, P, I, L, I, I, I, F, P, P]
    lib.g2v_decode_attn_pg_kv8.restype = I
    return lib


def test_library_exports_and_declares_the_kv8_symbols(lib):
    from g2vlm_amd import build
    hdr = open(os.path.join(ROOT, "include", "g2vlm_hip.h")).read()
    for name in ("g2v_kv_quant_e4m3", "g2v_kv_dequant_e4m3", "g2v_decode_attn_pg_kv8"):
        assert hasattr(lib, name) and name in hip.EXPORTS
        assert re.search(r"\bint " + name + r"\(", hdr), name
    assert all(callable(getattr(hip, n)) for n in KV8_CALLS)
    assert "decode_kv8.hip" in build.SOURCES and "decode_kv8.hip" in build.RESOURCE_AUDIT
    assert len(hip._SIGS["g2v_decode_attn_pg_kv8"][0]) == len(hip._SIGS["g2v_decode_attn_pg"][0]) + 2


def attn_call(lib, **kw):
    """A valid argument set (no pointer is dereferenced: every call below is refused before any launch), with overrides."""
    a = dict(qkv=16, qw=16, kw=16, eps=1e-6, und=1, cos=16, sin=16, kc=16, vc=16, ks=16, vs=16, out=16, len=16, batch=2, scene_rows=4096,
             max_len=4096, Hq=12, Hkv=2, scale=0.088, ws=16, stream=None)
    a.update(kw)
    return lib.g2v_decode_attn_pg_kv8(*[a[n] for n in ATTN_NAMES])


@pytest.mark.parametrize("bad", [dict(ks=None), dict(vs=None), dict(kc=None), dict(vc=None), dict(qkv=None), dict(out=None), dict(ws=None),
                                 dict(len=None), dict(batch=0), dict(batch=65536), dict(max_len=0), dict(scene_rows=4095), dict(Hq=13),
                                 dict(Hq=18), dict(Hkv=0), dict(Hkv=129, Hq=129)])
def test_attention_argument_errors_return_einval_without_a_device(lib, bad):
    assert attn_call(lib, **bad) == -22


def test_quantiser_argument_errors_return_einval_without_a_device(lib):
    for rows, hkv in ((0, 2), (-1, 2), (5, 0), (5, 129)):
        assert lib.g2v_kv_quant_e4m3(16, rows, hkv, 16, 16, None) == -22
        assert lib.g2v_kv_dequant_e4m3(16, 16, rows, hkv, 16, None) == -22
    for args in ((None, 5, 2, 16, 16, None), (16, 5, 2, None, 16, None), (16, 5, 2, 16, None, None)):
        assert lib.g2v_kv_quant_e4m3(*args) == -22
    for args in ((None, 16, 5, 2, 16, None), (16, None, 5, 2, 16, None), (16, 16, 5, 2, None, None)):
        assert lib.g2v_kv_dequant_e4m3(*args) == -22


def test_decode_kv_setter():
    eng = Engine(TinyWeights(D.TINY["llm"]), D.TINY)
    assert eng.decode_kv == "bf16"
    with pytest.raises(ValueError):
        eng.decode_kv = "int8"
    eng.decode_gen = 1
    with pytest.raises(ValueError):                          # either order of setting
        eng.decode_kv = "fp8"
    assert eng.decode_kv == "bf16"
    eng.decode_gen = 2
    eng._decode_cached["x"] = 1
    eng.decode_kv = "fp8"
    assert eng.decode_kv == "fp8" and not eng._decode_cached   # a captured step belongs to the mode it was captured with
    with pytest.raises(ValueError):
        eng.decode_gen = 1
    assert eng.decode_gen == 2
    eng._decode_cached["x"] = 1
    eng.decode_kv = "fp8"
    assert eng._decode_cached                                  # unchanged mode: nothing dropped
    eng.decode_kv = "bf16"
    assert not eng._decode_cached
    eng.decode_gen = 1


def test_the_mode_is_plumbed_like_decode_weights():
    import inspect
    from g2vlm_amd import g2vlm_utils
    from g2vlm_amd.modeling.g2vlm.g2vlm import G2VLM
    assert isinstance(G2VLM.decode_kv, property)
    assert inspect.signature(g2vlm_utils.build_model).parameters["decode_kv"].default == "bf16"
    assert "decode_kv" in inspect.signature(g2vlm_utils.load_model_and_tokenizer).parameters
    assert "--decode-kv" in open(os.path.join(ROOT, "inference_chat.py")).read()


# ------------------------------------------------------------------------------------------------ 3. the step program
@pytest.fixture(scope="module")
def kv8_traces():
    """{(mode, B, weights): (calls of begin / set_slot, calls of one eager step, calls of decode_end or None, state)}"""
    mp = pytest.MonkeyPatch()
    try:
        w = TinyWeights(D.TINY["llm"])
        rec = Recorder(mp, w)
        for name in KV8_CALLS:
            mp.setattr(hip, name, rec._wrap(name, getattr(hip, name)))
        eng = Engine(w, D.TINY)
        Lc = D.TINY["llm"]
        out = {}
        for enc in ("bf16", "fp8"):
            eng.decode_weights = enc
            eng.decode_kv = "fp8"
            user = filled_cache(Lc, 5, 1)
            st = eng.decode_begin(user, 3, 5, 4, use_graph=False)
            begin = rec.take()
            eng.decode_step(st)
            step = rec.take()
            eng.decode_end(st)
            out[("b1", 1, enc)] = (begin, step, rec.take(), st, user)
            for B in (2, 9):
                st = eng.decode_begin_batch([filled_cache(Lc, 4 + j, j) for j in range(B)], [3] * B, [5] * B, 4, use_graph=False)
                begin = rec.take()
                eng.decode_step_batch(st)
                out[("batch", B, enc)] = (begin, rec.take(), None, st, None)
            st = eng.decode_begin_shared(filled_cache(Lc, 6, 99), [filled_cache(Lc, 2 + j % 3, j) for j in range(2)], [3] * 2, [9] * 2, 4,
                                         use_graph=False)
            begin = rec.take()
            eng.decode_step_batch(st)
            out[("shared", 2, enc)] = (begin, rec.take(), None, st, None)
        yield out
    finally:
        mp.undo()


def _names(calls):
    return [c[0] for c in calls]


def test_the_fp8_kv_step_at_batch_1_reads(kv8_traces):
    begin, step, end, st, user = kv8_traces[("b1", 1, "bf16")]
    assert _names(step) == ["gather_rows", "mrope_table_into",
                            "gemv_pg", "decode_attn_pg_kv8", "gemv_pg", "gemv_pg", "gemv_pg",
                            "gemv_pg", "decode_attn_pg_kv8", "gemv_pg", "gemv_pg", "gemv_pg",
                            "gemv_pg", "argmax_bf16", "decode_advance"]
    assert _names(kv8_traces[("b1", 1, "fp8")][1]) == [n + "_fp8" if n == "gemv_pg" else n for n in _names(step)]
    # the caller's 5 rows are quantised into the engine's block, K and V of every layer; the appended row comes back dequantised
    assert _names(begin) == ["kv_quant_e4m3"] * (2 * LAYERS)
    for c in begin:
        assert c[1]["src"][2:] == ((5, 1, 128), "torch.bfloat16") and c[1]["codes"][2:] == ((5, 1, 128), "torch.uint8")
        assert c[1]["scales"][2:] == ((5, 1), "torch.float32")
    assert _names(end) == ["kv_dequant_e4m3"] * (2 * LAYERS)
    for c in end:
        assert c[1]["codes"][2:] == ((1, 1, 128), "torch.uint8") and c[1]["out"][2:] == ((1, 1, 128), "torch.bfloat16")
    assert st["kv"] == "fp8" and st["graph"] is None and user.length == 6 and st["user_cache"] is None


@pytest.mark.parametrize("B", [2, 9])
@pytest.mark.parametrize("enc", ["bf16", "fp8"])
def test_the_fp8_kv_batched_step(kv8_traces, B, enc):
    begin, step, _, st, _ = kv8_traces[("batch", B, enc)]
    lin = (["gemv_pg_batch_fp8"] if enc == "fp8" else ["gemv_pg_batch"]) if B <= 8 else None
    if lin:
        layer = lin + ["decode_attn_pg_kv8"] + lin * 3
        head = lin
    else:                                                    # more than 8 slots: the bf16 skinny-GEMM Linears, the e4m3 cache all the same
        layer = ["rmsnorm", "linear", "decode_attn_pg_kv8", "linear", "rmsnorm", "linear", "linear"]
        head = ["rmsnorm", "linear"]
    assert _names(step) == ["gather_rows", "mrope_table_into"] + layer * LAYERS + head + ["argmax_rows_bf16", "decode_advance_batch"]
    assert _names(begin) == ["kv_quant_e4m3"] * (2 * LAYERS * B)
    cap = st["cap"]
    assert cap % 64 == 0
    for c in step:
        if c[0] == "decode_attn_pg_kv8":
            a = c[1]
            assert a["k_codes"][2:] == ((B, cap, 1, 128), "torch.uint8") and a["v_codes"][2:] == ((B, cap, 1, 128), "torch.uint8")
            assert a["k_scale"][2:] == ((B, cap, 1), "torch.float32") and a["v_scale"][2:] == ((B, cap, 1), "torch.float32")
            assert a["scene_rows"] == a["max_len"] == cap
            assert len({a[n][1] for n in ("k_codes", "v_codes", "k_scale", "v_scale")}) == 4
    # an idle slot's first row: zero codes, scale 1 (it is the one key an idle slot attends to)
    own = st["cache8"]
    own.kc[:, 1, 0] = 9; own.ksc[:, 1, 0] = float("nan"); own.vc[:, 1, 0] = 9; own.vsc[:, 1, 0] = float("nan")
    Engine.decode_idle_slot(None, st, 1)
    assert (own.kc[:, 1, 0] == 0).all() and (own.vc[:, 1, 0] == 0).all() and (own.ksc[:, 1, 0] == 1).all() and (own.vsc[:, 1, 0] == 1).all()
    assert int(st["len"][1]) == 1 and int(st["row"][1]) == cap


def test_a_shared_prefix_state_keeps_its_bf16_blocks(kv8_traces):
    for enc in ("bf16", "fp8"):
        begin, step, _, st, _ = kv8_traces[("shared", 2, enc)]
        assert st["kv"] == "bf16" and not [n for n in _names(begin) + _names(step) if n in KV8_CALLS]
        attn = [c for c in step if c[0] == "decode_attn_shared"]
        assert len(attn) == LAYERS and len([c for c in step if c[0].startswith("decode_attn")]) == LAYERS
        for c in attn:
            assert c[1]["k_suffix"][3] == "torch.bfloat16" and c[1]["k_prefix"][3] == "torch.bfloat16"


def test_the_capture_key_keeps_the_weight_mode_last():
    mp = pytest.MonkeyPatch()
    try:
        w = TinyWeights(D.TINY["llm"])
        rec = Recorder(mp, w)
        for name in KV8_CALLS:
            mp.setattr(hip, name, rec._wrap(name, getattr(hip, name)))
        eng = Engine(w, D.TINY)
        mp.setattr(eng, "_capture", lambda st: None)
        for kv in ("bf16", "fp8"):
            for enc in ("bf16", "fp8"):
                eng.decode_weights, eng.decode_kv = enc, kv
                eng.decode_begin(filled_cache(D.TINY["llm"], 5, 1), 3, 5, 4, use_graph=True)
                (key,) = eng._decode_cached
                assert key[-1] == enc and key[-2] == kv, key
    finally:
        mp.undo()


# ------------------------------------------------------------------------------------------------ 4. build audit
@pytest.mark.timeout(1800)
def test_every_kv8_kernel_is_spill_free():
    if not os.path.exists(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from test_fp8_decode_cpu import _remarks
    rows = _remarks("decode_kv8.hip")
    for pat in ("kv_quant_e4m3_kernel", "kv_dequant_e4m3_kernel", "decode_attn_pg_kv8_kernel", "decode_combine_pg_kernel"):
        assert len([r for r in rows if pat in r["name"]]) == 1, pat
    for r in rows:
        assert int(r["ScratchSize [bytes/lane]"]) == 0, r
        assert int(r["VGPRs"]) + int(r.get("AGPRs", 0)) <= 256, r


# ------------------------------------------------------------------------------------------------ 5. the bound
def attention64(q, K, V, Hkv):
    """fp64 softmax attention of one query token: q [Hq, 128], K / V [L, Hkv, 128] -> [Hq, 128]."""
    Hq = q.shape[0]
    G = Hq // Hkv
    out = torch.empty((Hq, 128), dtype=torch.float64)
    for h in range(Hkv):
        p = torch.softmax((q[h * G:(h + 1) * G].double() @ K[:, h].double().T) * 128 ** -0.5, dim=-1)
        out[h * G:(h + 1) * G] = p @ V[:, h].double()
    return out


def roundtrip(x):
    """dequant(quant(x)) of cache rows x [rows, Hkv, 128] (bf16), on the host."""
    q, s = quantize_rows_e4m3(x.reshape(-1, 128))
    return dequantize_rows(q, s).view(x.shape)


def test_the_quantisation_bound_of_the_attention_output():
    """What an e4m3 cache costs the attention output, with nothing else in the way: fp64 attention over dequant(quant(K, V))
    against fp64 attention over K, V, Gaussian bf16 inputs, Hq 12, Hkv 2.  The worst rel-L2 over the lengths and seeds below
    was 4.3e-2 when the feature was written; tests/test_kv8_gpu.py allows the kernel 1.5 x the bound asserted here against the
    bf16 kernel on the unquantised rows."""
    Hq, Hkv, worst = 12, 2, 0.0
    for L in (1, 2, 33, 357, 4103):
        for seed in range(8):
            g = torch.Generator(); g.manual_seed(1000 * L + seed)
            q = torch.randn((Hq, 128), generator=g).bfloat16()
            K = torch.randn((L, Hkv, 128), generator=g).bfloat16()
            V = torch.randn((L, Hkv, 128), generator=g).bfloat16()
            want = attention64(q, K, V, Hkv)
            got = attention64(q, roundtrip(K), roundtrip(V), Hkv)
            r = float((got - want).norm() / want.norm())
            worst = max(worst, r)
    print(f"[kv8] fp64 attention over dequant(quant(K, V)) vs over K, V: worst rel-L2 {worst:.3e}")
    assert worst <= 4.5e-2, worst
