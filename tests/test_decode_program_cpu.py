"""CPU (no GPU): the decode step PROGRAM and the persistent-grid GEMV ROUTES.

1. The step program (g2vlm_amd/decode.py).  Every hip.* entry point the step calls is replaced by a recorder, the engine is
   built on CPU tensors at the TINY LLM dims, and one eager step is run in every mode: batch 1, B = 2 / 8 / 9 slots, B = 2 / 8 / 9
   questions over a shared prefix, each with the generation-1 kernels, the persistent-grid kernels and those on e4m3 weights,
   each greedy and sampled (42 traces).  The expected entry-point sequence of every mode is written out below; the weights and
   the buffer shapes of the five Linears are checked; no mode may call an entry point of another family.
2. The routes (csrc/decode_dispatch.h through g2v_gemv_pg_route): the production Linears' rows are pinned to what the four
   entry points launched before they shared one plan function, and the route refuses every shape the entry points refuse.
"""
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import dims as D  # noqa: E402

from g2vlm_amd import hip  # noqa: E402
from g2vlm_amd.engine import Engine, KVCache  # noqa: E402
from g2vlm_amd.weights import interleave_gate_up  # noqa: E402

# ------------------------------------------------------------------------------------------------ 1. the recorder
STEP_CALLS = ("gather_rows", "mrope_table_into", "gemv_rmsnorm_bf16", "gemv_bf16", "gemv_rmsnorm_swiglu_bf16", "gemv_pg", "gemv_pg_fp8",
              "gemv_pg_batch", "gemv_pg_batch_fp8", "rmsnorm", "linear", "decode_attn_pg", "decode_attn_fused", "decode_attn_batch",
              "decode_attn_shared", "qknorm_mrope_cache", "argmax_bf16", "argmax_rows_bf16", "sample_rows_bf16", "decode_advance",
              "decode_advance_batch")
HOST_STUBS = {                                             # sizes that depend on every argument, so a changed argument shows
    "decode_attn_workspace": lambda Lk, Hq: 4 * (Lk + 7 * Hq),
    "decode_attn_pg_workspace": lambda Hq, Hkv, batch=1: 4 * (130 * Hq + 3 * Hkv + 1000 * batch),
    "decode_attn_shared_workspace": lambda Hq, Hkv, batch, prefix_len, suffix_max_len: 4 * (11 * Hq + 3 * Hkv + 1000 * batch + prefix_len
                                                                                            + 5 * suffix_max_len),
    "make_rng": lambda seed, temperature, device: torch.tensor([seed, int(temperature * 1000), 0, 0], dtype=torch.int64, device=device),
}


class TinyWeights:
    """The tensors the decode step touches, at the TINY LLM dims, on the CPU."""

    def __init__(self, L):
        H, Hq, Hkv, Fd, V = L["hidden"], L["heads"], L["kv_heads"], L["ffn"], L["vocab"]
        g = torch.Generator(); g.manual_seed(0)
        r = lambda *s: torch.randn(s, generator=g) * 0.05  # noqa: E731
        self.device, self.t = torch.device("cpu"), {}
        t = self.t
        t["embed"], t["lm_head"], t["norm.und"] = r(V, H), r(V, H).bfloat16(), torch.ones(H)
        t["inv_freq"] = 1.0 / (L["theta"] ** (torch.arange(0, 128, 2).float() / 128))
        for i in range(L["layers"]):
            p = f"L{i}.und."
            t[p + "qkv.w"], t[p + "qkv.b"] = r((Hq + 2 * Hkv) * 128, H).bfloat16(), r((Hq + 2 * Hkv) * 128).bfloat16()
            t[p + "o.w"], t[p + "down.w"] = r(H, Hq * 128).bfloat16(), r(H, Fd).bfloat16()
            t[p + "gu.w"] = interleave_gate_up(r(Fd, H), r(Fd, H)).bfloat16()
            for n in ("qn", "kn"):
                t[p + n] = torch.ones(128)
            t[p + "ln1"], t[p + "ln2"] = torch.ones(H), torch.ones(H)

    def __getitem__(self, k):
        return self.t[k]


class Recorder:
    """Replaces the step's hip.* entry points.  A call is (name, {parameter: value}) with the arguments bound to the real
    function's signature (defaults applied); a tensor is ("w", weight name) or ("buf", number of the buffer in order of first
    use - so aliasing is part of the trace), with its shape and dtype; a list entry of the KV cache is a buffer like any other."""

    def __init__(self, monkeypatch, weights):
        self.calls, self.w, self.bufs = [], weights, {}
        for name in STEP_CALLS:
            monkeypatch.setattr(hip, name, self._wrap(name, getattr(hip, name)))
        for name, fn in HOST_STUBS.items():
            monkeypatch.setattr(hip, name, fn)

    def _wrap(self, name, real):
        sig = inspect.signature(real)

        def rec(*a, **kw):
            b = sig.bind(*a, **kw)
            b.apply_defaults()
            self.calls.append((name, {k: self._describe(v) for k, v in b.arguments.items()}))
            return b.arguments.get("out")
        return rec

    def _describe(self, v):
        if not isinstance(v, torch.Tensor):
            return v if not isinstance(v, torch.dtype) else str(v)
        shape, dt = tuple(v.shape), str(v.dtype)
        for name, t in self.w.t.items():
            if t.data_ptr() == v.data_ptr() and t.shape == v.shape:
                return ("w", name, shape, dt)
        return ("buf", self.bufs.setdefault(v.data_ptr(), len(self.bufs)), shape, dt)

    def take(self):
        calls, self.calls, self.bufs = self.calls, [], {}
        return calls


GENS = ((1, "bf16"), (2, "bf16"), (2, "fp8"))
MODES = [("b1", 1)] + [("batch", B) for B in (2, 8, 9)] + [("shared", B) for B in (2, 8, 9)]


def filled_cache(L, n, seed):
    c = KVCache(L["layers"], L["kv_heads"], "cpu", capacity=n)
    g = torch.Generator(); g.manual_seed(seed)
    for i in range(L["layers"]):
        c.k[i][:n] = torch.randn((n, L["kv_heads"], 128), generator=g).bfloat16()
        c.v[i][:n] = torch.randn((n, L["kv_heads"], 128), generator=g).bfloat16()
    c.length = n
    return c


def one_trace(rec, eng, mode, B, gen, enc, sampled, cap_rows=None):
    """The calls of one eager step.  cap_rows: open the slots with this many rows instead (batch mode)."""
    L = eng.dims["llm"]
    eng.decode_weights = "bf16"
    eng.decode_gen = gen
    eng.decode_weights = enc
    sample = (7, 0.5) if sampled else None
    if mode == "b1":
        st = eng.decode_begin(filled_cache(L, 5, 1), 3, 5, 4, use_graph=False, sample=sample)
        rec.take()
        eng.decode_step(st)
    elif mode == "batch" and cap_rows:
        st = eng.decode_open_slots(B, cap_rows, use_graph=False, sample=sample)
        rec.take()
        eng.decode_step_batch(st)
    elif mode == "batch":
        st = eng.decode_begin_batch([filled_cache(L, 4 + j, j) for j in range(B)], [3] * B, [5] * B, 4, use_graph=False, sample=sample)
        rec.take()
        eng.decode_step_batch(st)
    else:
        st = eng.decode_begin_shared(filled_cache(L, 6, 99), [filled_cache(L, 2 + j % 3, j) for j in range(B)], [3] * B, [9] * B, 4,
                                     use_graph=False, sample=sample)
        rec.take()
        eng.decode_step_batch(st)
    return rec.take(), st


def all_traces(monkeypatch):
    """{(mode, B, gen, encoding, sampled): calls} for the 42 modes plus the split-attention one."""
    w = TinyWeights(D.TINY["llm"])
    rec = Recorder(monkeypatch, w)
    eng = Engine(w, D.TINY)
    out = {}
    for mode, B in MODES:
        for gen, enc in GENS:
            for sampled in (False, True):
                out[(mode, B, gen, enc, sampled)] = one_trace(rec, eng, mode, B, gen, enc, sampled)[0]
    out[("batch-split", 9, 1, "bf16", False)] = one_trace(rec, eng, "batch", 9, 1, "bf16", False, cap_rows=SPLIT_CAP)[0]
    return out


# 9 slots x ceil(cap / 256) key blocks x 1 kv head > 512 workgroups: the fused attention no longer fits the chip at once
SPLIT_CAP = 58 * 256

# ------------------------------------------------------------------------------------------------ 2. the expected programs
LAYERS = 2
LINEAR_FAMILY = {                                          # qkv, o, gate/up, down as the family issues them
    "gemv1": (["gemv_rmsnorm_bf16"], ["gemv_bf16"], ["gemv_rmsnorm_swiglu_bf16"], ["gemv_bf16"]),
    "pg": (["gemv_pg"],) * 4,
    "pg8": (["gemv_pg_fp8"],) * 4,
    "pgb": (["gemv_pg_batch"],) * 4,
    "pgb8": (["gemv_pg_batch_fp8"],) * 4,
    "skinny": (["rmsnorm", "linear"], ["linear"], ["rmsnorm", "linear"], ["linear"]),
}
LM_HEAD = {"gemv1": ["gemv_rmsnorm_bf16"], "pg": ["gemv_pg"], "pg8": ["gemv_pg_fp8"], "pgb": ["gemv_pg_batch"], "pgb8": ["gemv_pg_batch_fp8"],
           "skinny": ["rmsnorm", "linear"]}
ATTENTION = {"pg": ["decode_attn_pg"], "fused": ["decode_attn_fused"], "split": ["qknorm_mrope_cache", "decode_attn_batch"],
             "shared": ["decode_attn_shared"]}
FAMILY_CALLS = {f: set(sum(v, [])) for f, v in LINEAR_FAMILY.items()}


def expected_forms(mode, B, gen, enc):
    """(Linear family, attention form) by the selection rules of the step."""
    if mode == "b1":
        return ("gemv1", "fused") if gen == 1 else (("pg8" if enc == "fp8" else "pg"), "pg")
    pg = gen == 2 and B <= 8
    family = ("pgb8" if enc == "fp8" else "pgb") if pg else "skinny"
    attn = "shared" if mode == "shared" else ("pg" if gen == 2 else ("split" if mode == "batch-split" else "fused"))
    return family, attn


def expected_names(mode, family, attn, sampled):
    qkv, o, gu, down = LINEAR_FAMILY[family]
    layer = qkv + ATTENTION[attn] + o + gu + down
    pick = "sample_rows_bf16" if sampled else ("argmax_bf16" if mode == "b1" else "argmax_rows_bf16")
    return ["gather_rows", "mrope_table_into"] + layer * LAYERS + LM_HEAD[family] + [pick, "decode_advance" if mode == "b1" else "decode_advance_batch"]


@pytest.fixture(scope="module")
def traces():
    mp = pytest.MonkeyPatch()
    try:
        yield all_traces(mp)
    finally:
        mp.undo()


def test_the_matrix_is_the_42_modes_and_the_split_attention(traces):
    assert len(traces) == 43
    assert len([k for k in traces if k[0] != "batch-split"]) == 7 * 3 * 2


def test_every_mode_runs_its_literal_entry_point_sequence(traces):
    for key, calls in traces.items():
        mode, B, gen, enc, sampled = key
        family, attn = expected_forms(mode, B, gen, enc)
        names = [c[0] for c in calls]
        assert names == expected_names(mode, family, attn, sampled), (key, names)
        assert len(names) == {"skinny": 20}.get(family, 15) + (2 if attn == "split" else 0), key


def test_an_fp8_step_at_batch_1_reads(traces):
    """The example of the issue, literally."""
    names = [c[0] for c in traces[("b1", 1, 2, "fp8", False)]]
    assert names == ["gather_rows", "mrope_table_into",
                     "gemv_pg_fp8", "decode_attn_pg", "gemv_pg_fp8", "gemv_pg_fp8", "gemv_pg_fp8",
                     "gemv_pg_fp8", "decode_attn_pg", "gemv_pg_fp8", "gemv_pg_fp8", "gemv_pg_fp8",
                     "gemv_pg_fp8", "argmax_bf16", "decode_advance"]


def test_no_mode_calls_an_entry_point_of_another_family(traces):
    linear_calls = set().union(*FAMILY_CALLS.values())
    attn_calls = set(sum(ATTENTION.values(), []))
    for key, calls in traces.items():
        mode, B, gen, enc, sampled = key
        family, attn = expected_forms(mode, B, gen, enc)
        names = [c[0] for c in calls]
        for foreign in linear_calls - FAMILY_CALLS[family]:
            assert names.count(foreign) == 0, (key, foreign)
        for foreign in attn_calls - set(ATTENTION[attn]):
            assert names.count(foreign) == 0, (key, foreign)
    assert [c[0] for c in traces[("b1", 1, 2, "fp8", False)]].count("gemv_pg") == 0
    assert not [c for c in traces[("batch", 9, 2, "fp8", False)] if c[0].startswith("gemv_pg_batch")]


def _weight_args(call):
    return [v[1] for v in call[1].values() if isinstance(v, tuple) and v[0] == "w"]


def _shape(call, arg):
    v = call[1][arg]
    return None if v is None else v[2]


def test_the_linears_stream_their_weights_into_buffers_of_the_right_shape(traces):
    L = D.TINY["llm"]
    H, nq, nqkv, Fd, V = L["hidden"], L["heads"] * 128, (L["heads"] + 2 * L["kv_heads"]) * 128, L["ffn"], L["vocab"]
    for key, calls in traces.items():
        mode, B, gen, enc, sampled = key
        family, _ = expected_forms(mode, B, gen, enc)
        rows = (lambda n: (n,)) if mode == "b1" else (lambda n: (B, n))
        fp8 = family in ("pg8", "pgb8")
        lin = [c for c in calls if c[0] in FAMILY_CALLS[family] and c[0] != "rmsnorm"]
        assert len(lin) == 4 * LAYERS + 1, key
        want = [(f"L{i}.und.{n}", shp) for i in range(LAYERS) for n, shp in (("qkv", nqkv), ("o", H), ("gu", Fd), ("down", H))]
        for c, (name, n_out) in zip(lin, want + [("lm_head", V)]):
            stem = name.split(".")[-1]
            ws = _weight_args(c)
            if fp8:
                assert set(ws) >= {name + ".w8", name + ".ws"}, (key, c[0], ws)
                assert not [n for n in ws if n.endswith(".w") or n == "lm_head"], (key, ws)
            else:
                assert ("lm_head" if name == "lm_head" else name + ".w") in ws, (key, c[0], ws)
                assert not [n for n in ws if n.endswith((".w8", ".ws"))], (key, ws)
            if stem == "qkv":
                assert f"L{name[1]}.und.qkv.b" in ws, (key, ws)
            # where the result goes: the fp32 residual stream for o / down, a bf16 buffer of the Linear's width otherwise
            if stem in ("o", "down"):
                assert _shape(c, "res") == rows(H), (key, c)
            else:
                out = "act_out" if c[0] == "gemv_rmsnorm_swiglu_bf16" else "out"
                assert _shape(c, out) == rows(n_out), (key, c)
        # the fused norms: eps travels with the norm weight and only with it
        for c in lin:
            if "norm_w" in c[1] and c[0].startswith("gemv_pg"):
                assert c[1]["eps"] == (0.0 if c[1]["norm_w"] is None else L["eps"]), (key, c)
        if mode == "b1":
            assert _shape(calls[-2], "x") == (V,), key
        else:
            assert _shape(calls[-2], "x") == (B, V), key


def test_the_attention_reads_the_state_s_cache_rows_and_caps(traces):
    for key, calls in traces.items():
        mode, B, gen, enc, sampled = key
        for c in calls:
            if c[0] in ("decode_attn_pg", "decode_attn_fused", "decode_attn_batch", "decode_attn_shared"):
                a = c[1]
                if c[0] == "decode_attn_shared":
                    a = dict(scene_rows=a["suffix_rows"], max_len=a["suffix_max_len"])
                    assert c[1]["prefix_len"] == 6
                assert a["scene_rows"] >= a["max_len"] > 0, (key, c)
                if mode == "b1":
                    assert a["max_len"] % 4096 == 0 or c[0] == "decode_attn_fused", (key, c)
                else:
                    assert a["scene_rows"] == a["max_len"] and a["max_len"] % 64 == 0, (key, c)


# ------------------------------------------------------------------------------------------------ 3. the routes
# (B, fp8) -> route of qkv 2048 x 1536 norm + bias, o 1536 x 1536, gate/up 17920 x 1536 norm + act, down 1536 x 8960,
# lm_head 151936 x 1536 norm: {form, threads per block, RB (R for form 3), KCH (CW / S for form 3)}.  Taken from the decision
# code of the four entry points as it stood when each had its own copy (B == 0: the batch-1 entry points).
PRODUCTION = (("qkv", 2048, 1536, 0, 1), ("o", 1536, 1536, 0, 0), ("gu", 17920, 1536, 1, 1), ("down", 1536, 8960, 0, 0),
              ("lm_head", 151936, 1536, 0, 1))
ROUTES = {(0, 0): ((1, 256, 2, 3), (1, 192, 2, 3), (1, 448, 5, 3), (1, 384, 1, 18), (1, 384, 8, 3)),
          (0, 1): ((1, 256, 2, 2), (1, 192, 2, 2), (1, 448, 6, 2), (1, 384, 1, 9), (1, 384, 12, 2))}
for _Bs, _bf16, _fp8 in (                                  # B rows run as NB = 2, 4 or 8 scenes per weight pass
        ((1, 2), ((2, 512, 1, 3), (2, 512, 1, 3), (2, 512, 5, 3), (3, 512, 6, 140), (2, 512, 5, 3)),
                 ((2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 4, 2), (3, 576, 8, 9), (2, 512, 4, 2))),
        ((3, 4), ((2, 512, 1, 3), (2, 512, 1, 3), (2, 512, 3, 3), (3, 512, 6, 140), (2, 512, 3, 3)),
                 ((2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 4, 2), (3, 576, 8, 9), (2, 512, 4, 2))),
        ((5, 6, 7, 8), ((2, 512, 1, 3), (2, 512, 1, 3), (2, 512, 2, 3), (3, 512, 6, 140), (2, 512, 2, 3)),
                       ((2, 512, 1, 2), (2, 512, 1, 2), (2, 512, 2, 2), (3, 576, 4, 9), (2, 512, 2, 2)))):
    for _B in _Bs:
        ROUTES[(_B, 0)], ROUTES[(_B, 1)] = _bf16, _fp8


@pytest.fixture(scope="module")
def built():
    from g2vlm_amd import build
    build.build()
    return hip


def test_the_route_is_exported_and_declared(built):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "g2vlm_hip.h")).read()
    assert "g2v_gemv_pg_route" in hip.EXPORTS and "int g2v_gemv_pg_route(" in hdr and hasattr(hip.lib(), "g2v_gemv_pg_route")


def test_production_routes_are_pinned(built):
    assert sorted(ROUTES) == sorted((B, f) for B in range(9) for f in (0, 1))
    for (B, fp8), rows in ROUTES.items():
        for (name, N, K, act, norm), want in zip(PRODUCTION, rows):
            assert hip.gemv_pg_route(B, N, K, act, norm, fp8) == want, (B, fp8, name)


@pytest.mark.parametrize("fp8", [0, 1])
@pytest.mark.parametrize("B", [0, 2])
@pytest.mark.parametrize("bad", [dict(K=1528), dict(K=1544), dict(K=0), dict(N=0), dict(K=1 << 20), dict(act=1, norm=1, N=2040),
                                 dict(act=1, norm=0, N=2048), dict(norm=1, K=1552), dict(norm=1, K=8960)])
def test_route_refuses_what_the_entry_points_refuse(built, B, fp8, bad):
    """The shape cases of tests/test_fp8_decode_cpu.py (its pointer cases have no counterpart: the route takes no pointers).
    K = 1528 and 1544 are multiples of 8, not of 16: refused in e4m3 only."""
    a = dict(B=B, N=2048, K=1536, act=0, norm=0, fp8=fp8)
    a.update(bad)
    out = (hip.C.c_int32 * 4)()
    rc = hip.lib().g2v_gemv_pg_route(a["B"], a["N"], a["K"], a["act"], a["norm"], a["fp8"], hip.C.byref(out))
    legal_in_bf16 = not fp8 and bad in (dict(K=1528), dict(K=1544))
    assert rc == (0 if legal_in_bf16 else -22), (a, rc)


def test_route_k_and_b_limits(built):
    for fp8 in (0, 1):
        assert hip.gemv_pg_route(0, 2048, 9216, fp8=fp8)[0] == 1 and hip.gemv_pg_route(8, 2048, 12288, fp8=fp8)[0] == 3
        for B, K in ((0, 9216 + 16), (1, 12288 + 16), (9, 1536), (-1, 1536), (64, 1536)):
            with pytest.raises(hip.HipError):
                hip.gemv_pg_route(B, 2048, K, fp8=fp8)
