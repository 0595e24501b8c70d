"""CPU (no GPU): scoring given continuations (Engine.score_rows, G2VLM.score_continuations / chat_with_recon_choices,
csrc/logprob.hip).

1. The C ABI: g2v_logprob_rows_bf16 is exported and declared, argument errors come back as -22 before anything touches a
   device, the build remarks show no scratch.
2. The packing of continuations into rows, positions, targets and attention windows, on hand-written cases, and what the
   attention plan makes of those windows.
3. The entry-point sequence of one scoring pass, traced as tests/test_kv8_cpu.py traces the decode step: one lm_head GEMM and
   one logprob launch whatever the number of continuations, nothing of the FP8 modes, and nothing new in the decode step.
4. The ValueError cases of the two public methods.
"""
import ctypes as C
import inspect
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
from g2vlm_amd.engine import Engine, pack_continuations, score_windows  # noqa: E402
from test_decode_program_cpu import LAYERS, Recorder, TinyWeights, filled_cache  # noqa: E402
from test_kv8_cpu import KV8_CALLS  # noqa: E402

P, I, L64 = C.c_void_p, C.c_int, C.c_int64
NAMES = ("x", "rows", "n", "ld", "targets", "out_lp", "out_lse", "out_rank", "scratch", "scratch_bytes", "stream")


# ------------------------------------------------------------------------------------------------ 1. the C ABI
@pytest.fixture(scope="module")
def lib():
    from g2vlm_amd import build
    lib = C.CDLL(build.build())
    lib.g2v_logprob_rows_bf16.argtypes, lib.g2v_logprob_rows_bf16.restype = [P, I, I, L64, P, P, P, P, P, L64, P], I
    lib.g2v_logprob_rows_workspace.argtypes, lib.g2v_logprob_rows_workspace.restype = [I, I], L64
    return lib


def test_library_exports_and_declares_the_entry_point(lib):
    from g2vlm_amd import build
    hdr = open(os.path.join(ROOT, "include", "g2vlm_hip.h")).read()
    assert hasattr(lib, "g2v_logprob_rows_bf16") and "g2v_logprob_rows_bf16" in hip.EXPORTS
    assert re.search(r"\bint g2v_logprob_rows_bf16\(", hdr) and re.search(r"\bint64_t g2v_logprob_rows_workspace\(", hdr)
    assert "g2v_logprob_rows_workspace" in hip.EXPORTS
    assert "logprob.hip" in build.SOURCES and "logprob.hip" in build.RESOURCE_AUDIT
    assert list(inspect.signature(hip.logprob_rows_bf16).parameters)[:4] == ["logits", "targets", "lse", "rank"]
    # the declaration has as many parameters as the binding passes
    decl = re.search(r"\bint g2v_logprob_rows_bf16\((.*?)\);", hdr, re.S).group(1)
    assert len(decl.split(",")) == len(hip._SIGS["g2v_logprob_rows_bf16"][0]) == len(NAMES)


def call(lib, **kw):
    """A valid argument set (no pointer is dereferenced: every call below is refused before any launch), with overrides."""
    a = dict(x=16, rows=3, n=100, ld=100, targets=16, out_lp=16, out_lse=16, out_rank=16, scratch=None, scratch_bytes=0, stream=None)
    a.update(kw)
    return lib.g2v_logprob_rows_bf16(*[a[k] for k in NAMES])


@pytest.mark.parametrize("bad", [dict(rows=0), dict(rows=-1), dict(n=0), dict(n=-5), dict(ld=99), dict(ld=0), dict(x=None), dict(targets=None),
                                 dict(out_lp=None), dict(x=None, out_lse=None, out_rank=None), dict(rows=0, scratch=16, scratch_bytes=1 << 20)])
def test_argument_errors_return_einval_without_a_device(lib, bad):
    assert call(lib, **bad) == -22


def test_the_workspace_is_only_asked_for_where_rows_are_split(lib):
    ws = lib.g2v_logprob_rows_workspace
    assert ws(0, 100) == 0 and ws(3, 0) == 0 and ws(-1, -1) == 0
    assert ws(1, 8192) == 0 and ws(64, 7) == 0               # one chunk per row: nothing to split
    assert ws(512, 151936) == 0 and ws(4096, 151936) == 0    # the rows fill the chip by themselves
    for rows in (1, 3, 64, 65, 511):
        assert ws(rows, 151936) == 4 * (512 + rows * 19 * 3)   # 19 chunks of 8192 elements, 3 words each, behind 512 tickets
    assert ws(1, 8193) == 4 * (512 + 2 * 3)


@pytest.mark.timeout(1800)
def test_the_kernel_is_spill_free():
    if not os.path.exists(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from test_fp8_decode_cpu import _remarks
    rows = _remarks("logprob.hip")
    assert len([r for r in rows if "logprob_rows_bf16_kernel" in r["name"]]) == 1 and len(rows) == 1, [r["name"] for r in rows]
    for r in rows:
        assert int(r["ScratchSize [bytes/lane]"]) == 0, r
        assert int(r["VGPRs Spill"]) == 0, r


# ------------------------------------------------------------------------------------------------ 2. the packing
def test_packing_one_continuation_of_one_token():
    assert pack_continuations(7, 40, [[99]]) == ([7], [40], [1], [99])
    assert score_windows(12, [1]) == ((0, 1, 0, 12, False), (0, 1, 12, 1, True))
    assert score_windows(0, [1]) == ((0, 1, 0, 1, True),)


def test_packing_three_continuations():
    ids, pos, lens, tgt = pack_continuations(7, 40, [[11], [21, 22, 23, 24, 25], [31, 32]])
    assert ids == [7, 7, 21, 22, 23, 24, 7, 31]
    assert pos == [40, 40, 41, 42, 43, 44, 40, 41]
    assert lens == [1, 5, 2]
    assert tgt == [11, 21, 22, 23, 24, 25, 31, 32]
    assert score_windows(100, lens) == ((0, 1, 0, 100, False), (0, 1, 100, 1, True),
                                        (1, 5, 0, 100, False), (1, 5, 101, 5, True),
                                        (6, 2, 0, 100, False), (6, 2, 106, 2, True))
    with pytest.raises(ValueError):
        pack_continuations(7, 40, [[1], []])


def test_packing_64_continuations():
    conts = [[1000 + j] * (1 + j % 3) for j in range(64)]
    ids, pos, lens, tgt = pack_continuations(5, 9, conts)
    assert lens == [1 + j % 3 for j in range(64)] and len(ids) == len(pos) == len(tgt) == sum(lens) == 127
    wins = score_windows(33, lens)
    assert len(wins) == 128
    off = 0
    for j, c in enumerate(conts):
        n = len(c)
        assert ids[off:off + n] == [5] + c[:-1] and pos[off:off + n] == list(range(9, 9 + n)) and tgt[off:off + n] == c
        assert wins[2 * j] == (off, n, 0, 33, False) and wins[2 * j + 1] == (off, n, 33 + off, n, True)
        off += n
    # every query row is in exactly two windows, every scored cache row in exactly one
    q_cover, k_cover = [0] * 127, [0] * 127
    for q0, ql, k0, kl, causal in wins:
        for r in range(q0, q0 + ql):
            q_cover[r] += 1
        if causal:
            for r in range(k0 - 33, k0 - 33 + kl):
                k_cover[r] += 1
    assert q_cover == [2] * 127 and k_cover == [1] * 127


def test_the_attention_plan_expresses_these_windows():
    """make_attn_plan on the windows of 1 / 5 / 2 tokens over a 100-row prefix: one tile per window, the causal one starting
    at its own keys with shift k_len - q_len = 0 (row i of the segment sees its keys 0 .. i), and one merge per segment and
    head over the partial results of its two windows."""
    Hq = 2
    wins = score_windows(100, [1, 5, 2])
    plan = hip.make_attn_plan(wins, Hq, torch.device("cpu"))
    assert plan.n_tiles == 6 and len(plan.phases) == 1 and plan.tile_rows == 128
    tiles = plan.tiles.tolist()
    for (q0, ql, k0, kl, causal), t in zip(wins, tiles):
        assert t[:4] == [q0, ql, k0, kl] and t[5] == q0
        assert t[4] == (0 if causal else hip.NO_CAUSAL)
    assert plan.n_comb == 3 * Hq
    comb = plan.comb.view(-1, 4).tolist()
    assert sorted((c[0], c[1]) for c in comb) == sorted((d, h) for d in (0, 2, 4) for h in range(Hq)) 
    assert all(c[3] >= 2 for c in comb) and sum(c[3] for c in comb) == plan.n_slots   # the prefix window may be cut further


# ------------------------------------------------------------------------------------------------ 3. the program of one pass
PREFILL_CALLS = ("gemm_bf16", "flash_attn", "logprob_rows_bf16")
FP8_CALLS = ("gemv_pg_fp8", "gemv_pg_batch_fp8") + KV8_CALLS


class ScoreWeights(TinyWeights):
    """TinyWeights plus what a prefill on the und expert names of the geo expert (split = 0: named, never applied)."""

    def __init__(self, Lc):
        super().__init__(Lc)
        H = Lc["hidden"]
        self.t["norm.geo"] = torch.ones(H)
        for i in range(Lc["layers"]):
            for n, size in (("geo.ln1", H), ("geo.ln2", H), ("geo.qn", 128), ("geo.kn", 128), ("ls1", H), ("ls2", H)):
                self.t[f"L{i}.{n}"] = torch.ones(size)


@pytest.fixture(scope="module")
def traced():
    """(recorder, engine) with every entry point of the decode step and of the prefill replaced by recorders."""
    mp = pytest.MonkeyPatch()
    try:
        w = ScoreWeights(D.TINY["llm"])
        rec = Recorder(mp, w)
        for name in PREFILL_CALLS + KV8_CALLS:
            mp.setattr(hip, name, rec._wrap(name, getattr(hip, name)))
        rms = hip.rmsnorm                                      # the recorder; the final norm is called without `out`

        def rmsnorm(x, w_lo, w_hi, split, eps, out_dtype=torch.bfloat16, out=None):
            if out is None:
                out = torch.empty(x.shape, dtype=out_dtype)
            return rms(x, w_lo, w_hi, split, eps, out_dtype, out)
        mp.setattr(hip, "rmsnorm", rmsnorm)
        mp.setattr(hip, "mrope_table", lambda pos, inv_freq: (rec.calls.append(("mrope_table", {"L": pos.shape[1]})),
                                                              (torch.empty(pos.shape[1], 128), torch.empty(pos.shape[1], 128)))[1])
        plans = []
        mp.setattr(hip, "make_attn_plan", lambda windows, Hq, device, **kw: plans.append((tuple(windows), Hq, kw)) or ("plan", len(plans)))
        eng = Engine(w, D.TINY)
        yield rec, eng, plans
    finally:
        mp.undo()


def score_trace(rec, eng, seg_lens, prefix=6):
    Lc = D.TINY["llm"]
    cache = filled_cache(Lc, prefix, 3)
    before = [(cache.k[i][:prefix].clone(), cache.v[i][:prefix].clone()) for i in range(Lc["layers"])]
    n = sum(seg_lens)
    rec.take()
    lp, rank = eng.score_rows(cache, prefix, torch.zeros(n, dtype=torch.int32), torch.zeros((3, n), dtype=torch.int32), seg_lens,
                              torch.zeros(n, dtype=torch.int32))
    assert cache.length == prefix and lp.shape == (n,) and lp.dtype == torch.float32 and rank.shape == (n,) and rank.dtype == torch.int32
    for i, (k, v) in enumerate(before):
        assert torch.equal(cache.k[i][:prefix], k) and torch.equal(cache.v[i][:prefix], v)
    return rec.take()


def _names(calls):
    return [c[0] for c in calls]


LAYER = ["rmsnorm", "gemm_bf16", "qknorm_mrope_cache", "flash_attn", "gemm_bf16", "rmsnorm", "gemm_bf16", "gemm_bf16"]


@pytest.mark.parametrize("seg_lens", [[1], [1, 5, 2], [2] * 64, [40, 31]])
def test_one_pass_one_lm_head_gemm_one_logprob_launch(traced, seg_lens):
    rec, eng, plans = traced
    calls = score_trace(rec, eng, seg_lens)
    n = sum(seg_lens)
    assert _names(calls) == ["gather_rows", "mrope_table"] + LAYER * LAYERS + ["rmsnorm", "linear", "logprob_rows_bf16"]
    assert plans[-1][0] == score_windows(6, seg_lens)
    V, H = D.TINY["llm"]["vocab"], D.TINY["llm"]["hidden"]
    (head,) = [c for c in calls if c[0] == "linear"]
    assert head[1]["w"][:2] == ("w", "lm_head") and head[1]["x"][2:] == ((n, H), "torch.bfloat16") and head[1]["out"][2:] == ((n, V), "torch.bfloat16")
    assert head[1]["x"][1] == calls[-3][1]["out"][1]           # the bf16 final norm feeds it
    (lp,) = [c for c in calls if c[0] == "logprob_rows_bf16"]
    assert lp[1]["logits"][1] == head[1]["out"][1] and lp[1]["targets"][2:] == ((n,), "torch.int32")
    assert lp[1]["out"][2:] == ((n,), "torch.float32") and lp[1]["rank"][2:] == ((n,), "torch.int32")
    lm_head = eng.w["lm_head"].data_ptr()
    for c in calls:                                            # no other launch reads lm_head
        if c[0] == "gemm_bf16":
            assert all(g["W"].data_ptr() != lm_head for g in c[1]["groups"])
    # the rows' K / V go to the cache rows behind the prefix, in order
    for c in calls:
        if c[0] == "qknorm_mrope_cache":
            assert c[1]["split"] == 0 and c[1]["und_rounding"] == 1 and c[1]["kv_rows"][2:] == ((n,), "torch.int32")


def test_the_fp8_modes_do_not_reach_the_scoring_pass(traced):
    rec, eng, _ = traced
    plain = _names(score_trace(rec, eng, [1, 5, 2]))
    eng.decode_weights, eng.decode_kv = "fp8", "fp8"
    try:
        calls = score_trace(rec, eng, [1, 5, 2])
    finally:
        eng.decode_weights, eng.decode_kv = "bf16", "bf16"
    assert _names(calls) == plain and not [n for n in _names(calls) if n in FP8_CALLS]
    described = repr(calls)
    assert ".w8" not in described and ".ws" not in described and "uint8" not in described


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_the_decode_step_calls_nothing_new(traced, weights, kv):
    rec, eng, _ = traced
    eng.decode_weights, eng.decode_kv = weights, kv
    try:
        rec.take()
        st = eng.decode_begin(filled_cache(D.TINY["llm"], 5, 1), 3, 5, 4, use_graph=False)
        begin = rec.take()
        eng.decode_step(st)
        step = rec.take()
        eng.decode_end(st)
        end = rec.take()
    finally:
        eng.decode_weights, eng.decode_kv = "bf16", "bf16"
    new = PREFILL_CALLS + ("mrope_table", "linear", "rmsnorm", "qknorm_mrope_cache")
    assert not [n for n in _names(begin) + _names(step) + _names(end) if n in new]
    lin = "gemv_pg_fp8" if weights == "fp8" else "gemv_pg"
    att = "decode_attn_pg_kv8" if kv == "fp8" else "decode_attn_pg"
    assert _names(step) == ["gather_rows", "mrope_table_into"] + [lin, att, lin, lin, lin] * LAYERS + [lin, "argmax_bf16", "decode_advance"]


def test_only_the_most_recent_scoring_plans_are_kept(traced):
    rec, eng, plans = traced
    other = ((0, 4, 0, 4, False),)
    eng.plan(other, 2)                                         # somebody else's plan: never evicted by scoring
    built = len(plans)
    for prefix in range(3, 3 + Engine.SCORE_PLANS_KEPT + 5):
        score_trace(rec, eng, [2, 1], prefix=prefix)
    mine = [k for k in eng._tiles if k in eng._score_plans]
    assert len(mine) == len(eng._score_plans) == Engine.SCORE_PLANS_KEPT and (other, 2) in eng._tiles
    assert len(plans) == built + Engine.SCORE_PLANS_KEPT + 5
    newest = (score_windows(3 + Engine.SCORE_PLANS_KEPT + 4, [2, 1]), D.TINY["llm"]["heads"])
    oldest = (score_windows(3, [2, 1]), D.TINY["llm"]["heads"])
    assert newest in eng._tiles and oldest not in eng._tiles
    score_trace(rec, eng, [2, 1], prefix=3 + Engine.SCORE_PLANS_KEPT + 4)      # a kept shape is not rebuilt
    assert len(plans) == built + Engine.SCORE_PLANS_KEPT + 5


def test_score_rows_refuses_what_it_cannot_take(traced):
    rec, eng, _ = traced
    cache = filled_cache(D.TINY["llm"], 4, 0)
    z = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731
    for seg_lens in ([], [1] * 65, [3, 0], [Engine.SCORE_MAX_ROWS + 1], [Engine.SCORE_MAX_ROWS // 2 + 1] * 2):
        n = sum(seg_lens)
        with pytest.raises(ValueError):
            eng.score_rows(cache, 4, z(n), torch.zeros((3, n), dtype=torch.int32), seg_lens, z(n))
    assert cache.length == 4 and not rec.take()


# ------------------------------------------------------------------------------------------------ 4. the public methods
class Tok:
    eos_token_id = 2

    def __init__(self, table):
        self.table = table

    def encode(self, text, add_special_tokens=True):
        assert add_special_tokens is False
        return list(self.table[text])


def bare_model():
    from g2vlm_amd.modeling.g2vlm.g2vlm import G2VLM
    m = G2VLM.__new__(G2VLM)
    m.dims = D.TINY

    def no_prefill(*a, **kw):
        raise AssertionError("the prefill ran before the arguments were checked")
    m._chat_prefill = no_prefill
    return m


def test_score_continuations_value_errors():
    m, V = bare_model(), D.TINY["llm"]["vocab"]
    for bad in ([], [[1]] * 65, [[1], []], [[V]], [[-1]], [[1] * (Engine.SCORE_MAX_ROWS + 1)], [[1] * 200] * 64):
        with pytest.raises(ValueError):
            m.score_continuations(None, None, bad)


def test_chat_with_recon_choices_value_errors_come_before_the_prefill():
    m = bare_model()
    tok = Tok({"a": [7], "b": [8, 9], "": [], "long": [5] * (Engine.SCORE_MAX_ROWS + 1)})
    nt = dict(eos_token_id=2)
    for choices in ([], ["a"] * 65, ["a", ""], ["long"]):
        with pytest.raises(ValueError):
            m.chat_with_recon_choices(tok, nt, None, None, None, "q", choices)
    with pytest.raises(AssertionError, match="prefill ran"):    # valid choices do reach the prefill
        m.chat_with_recon_choices(tok, nt, None, None, None, "q", ["a", "b"])
    sig = inspect.signature(type(m).chat_with_recon_choices).parameters
    assert sig["append_eos"].default is True and sig["normalize"].default is False
    assert "--choices" in open(os.path.join(ROOT, "inference_chat.py")).read()
