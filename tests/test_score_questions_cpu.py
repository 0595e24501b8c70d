"""CPU (no GPU): scoring the choices of several questions about one scene in one pass, with top-k tokens (Engine.score_questions,
G2VLM.score_questions / chat_with_recon_questions_choices, csrc/topk.hip), in the style of tests/test_score_cpu.py.

1. The C ABI of g2v_topk_rows_bf16: exported and declared, argument errors come back as -22 before anything touches a device,
   the workspace is 0 where nothing splits, the build remarks show no scratch and no spill.
2. pack_questions / question_windows on hand-written cases, their coverage, and what the attention plan makes of the windows.
3. The entry-point sequence of one pass: one layer sequence per layer, one lm_head GEMM over the choice rows only, one logprob
   launch, a top-k launch exactly when top_k > 0, nothing of the FP8 modes, the cache left alone; score_rows the same.
4. The ValueError cases of the public methods."""
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
from g2vlm_amd.engine import Engine, pack_continuations, pack_questions, question_windows  # noqa: E402
from test_decode_program_cpu import LAYERS, Recorder, filled_cache  # noqa: E402
from test_score_cpu import FP8_CALLS, LAYER, PREFILL_CALLS, ScoreWeights, _names, bare_model  # noqa: E402
from test_kv8_cpu import KV8_CALLS  # noqa: E402

P, I, L64 = C.c_void_p, C.c_int, C.c_int64
NAMES = ("x", "rows", "n", "ld", "k", "out_idx", "out_val", "scratch", "scratch_bytes", "stream")


# ------------------------------------------------------------------------------------------------ 1. the C ABI
@pytest.fixture(scope="module")
def lib():
    from g2vlm_amd import build
    lib = C.CDLL(build.build())
    lib.g2v_topk_rows_bf16.argtypes, lib.g2v_topk_rows_bf16.restype = [P, I, I, L64, I, P, P, P, L64, P], I
    lib.g2v_topk_rows_workspace.argtypes, lib.g2v_topk_rows_workspace.restype = [I, I, I], L64
    return lib


def test_library_exports_and_declares_the_entry_points(lib):
    from g2vlm_amd import build
    hdr = open(os.path.join(ROOT, "include", "g2vlm_hip.h")).read()
    for name in ("g2v_topk_rows_bf16", "g2v_topk_rows_workspace"):
        assert hasattr(lib, name) and name in hip.EXPORTS
    assert re.search(r"\bint g2v_topk_rows_bf16\(", hdr) and re.search(r"\bint64_t g2v_topk_rows_workspace\(", hdr)
    assert re.search(r"#define G2V_TOPK_MAX 32\b", hdr) and hip.TOPK_MAX == 32
    assert "topk.hip" in build.SOURCES and "topk.hip" in build.RESOURCE_AUDIT
    assert list(inspect.signature(hip.topk_rows_bf16).parameters) == ["logits", "k", "out_idx", "out_val", "scratch"]
    decl = re.search(r"\bint g2v_topk_rows_bf16\((.*?)\);", hdr, re.S).group(1)
    assert len(decl.split(",")) == len(hip._SIGS["g2v_topk_rows_bf16"][0]) == len(NAMES)
    decl = re.search(r"\bint64_t g2v_topk_rows_workspace\((.*?)\);", hdr, re.S).group(1)
    assert len(decl.split(",")) == len(hip._SIGS["g2v_topk_rows_workspace"][0]) == 3
    assert "g2v_topk_rows_bf16" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def call(lib, **kw):
    """A valid argument set (no pointer is dereferenced: every call below is refused before any launch), with overrides."""
    a = dict(x=16, rows=3, n=100, ld=100, k=5, out_idx=16, out_val=16, scratch=None, scratch_bytes=0, stream=None)
    a.update(kw)
    return lib.g2v_topk_rows_bf16(*[a[k] for k in NAMES])


@pytest.mark.parametrize("bad", [dict(rows=0), dict(rows=-1), dict(n=0), dict(n=-5), dict(ld=99), dict(ld=0), dict(k=0), dict(k=-1), dict(k=33),
                                 dict(x=None), dict(out_idx=None), dict(x=None, out_val=None), dict(k=33, out_val=None),
                                 dict(rows=0, scratch=16, scratch_bytes=1 << 20)])
def test_argument_errors_return_einval_without_a_device(lib, bad):
    assert call(lib, **bad) == -22


def test_the_workspace_is_only_asked_for_where_rows_are_split(lib):
    ws = lib.g2v_topk_rows_workspace
    assert ws(0, 100, 5) == 0 and ws(3, 0, 5) == 0 and ws(-1, -1, 5) == 0 and ws(3, 151936, 0) == 0 and ws(3, 151936, 33) == 0
    assert ws(1, 8192, 32) == 0 and ws(64, 7, 1) == 0          # one chunk per row: nothing to split
    assert ws(512, 151936, 5) == 0 and ws(4096, 151936, 32) == 0   # the rows fill the chip by themselves
    for rows, S in ((1, 19), (3, 19), (64, 8), (65, 8), (511, 2)):   # min(ceil(512 / rows), 19 chunks) lists of k pairs per row
        for k in (1, 5, 32):
            assert ws(rows, 151936, k) == 4 * (512 + rows * S * 2 * k)
            assert ws(rows, 151936, k) <= 4 * hip.TOPK_WS_WORDS   # the binding's own scratch covers every split launch
    assert ws(1, 8193, 5) == 4 * (512 + 2 * 2 * 5)


@pytest.mark.timeout(1800)
def test_the_kernel_is_spill_free():
    if not os.path.exists(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    from test_fp8_decode_cpu import _remarks
    rows = _remarks("topk.hip")
    assert rows and all("topk_rows_bf16_kernel" in r["name"] for r in rows), [r["name"] for r in rows]
    for r in rows:
        assert int(r["ScratchSize [bytes/lane]"]) == 0, r
        assert int(r["VGPRs Spill"]) == 0, r


# ------------------------------------------------------------------------------------------------ 2. the packing
def test_packing_one_question_with_one_choice_of_one_token():
    ids, pos, layout, tgt = pack_questions([([5], [30], 7, 31, [[99]])])
    assert (ids, pos, layout, tgt) == ([5, 7], [30, 31], ((1, (1,)),), [99])
    assert question_windows(12, layout) == ((0, 1, 0, 12, False), (0, 1, 12, 1, True),
                                            (1, 1, 0, 12, False), (1, 1, 12, 1, False), (1, 1, 13, 1, True))
    assert question_windows(0, layout) == ((0, 1, 0, 1, True), (1, 1, 0, 1, False), (1, 1, 1, 1, True))
    for bad in ([([], [], 7, 31, [[99]])], [([5], [30, 31], 7, 31, [[99]])], [([5], [30], 7, 31, [])], [([5], [30], 7, 31, [[1], []])]):
        with pytest.raises(ValueError):
            pack_questions(bad)


def test_packing_two_questions():
    """Questions of 5 and 3 rows with choices of lengths [2, 1] and [4] over a scene of 100 rows."""
    qs = [([11, 12, 13, 14, 15], [40, 41, 42, 43, 44], 7, 45, [[21, 22], [31]]),
          ([16, 17, 18], [40, 41, 42], 7, 43, [[51, 52, 53, 54]])]
    ids, pos, layout, tgt = pack_questions(qs)
    assert ids == [11, 12, 13, 14, 15, 16, 17, 18] + [7, 21] + [7] + [7, 51, 52, 53]
    assert pos == [40, 41, 42, 43, 44, 40, 41, 42] + [45, 46] + [45] + [43, 44, 45, 46]
    assert layout == ((5, (2, 1)), (3, (4,)))
    assert tgt == [21, 22, 31, 51, 52, 53, 54]
    assert question_windows(100, layout) == (
        (0, 5, 0, 100, False), (0, 5, 100, 5, True),                                  # question 0: the scene, itself
        (5, 3, 0, 100, False), (5, 3, 105, 3, True),                                  # question 1
        (8, 2, 0, 100, False), (8, 2, 100, 5, False), (8, 2, 108, 2, True),           # choice 0 of question 0: scene, question 0, itself
        (10, 1, 0, 100, False), (10, 1, 100, 5, False), (10, 1, 110, 1, True),        # choice 1 of question 0
        (11, 4, 0, 100, False), (11, 4, 105, 3, False), (11, 4, 111, 4, True))        # the choice of question 1: scene, question 1, itself
    # every segment of the tail is what pack_continuations makes of it
    assert (ids[8:11], pos[8:11], tgt[:3]) == tuple(pack_continuations(7, 45, [[21, 22], [31]])[i] for i in (0, 1, 3))


def windows_cover(P, layout, wins):
    Lq = sum(m for m, _ in layout)
    L = Lq + sum(sum(s) for _, s in layout)
    q_cover, k_cover = [0] * L, [0] * L
    for q0, ql, k0, kl, causal in wins:
        for r in range(q0, q0 + ql):
            q_cover[r] += 1
        if causal:
            assert k0 == P + q0 and kl == ql                   # a causal window is a segment over its own rows
            for r in range(k0 - P, k0 - P + kl):
                k_cover[r] += 1
    return q_cover, k_cover, Lq, L


def test_packing_64_questions():
    qs = [(list(range(100 + j, 100 + j + 1 + j % 4)), list(range(9, 9 + 1 + j % 4)), 5, 10 + j % 4,
           [[1000 + j + c] * (1 + (j + c) % 3) for c in range(1 + j % 5)]) for j in range(64)]
    ids, pos, layout, tgt = pack_questions(qs)
    assert len(layout) == 64 and [m for m, _ in layout] == [1 + j % 4 for j in range(64)]
    wins = question_windows(33, layout)
    n_choices = sum(len(s) for _, s in layout)
    assert len(wins) == 2 * 64 + 3 * n_choices
    q_cover, k_cover, Lq, L = windows_cover(33, layout, wins)
    assert len(ids) == len(pos) == L and len(tgt) == L - Lq
    # every question row is in exactly two windows, every choice row in exactly three, every new cache row is the key of exactly
    # one causal window
    assert q_cover == [2] * Lq + [3] * (L - Lq) and k_cover == [1] * L
    a, b, t = 0, Lq, 0
    for j, (q, (m, segs)) in enumerate(zip(qs, layout)):
        assert ids[a:a + m] == q[0] and pos[a:a + m] == q[1]
        for c, n in zip(q[4], segs):
            assert ids[b:b + n] == [5] + c[:-1] and pos[b:b + n] == list(range(q[3], q[3] + n)) and tgt[t:t + n] == c
            mine = [w for w in wins if w[0] == b]
            assert mine == [(b, n, 0, 33, False), (b, n, 33 + a, m, False), (b, n, 33 + b, n, True)]
            b += n
            t += n
        a += m
    # without a scene: one window less per segment
    q0, k0, _, _ = windows_cover(0, layout, question_windows(0, layout))
    assert q0 == [1] * Lq + [2] * (L - Lq) and k0 == [1] * L


def test_the_attention_plan_expresses_these_windows():
    """make_attn_plan on the windows of two questions (5 and 3 rows; choices of 2, 1 and 4) over a 100-row scene: one tile per
    window and one merge per segment and head, over the partial results of its two (question) or three (choice) windows."""
    Hq = 2
    layout = ((5, (2, 1)), (3, (4,)))
    wins = question_windows(100, layout)
    plan = hip.make_attn_plan(wins, Hq, torch.device("cpu"))
    assert plan.n_tiles == len(wins) == 13 and len(plan.phases) == 1 and plan.tile_rows == 128
    for (q0, ql, k0, kl, causal), t in zip(wins, plan.tiles.tolist()):
        assert t[:4] == [q0, ql, k0, kl] and t[5] == q0
        assert t[4] == (0 if causal else hip.NO_CAUSAL)
    assert plan.n_comb == 5 * Hq
    comb = plan.comb.view(-1, 4).tolist()
    first = {0: 0, 5: 2, 8: 4, 10: 7, 11: 10}                 # segment start -> its first descriptor
    assert sorted((c[0], c[1]) for c in comb) == sorted((d, h) for d in first.values() for h in range(Hq))
    want = {0: 2, 2: 2, 4: 3, 7: 3, 10: 3}                     # partial results per merge, at least (the scene window may be cut further)
    assert all(c[3] >= want[c[0]] for c in comb) and sum(c[3] for c in comb) == plan.n_slots


# ------------------------------------------------------------------------------------------------ 3. the program of one pass
@pytest.fixture(scope="module")
def traced():
    """(recorder, engine, plans) with every entry point of the decode step, of the prefill and the top-k replaced by recorders."""
    mp = pytest.MonkeyPatch()
    try:
        w = ScoreWeights(D.TINY["llm"])
        rec = Recorder(mp, w)
        for name in PREFILL_CALLS + KV8_CALLS + ("topk_rows_bf16",):
            mp.setattr(hip, name, rec._wrap(name, getattr(hip, name)))
        rms = hip.rmsnorm

        def rmsnorm(x, w_lo, w_hi, split, eps, out_dtype=torch.bfloat16, out=None):
            if out is None:
                out = torch.empty(x.shape, dtype=out_dtype)
            return rms(x, w_lo, w_hi, split, eps, out_dtype, out)
        mp.setattr(hip, "rmsnorm", rmsnorm)
        mp.setattr(hip, "mrope_table", lambda pos, inv_freq: (rec.calls.append(("mrope_table", {"L": pos.shape[1]})),
                                                              (torch.empty(pos.shape[1], 128), torch.empty(pos.shape[1], 128)))[1])
        plans = []
        mp.setattr(hip, "make_attn_plan", lambda windows, Hq, device, **kw: plans.append((tuple(windows), Hq, kw)) or ("plan", len(plans)))
        yield rec, Engine(w, D.TINY), plans
    finally:
        mp.undo()


def questions_trace(rec, eng, layout, top_k, prefix=6):
    Lc = D.TINY["llm"]
    cache = filled_cache(Lc, prefix, 3)
    before = [(cache.k[i][:prefix].clone(), cache.v[i][:prefix].clone()) for i in range(Lc["layers"])]
    Lq = sum(m for m, _ in layout)
    n = sum(sum(s) for _, s in layout)
    z = lambda k: torch.zeros(k, dtype=torch.int32)  # noqa: E731
    rec.take()
    res = eng.score_questions(cache, prefix, z(Lq + n), torch.zeros((3, Lq + n), dtype=torch.int32), layout, z(n), top_k=top_k)
    assert len(res) == (5 if top_k else 2)
    assert [tuple(t.shape) for t in res[:2]] == [(n,), (n,)] and [t.dtype for t in res[:2]] == [torch.float32, torch.int32]
    if top_k:
        assert [tuple(t.shape) for t in res[2:]] == [(n,), (n, top_k), (n, top_k)]
        assert [t.dtype for t in res[2:]] == [torch.float32, torch.int32, torch.float32]
    assert cache.length == prefix
    for i, (k, v) in enumerate(before):
        assert torch.equal(cache.k[i][:prefix], k) and torch.equal(cache.v[i][:prefix], v)
    return rec.take()


LAYOUTS = [((1, (1,)),), ((5, (2, 1)), (3, (4,))), tuple((1 + j % 3, (2,) * (1 + j % 2)) for j in range(64)), ((40, (31, 9)),)]


@pytest.mark.parametrize("top_k", [0, 1, 5])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_pass_one_lm_head_gemm_over_the_choice_rows(traced, layout, top_k):
    rec, eng, plans = traced
    calls = questions_trace(rec, eng, layout, top_k)
    Lq = sum(m for m, _ in layout)
    n = sum(sum(s) for _, s in layout)
    L = Lq + n
    tail = ["rmsnorm", "linear", "logprob_rows_bf16"] + (["topk_rows_bf16"] if top_k else [])
    assert _names(calls) == ["gather_rows", "mrope_table"] + LAYER * LAYERS + tail
    assert plans[-1][0] == question_windows(6, layout)
    V, H = D.TINY["llm"]["vocab"], D.TINY["llm"]["hidden"]
    (head,) = [c for c in calls if c[0] == "linear"]
    norm = calls[len(calls) - len(tail)]
    assert norm[1]["out"][2:] == ((L, H), "torch.bfloat16")     # the final norm runs over every row ...
    assert head[1]["w"][:2] == ("w", "lm_head") and head[1]["x"][2:] == ((n, H), "torch.bfloat16")   # ... the head over the choices'
    assert head[1]["out"][2:] == ((n, V), "torch.bfloat16")
    (lp,) = [c for c in calls if c[0] == "logprob_rows_bf16"]
    assert lp[1]["logits"][1] == head[1]["out"][1] and lp[1]["targets"][2:] == ((n,), "torch.int32")
    assert lp[1]["out"][2:] == ((n,), "torch.float32") and lp[1]["rank"][2:] == ((n,), "torch.int32")
    assert (lp[1]["lse"] is None) == (top_k == 0)
    if top_k:
        assert lp[1]["lse"][2:] == ((n,), "torch.float32")
        (tk,) = [c for c in calls if c[0] == "topk_rows_bf16"]
        assert tk[1]["logits"][1] == head[1]["out"][1] and tk[1]["k"] == top_k
        assert tk[1]["out_idx"][2:] == ((n, top_k), "torch.int32") and tk[1]["out_val"][2:] == ((n, top_k), "torch.float32")
    lm_head = eng.w["lm_head"].data_ptr()
    for c in calls:
        if c[0] == "gemm_bf16":
            assert all(g["W"].data_ptr() != lm_head for g in c[1]["groups"])
        if c[0] == "qknorm_mrope_cache":
            assert c[1]["split"] == 0 and c[1]["und_rounding"] == 1 and c[1]["kv_rows"][2:] == ((L,), "torch.int32")
    assert not [m for m in _names(calls) if m in FP8_CALLS]


def test_the_fp8_modes_do_not_reach_the_pass(traced):
    rec, eng, _ = traced
    layout = LAYOUTS[1]
    plain = _names(questions_trace(rec, eng, layout, 5))
    eng.decode_weights, eng.decode_kv = "fp8", "fp8"
    try:
        calls = questions_trace(rec, eng, layout, 5)
    finally:
        eng.decode_weights, eng.decode_kv = "bf16", "bf16"
    assert _names(calls) == plain and not [n for n in _names(calls) if n in FP8_CALLS]
    described = repr(calls)
    assert ".w8" not in described and ".ws" not in described and "uint8" not in described


def test_score_rows_adds_lse_and_one_topk_launch_only_when_asked(traced):
    rec, eng, _ = traced
    z = lambda k: torch.zeros(k, dtype=torch.int32)  # noqa: E731

    def run(**kw):
        cache = filled_cache(D.TINY["llm"], 6, 3)
        rec.take()
        res = eng.score_rows(cache, 6, z(8), torch.zeros((3, 8), dtype=torch.int32), [1, 5, 2], z(8), **kw)
        assert cache.length == 6
        return res, rec.take()
    res0, plain = run()
    res00, zero = run(top_k=0)
    shapes = lambda c: {k: (v[2:] if isinstance(v, tuple) and v[:1] == ("buf",) else v) for k, v in c[1].items()}  # noqa: E731
    same = lambda a, b: _names(a) == _names(b) and all(shapes(a[i]) == shapes(b[i]) for i in (-1, -2))  # noqa: E731  (head, logprob)
    assert len(res0) == len(res00) == 2 and same(plain, zero) and "topk_rows_bf16" not in _names(plain)
    assert [c for c in plain if c[0] == "logprob_rows_bf16"][0][1]["lse"] is None
    res5, five = run(top_k=5)
    assert _names(five) == _names(plain) + ["topk_rows_bf16"] and len(res5) == 5
    assert [c for c in five if c[0] == "logprob_rows_bf16"][0][1]["lse"][2:] == ((8,), "torch.float32")
    assert five[-1][1]["k"] == 5 and five[-1][1]["out_idx"][2:] == ((8, 5), "torch.int32")


def test_the_plan_cache_is_shared_with_score_rows(traced):
    rec, eng, plans = traced
    layout = ((2, (1, 1)), (1, (3,)))                          # a shape no other test of this module plans
    built = len(plans)
    for prefix in range(3, 3 + Engine.SCORE_PLANS_KEPT + 5):
        questions_trace(rec, eng, layout, 0, prefix=prefix)
    assert len([k for k in eng._tiles if k in eng._score_plans]) == len(eng._score_plans) == Engine.SCORE_PLANS_KEPT
    assert len(plans) == built + Engine.SCORE_PLANS_KEPT + 5
    heads = D.TINY["llm"]["heads"]
    assert (question_windows(3 + Engine.SCORE_PLANS_KEPT + 4, layout), heads) in eng._tiles
    assert (question_windows(3, layout), heads) not in eng._tiles
    questions_trace(rec, eng, layout, 0, prefix=3 + Engine.SCORE_PLANS_KEPT + 4)    # a kept shape is not rebuilt
    assert len(plans) == built + Engine.SCORE_PLANS_KEPT + 5


def test_score_questions_refuses_what_it_cannot_take(traced):
    rec, eng, _ = traced
    cache = filled_cache(D.TINY["llm"], 4, 0)
    z = lambda k: torch.zeros(k, dtype=torch.int32)  # noqa: E731
    R = Engine.SCORE_MAX_ROWS
    bad = [(), ((1, (1,)),) * 65, ((0, (1,)),), ((1, ()),), ((1, (1,) * 65),), ((1, (2, 0)),), ((1, (1,) * 33),) * 32,
           ((R, (1,)),), ((1, (R,)),), ((R // 2, (R // 2, 1)),)]
    for layout in bad:
        Lq, n = sum(m for m, _ in layout), sum(sum(s) for _, s in layout)
        with pytest.raises(ValueError):
            eng.score_questions(cache, 4, z(Lq + n), torch.zeros((3, Lq + n), dtype=torch.int32), layout, z(n))
    for top_k in (-1, 33):
        with pytest.raises(ValueError):
            eng.score_questions(cache, 4, z(2), torch.zeros((3, 2), dtype=torch.int32), ((1, (1,)),), z(1), top_k=top_k)
        with pytest.raises(ValueError):
            eng.score_rows(cache, 4, z(1), torch.zeros((3, 1), dtype=torch.int32), [1], z(1), top_k=top_k)
    assert cache.length == 4 and not rec.take()
    assert ((1, (1,) * 32),) * 32 and sum(len(s) for _, s in ((1, (1,) * 32),) * 32) == Engine.SCORE_MAX_CHOICES   # 1024 is taken


# ------------------------------------------------------------------------------------------------ 4. the public methods
class Tok:
    eos_token_id = 2

    def __init__(self, table):
        self.table = table

    def encode(self, text, add_special_tokens=False):
        return list(self.table.get(text, [3] * len(text.split())))


def scene_free_model():
    m = bare_model()

    def no_prefill(*a, **kw):
        raise AssertionError("the prefill ran before the arguments were checked")
    m._chat_geometry = no_prefill
    return m


def test_score_questions_value_errors():
    m, V = bare_model(), D.TINY["llm"]["vocab"]
    ti = dict(packed_text_ids=torch.zeros(3, dtype=torch.long))
    q = lambda conts: (ti, None, conts)  # noqa: E731
    R = Engine.SCORE_MAX_ROWS
    for bad in ([], [q([[1]])] * 65, [q([])], [q([[1]] * 65)], [q([[1], []])], [q([[V]])], [q([[-1]])], [q([[1]] * 33)] * 32,
                [q([[1] * (R - 2)])], [q([[1] * 200] * 41)]):
        with pytest.raises(ValueError):
            m.score_questions(None, bad)
    for top_k in (-1, 33):
        with pytest.raises(ValueError):
            m.score_questions(None, [q([[1]])], top_k=top_k)
        with pytest.raises(ValueError):
            m.score_continuations(None, None, [[1]], top_k=top_k)
    sig = inspect.signature(type(m).score_questions).parameters
    assert list(sig) == ["self", "past_key_values", "questions", "top_k"] and sig["top_k"].default == 0
    assert inspect.signature(type(m).score_continuations).parameters["top_k"].default == 0
    assert inspect.signature(type(m).chat_with_recon_choices).parameters["top_k"].default == 0


def test_chat_with_recon_questions_choices_value_errors_come_before_the_prefill():
    m = scene_free_model()
    tok = Tok({"a": [7], "b": [8, 9], "": [], "long": [5] * (Engine.SCORE_MAX_ROWS + 1), "half": [5] * (Engine.SCORE_MAX_ROWS // 2)})
    nt = dict(eos_token_id=2)
    run = lambda prompts, choices, **kw: m.chat_with_recon_questions_choices(tok, nt, None, None, None, prompts, choices, **kw)  # noqa: E731
    bad = [([], ["a"]), (["q"] * 65, ["a"]), (["q"], []), (["q"], ["a"] * 65), (["q"], ["a", ""]), (["q"], ["long"]),
           (["q", "r"], [["a"]]), (["q", "r"], [["a"], []]), (["q", "r"], [["a"], ["a", ""]]), (["q"] * 32, ["a"] * 33),
           (["q", "r"], [["half"], ["half"]])]
    for prompts, choices in bad:
        with pytest.raises(ValueError):
            run(prompts, choices)
    for top_k in (-1, 33):
        with pytest.raises(ValueError):
            run(["q"], ["a"], top_k=top_k)
        with pytest.raises(ValueError):
            m.chat_with_recon_choices(tok, nt, None, None, None, "q", ["a"], top_k=top_k)
    for prompts, choices in ((["q", "r"], ["a", "b"]), (["q", "r"], [["a"], ["b", "a"]])):   # valid arguments do reach the prefill
        with pytest.raises(AssertionError, match="prefill ran"):
            run(prompts, choices)
    sig = inspect.signature(type(m).chat_with_recon_questions_choices).parameters
    assert sig["append_eos"].default is True and sig["normalize"].default is False and sig["top_k"].default == 0
    src = open(os.path.join(ROOT, "inference_chat.py")).read()
    assert "--top-k" in src and "chat_with_recon_questions_choices" in src
