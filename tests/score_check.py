"""Row-by-row check of the scoring passes (Engine.score_rows / score_questions, _score_pass, _score_plan, pack_continuations,
score_windows, pack_questions, question_windows; G2VLM.score_continuations / score_questions / _score_dicts) against the
precise oracle.  Helper, no tests; CPU only.

The numbers of this path are read directly - log-probabilities, ranks, top-k alternatives; no argmax absorbs an error - and
what its glue gets wrong is finite, in bounds and wrong in a few rows: a question window one key short, a choice that sees the
previous question, a causal staircase shifted by one inside a window that starts at k0 > 0, K/V rows counted from the tail,
positions taken from the cache row, every question at question 0's start position, targets or h[first:] off by one row
(DESIGN 6s).

The reference is sequential, not windowed.  For one question (text ids and positions, start token and position) and ONE of
its choices c = [c0 .. c_{n-1}] over a scene of P cache rows, `one_pass` runs ONE causal OracleG2VLM.llm_forward_inference - und
mode, query_lens = [m + n], a NaiveCache of the scene's rows as the engine holds them - over the rows [text ; start, c0 ..
c_{n-2}], then lm_head on the choice rows.  For a causal LM that is what question_windows promises (the scene, the whole
question, causally the choice itself); score_rows is the same with m = 0.  None of score_windows, question_windows or pack_* is
used.  A question's own rows are taken from the pass of its first choice; causality makes them independent of the choice, and
`score` records how far the other choices' passes are from that (tests/test_score_check_cpu.py asserts it).
tests/test_score_check_cpu.py also ties `one_pass` to the sequential path of the existing oracle (forward_cache_update_text,
then generate_text).

Outputs per packed row (the engine's packing: every question's text rows, then every choice's rows): the final-norm row as
lm_head reads it, the new K row and V row of every layer, and for choice rows the logit row.  One verdict
(block_check.verdict / row_errors: not copied) per output kind - `final_norm`, `logits`, `k{i}`, `v{i}` - whose rows are the
packed rows of one case; row classes: first / last row of a question, first / last row of a choice, a row that starts a further
128-row attention tile of its window, the rest.

Reference and its precision (DESIGN 6o's argument, unchanged).  The precise side is fp32 weights and activations with fp64
attention.  Its own rounding is 2^-24 per fp32 operation; over the K <= 8960 terms of the longest dot product (down_proj) a
blocked fp32 sum stays below sqrt(8960) 2^-24 = 2^-17.4 relative; the fp64 softmax over the longest key count used here (the
column-(b) scene of chat_real2_margin: under 1024 keys; the cases: at most 129 + 259 = 388) adds 1024 2^-53 < 2^-43.  The bf16
flow rounds every Linear's input, weight and output to 2^-9 relative; the measured b_r are 2^-9 .. 2^-7.  2^-7 / 2^-17.4 > 2^10:
the reference's own error is more than 2^10 below the noise being compared.

Margin.  M_SCORE is measured on the oracle alone (tests/test_score_check_cpu.py re-measures it and asserts the constants):
the bf16 oracle's passes under legitimate re-orderings of their fp32 sums (VARIANTS: every Linear's K in 2 / 4 / 8 chunks -
decode_step_check.StepOracle's Linear, reused -, attention as an fp32 online softmax over tiles of 32 / 64 / 128 keys, and
attention as the two or three key ranges of the engine's windows, scene | question | self, each reduced on its own and merged
by (max, sum): what the combine pass does).  M_TABLE holds the largest (max e / max b, median e / median b) per re-ordering
over every case and output kind, M_SCORE = SLACK x the largest of all.  Nothing measured on the engine enters it.

FAULTS: the bf16 oracle's scoring with one named glue fault planted.  MISSES: the ones no check flags, each at most one
rounding by construction.  Integers and bits are not under the margin: `exact_scores` holds log-probabilities, logsumexp, ranks
and top-k entries to the logit rows they were computed from.
"""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import block_check as B  # noqa: E402
import decode_step_check as S  # noqa: E402
from block_check import SLACK, row_errors, verdict  # noqa: E402,F401
from decode_step_check import LM_HEAD, StepOracle, synth_rows, touched_rows  # noqa: E402,F401
from oracle.g2vlm_oracle import NaiveCache, OracleG2VLM, varlen_attention, vit_patchify  # noqa: E402

# largest (max e / max b, median e / median b) of each re-ordering over every case of CASES and every output kind, measured by
# tests/test_score_check_cpu.py::test_the_margin_reproduces on the oracle alone
M_TABLE = {
    "k2": (1.077, 1.036),
    "k4": (1.045, 1.027),
    "k8": (1.039, 1.040),
    "t32": (1.059, 1.011),
    "t64": (1.028, 1.011),
    "t128": (1.028, 1.011),
    "w": (1.028, 1.016),
}
M_SCORE = 1.346
SEED = 53
D_6H = 3.14e-2                   # how far the eager batch-1 decode fed the reference's ids is from the reference
E2E_ALLOWANCE = 2 * D_6H + 1e-3  # what tests/test_score_e2e_gpu.py and test_score_questions_e2e_gpu.py allow a greedy token

# column (b) of DESIGN 6s as measured by tests/test_score_check_cpu.py: the largest |lp - clean lp| over the 71 reference tokens of
# chat_real2_margin with the fault planted in the bf16 oracle's three-question scoring
COLUMN_B = {
    "question_window_one_short": 3.66e-2, "choice_misses_question": 2.46, "choice_sees_previous_question": 2.07e-1,
    "choice_sees_previous_choice": 2.69e-1, "prefix_last_key_dropped": 1.19e-1, "prefix_one_long": 1.58e-1,
    "causal_excludes_self": 7.47e-2, "causal_sees_next": 8.11e-2, "kv_rows_from_tail": 7.80e-1, "pos_is_cache_row": 1.03,
    "start_pos_of_question_0": 9.62e-1, "start_token_dropped": 61.5, "targets_shifted_one": 89.3, "first_row_off_by_one": 89.3,
    "wrong_layer_gamma": 3.14e-1, "und_rounding_flipped": 4.05e-2,
}

VARIANTS = {"k2": dict(k_chunks=2), "k4": dict(k_chunks=4), "k8": dict(k_chunks=8),
            "t32": dict(tile=32), "t64": dict(tile=64), "t128": dict(tile=128), "w": dict(ranges=True)}

# fault -> what a case must have for the fault to be planted in it (fault_applies).  One key among n at unit-rms keys and O(1)
# scores carries about 1 / n of the softmax mass: at n > 256 = 2^8 a key too few or too many is under the bf16 half-ulp 2^-9 of
# the values it is added to (measured there at 4095 keys: 1.03 .. 1.11), so every fault that adds or removes keys of a
# window ("keys") is planted only where the longest row of the case sees P + m + n <= 256 keys.
FAULTS = {
    "question_window_one_short": "keys question",     # a choice's window onto its question ends one key early
    "choice_misses_question": "keys question",        # a choice has no window onto its question
    "choice_sees_previous_question": "keys Q2",       # P + a_j taken from question j - 1 (question j's length)
    "choice_sees_previous_choice": "keys C2",         # a choice's own window starts at the previous choice's first row
    "prefix_last_key_dropped": "keys P1",             # the scene window (0, P - 1)
    "prefix_one_long": "keys P1",                     # the scene window (0, P + 1): reads cache row P, packed row 0's K/V
    "causal_excludes_self": "keys P1",                # key - k0 <= row - q0 - 1
    "causal_sees_next": "keys W2",                    # key - k0 <= row - q0 + 1 (inside the window)
    "kv_rows_from_tail": "L2",                        # row r's K/V written to cache row P + L - 1 - r
    "pos_is_cache_row": "any",                        # row r rotated at P + r
    "start_pos_of_question_0": "M2",                  # every question's choices start at question 0's start position
    "start_token_dropped": "any",                     # rows [c0 ..] where [start, c0 ..] is meant
    "targets_shifted_one": "T2",                      # row r scored against row r + 1's target
    "first_row_off_by_one": "question",               # lm_head over h[first - 1:-1]
    "wrong_layer_gamma": "depth2",                    # layer i >= 1 reads layer 0's input / post-attention layernorm gamma
    "und_rounding_flipped": "any",                    # q / k-norm's rounding flag inverted
}
# Faults no check flags at M_SCORE, with the largest ratio over their cases.  At most one rounding by construction:
#   und_rounding_flipped   und mode rounds the normalised q / k to bf16 before the gamma, the flipped flag does not: the two
#                          differ by at most half a bf16 ulp per element BEFORE q and k are rounded to bf16 anyway after the
#                          rope, i.e. by at most one ulp of values every clean run rounds at the same place.
MISSES = {"und_rounding_flipped": 1.31}
_ATTN = ("question_window_one_short", "choice_misses_question", "choice_sees_previous_question", "choice_sees_previous_choice",
         "prefix_last_key_dropped", "prefix_one_long", "causal_excludes_self", "causal_sees_next", "kv_rows_from_tail")
# faults that need the clean bf16 pass's packed K / V rows: what the wrong window finds in the cache.  The rows of another
# segment are taken from the CLEAN pass: a layer-1 row of that segment under the same fault would differ a little, which
# changes nothing in what is being shown (rows that are not the window's own).
_NEEDS_PACKED = ("choice_sees_previous_question", "choice_sees_previous_choice", "prefix_one_long", "kv_rows_from_tail")


# ------------------------------------------------------------------------------------------------ the cases
def _rows(P, segs, dims="tiny", top_k=0, cap="larger", exact_only=False):
    return dict(kind="rows", dims=dims, P=P, layout=((0, tuple(segs)),), top_k=top_k, cap=cap, exact_only=exact_only)


def _qs(P, layout, dims="tiny", top_k=0, cap="larger"):
    return dict(kind="questions", dims=dims, P=P, layout=tuple((m, tuple(s)) for m, s in layout), top_k=top_k, cap=cap, exact_only=False)


MIXED64 = tuple(1 + (5 * i + i // 7) % 3 for i in range(64))       # 64 lengths 1 .. 3
CASES = [
    # score_rows.  P: 0 (no prefix window), 1, around the 64-key tile and the 128-row tile; segment lengths 1, 2 and around both
    # tiles (a one-row causal window; segments that end before, on and after a 128-row tile); 1, 2, 3 and 64 segments; L <= 64 and
    # L = 65 (lm_head on the skinny and on a tiled form); top_k 0 / 5 / 32; capacity exactly P, exactly P + L, larger
    _rows(0, (3,), cap="exact"),
    _rows(1, (1,), top_k=5),
    _rows(63, (2, 63), cap="fit"),
    _rows(64, (64,), top_k=32),
    _rows(65, (65,), cap="exact", top_k=5),
    _rows(127, (127, 1)),
    _rows(128, (128, 2), top_k=5, cap="fit"),
    _rows(129, (129, 130, 1), cap="exact"),
    _rows(5, MIXED64, top_k=32),
    _rows(65, (2, 65), dims="real", top_k=5),
    _rows(700, (3, 5), top_k=5, exact_only=True),
    # score_questions.  1, 2, 3 and 64 questions; question lengths 1, 2, 64, 65, differing between questions (P + a_j != P + a_0
    # and the start positions differ); 1 .. 4 choices per question and one question with 64; Lq odd and even
    _qs(65, ((1, (1,)),), top_k=5, cap="exact"),
    _qs(63, ((2, (1, 2)), (65, (3,))), cap="fit"),                              # Lq = 67
    _qs(1, ((1, (2, 1)), (65, (1, 3, 2))), top_k=32),                           # Lq = 66
    _qs(64, ((64, (2, 1, 3, 1)), (1, (1,)), (2, (2, 2))), top_k=5),             # Lq = 67, 4 choices
    _qs(127, ((3, (3, 3, 2)), (2, (3, 3, 2)), (2, (3, 2))), top_k=5),           # the e2e tests' layout of choices: 3, 3 and 2
    _qs(63, tuple((1, (1,)) for _ in range(64))),                               # 64 one-row questions, one one-token choice each
    _qs(2, ((2, MIXED64), (3, (2,))), cap="fit"),                               # one question with 64 choices
    _qs(65, ((3, (2, 1)), (5, (3,))), dims="real", top_k=5),
]


def case_id(c):
    lay = "_".join(f"{m}q" + "+".join(str(n) for n in segs) if len(segs) <= 4 else f"{m}q{len(segs)}x" for m, segs in c["layout"]) \
        if len(c["layout"]) <= 3 else f"{len(c['layout'])}questions"
    return f"{c['kind']}_P{c['P']}_{lay}_{c['dims']}_k{c['top_k']}_{c['cap']}"


def dims_of(case):
    return S.dims_of(case)


def sizes(case):
    """(Lq, L, [a_j: first packed row of question j], [(j, c, b, n): the choices in packed order with their first packed row])."""
    a, starts = 0, []
    for m, _ in case["layout"]:
        starts.append(a)
        a += m
    Lq, b, chs = a, a, []
    for j, (m, segs) in enumerate(case["layout"]):
        for c, n in enumerate(segs):
            chs.append((j, c, b, n))
            b += n
    return Lq, b, starts, chs


def max_keys(case):
    """The largest key count any row of the case attends to."""
    return case["P"] + max(m + max(segs) for m, segs in case["layout"])


def capacity(case):
    """Rows of the scene's KVCache before the pass."""
    L = sizes(case)[1]
    return {"exact": max(case["P"], 1), "fit": case["P"] + L, "larger": case["P"] + L + 37}[case["cap"]]


def rope0(case):
    """The mRoPE position of a question's first row (of the start token for score_rows), never the cache row of any packed row.
    Wherever the scene is longer than the longest question of the case, every start position rope0 + m_j is below P, as it is
    after images (the position runs behind the cache row): P - 70 from P = 100 on, half of the room P - 1 - max m below that.
    A question as long as the scene or longer cannot start below P: those cases (and P = 0) start far behind the cache."""
    P, longest = case["P"], max(m for m, _ in case["layout"])
    if P >= 100:
        return P - 70
    return (P - 1 - longest) // 2 if longest < P else P + 1000


def tokens(case):
    """[(text ids, text positions, start token, start position, continuations)] per question: pack_questions' input."""
    V = dims_of(case)["llm"]["vocab"]
    out = []
    for j, (m, segs) in enumerate(case["layout"]):
        text = [(13 + 7 * j + 3 * i) % V for i in range(m)]
        conts = [[(29 + 11 * j + 5 * c + 3 * i * (1 + c % 2)) % (V - 64) for i in range(n)] for c, n in enumerate(segs)]
        out.append((text, list(range(rope0(case), rope0(case) + m)), V - 1 - j, rope0(case) + m, conts))    # the start token: no choice id
    return out


def scene_rows(case):
    """(K, V) bf16 [layers, capacity or P + L + 37, Hkv, 128]: rows [0, P) are the scene, the rest the finite stale rows the GPU
    module fills the cache with behind it (decode_step_check.synth_rows: the cache's own scale)."""
    n = case["P"] + sizes(case)[1] + 37
    return synth_rows(case, SEED, n, "k"), synth_rows(case, SEED, n, "v")


def fault_applies(fault, case):
    if case["exact_only"]:
        return False
    Lq, L, starts, chs = sizes(case)
    lay = case["layout"]
    for need in FAULTS[fault].split():
        ok = {"any": True, "keys": max_keys(case) <= 256, "question": case["kind"] == "questions", "Q2": len(lay) >= 2,
              "C2": len(chs) >= 2, "P1": case["P"] >= 1, "W2": max(max(m, max(s)) for m, s in lay) >= 2, "L2": L >= 2,
              "M2": any(m != lay[0][0] for m, _ in lay), "T2": L - Lq >= 2, "depth2": case["dims"] == "tiny"}[need]
        if not ok:
            return False
    return True


def fault_rows(fault, case):
    """The packed rows a fault may put an offender in (None: anywhere), by derivation: a fault of a choice's windows, of its
    start position or of its input rows leaves every question row as it was, and moves only the choices it names."""
    Lq, L, starts, chs = sizes(case)
    lay = case["layout"]
    rows = lambda pick: {r for j, c, b, n in chs if pick(j, c, b) for r in range(b, b + n)}     # noqa: E731
    if fault in ("question_window_one_short", "choice_misses_question", "start_token_dropped", "first_row_off_by_one"):
        return rows(lambda j, c, b: True) if case["kind"] == "questions" else None
    if fault == "choice_sees_previous_question":
        return rows(lambda j, c, b: j >= 1)
    if fault == "choice_sees_previous_choice":
        return rows(lambda j, c, b: b > Lq)
    if fault == "start_pos_of_question_0":
        return rows(lambda j, c, b: lay[j][0] != lay[0][0])
    return None


# ------------------------------------------------------------------------------------------------ the oracle
def ranges_attention(q, k, v, bounds, causal_offset):
    """q [H, Lq, d], k / v [H, Lk, d] fp32 under the mask key <= row + causal_offset: the keys in the contiguous ranges
    `bounds` = [(s, e)], each reduced on its own to (max, sum, partial output), the partials merged by their (max, sum) - the
    attention plan's combine pass.  A range a row sees nothing of contributes (-inf, 0)."""
    Lq, d = q.shape[1], q.shape[-1]
    row = torch.arange(Lq).view(-1, 1)
    ms, ls, os_ = [], [], []
    for s, e in bounds:
        if e <= s:
            continue
        sc = torch.matmul(q, k[:, s:e].transpose(1, 2)) / math.sqrt(d)
        sc = sc.masked_fill(torch.arange(s, e).view(1, -1) > row + causal_offset, float("-inf"))
        m = sc.max(-1, keepdim=True).values
        p = torch.exp(sc - torch.where(torch.isinf(m), torch.zeros_like(m), m))
        ms.append(m); ls.append(p.sum(-1, keepdim=True)); os_.append(torch.matmul(p, v[:, s:e]))
    top = torch.stack(ms).max(0).values
    l = sum(l_ * torch.exp(m - top) for l_, m in zip(ls, ms))
    o = sum(o_ * torch.exp(m - top) for o_, m in zip(os_, ms))
    return o / l


def masked_attention(q, k, v, mask):
    """q [Lq, Hq, d], k / v [Lk, Hkv, d], mask [Lq, Lk] (True: seen): varlen_attention's fp32 softmax under any mask."""
    rep = q.shape[1] // k.shape[1]
    qi = q.float().transpose(0, 1)
    ki = k.float().transpose(0, 1).repeat_interleave(rep, dim=0)
    vi = v.float().transpose(0, 1).repeat_interleave(rep, dim=0)
    s = torch.matmul(qi, ki.transpose(1, 2)) / math.sqrt(q.shape[-1])
    s = s.masked_fill(~mask, float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), vi).transpose(0, 1).to(q.dtype)


class ScoreOracle(StepOracle):
    """The oracle of one causal pass over [question ; start, choice]: precise, bf16, the bf16 one with its fp32 sums re-ordered
    (k_chunks: StepOracle's Linear; tile / ranges: the attention) or with ONE glue fault planted.  `ctx` (set by one_pass):
    P, m, n, and for a fault what the wrong window finds in the cache."""

    def __init__(self, sd, dims, precise=False, k_chunks=None, tile=None, ranges=False, fault=None):
        assert fault is None or fault in FAULTS
        inherited = {"wrong_layer_gamma": "wrong_layer_ln", "und_rounding_flipped": "und_rounding_flipped"}.get(fault)
        super().__init__(sd, dims, precise=precise, k_chunks=k_chunks, tile=tile, fault=inherited)
        self.fault, self.ranges, self.ctx = fault, ranges, None

    def varlen(self, q, k, v, cu_q, cu_k, causal):
        c, f, i = self.ctx, self.fault, self.layer
        P, m, n = c["P"], c["m"], c["n"]
        Lq, Lk = q.shape[0], k.shape[0]
        assert causal and Lq == m + n and Lk == P + Lq
        if f not in _ATTN:
            if self.tile is None and not self.ranges:
                return varlen_attention(q, k, v, cu_q, cu_k, causal, precise=self.precise)
            rep = q.shape[1] // k.shape[1]
            qi = q.float().transpose(0, 1)
            ki = k.float().transpose(0, 1).repeat_interleave(rep, dim=0)
            vi = v.float().transpose(0, 1).repeat_interleave(rep, dim=0)
            if self.tile:
                o = B.online_softmax_attention(qi, ki, vi, self.tile, P)
            else:
                o = ranges_attention(qi, ki, vi, [(0, P), (P, P + m), (P + m, Lk)], P)
            return o.transpose(0, 1).to(q.dtype)
        row, col = torch.arange(Lq).view(-1, 1), torch.arange(Lk).view(1, -1)
        mask = col <= row + P                                # the clean pass: the scene, and causally the rows themselves
        choice = (row >= m).expand(Lq, 1)
        ak, av, extra = k, v, None
        if f == "question_window_one_short":
            mask = mask & ~(choice & (col == P + m - 1))
        elif f == "choice_misses_question":
            mask = mask & ~(choice & (col >= P) & (col < P + m))
        elif f == "choice_sees_previous_question":           # the m rows from P + a_{j-1} on, and not its own question
            mask = mask & ~(choice & (col >= P) & (col < P + m))
            extra, seen = c["wrong_question"], choice
        elif f == "choice_sees_previous_choice":
            extra, seen = c["previous_choice"], choice
        elif f == "prefix_last_key_dropped":
            mask = mask & (col != P - 1)
        elif f == "prefix_one_long":
            extra, seen = c["row_0"], torch.ones((Lq, 1), dtype=torch.bool)
        elif f == "causal_excludes_self":
            mask = mask & (col != row + P)
        elif f == "causal_sees_next":                        # inside the window: the question's last row has no next key
            mask = mask | ((col == row + P + 1) & (row != m - 1))
        elif f == "kv_rows_from_tail":                       # the windows' cache rows hold other packed rows
            ak, av = k.clone(), v.clone()
            ak[P:], av[P:] = c["found"][0][i].to(k.dtype), c["found"][1][i].to(v.dtype)
        if extra is not None and extra[0][i].shape[0]:
            ek, ev = extra[0][i].to(k.dtype), extra[1][i].to(v.dtype)
            ak, av = torch.cat([ak, ek]), torch.cat([av, ev])
            mask = torch.cat([mask, seen.expand(Lq, ek.shape[0])], dim=1)
        return masked_attention(q, ak, av, mask)


def one_pass(orc, K, V, text_ids, text_pos, start, start_pos, cont, ctx=None):
    """ONE causal pass of `orc` over [text ; start, c0 .. c_{n-2}] behind the scene rows K / V (per layer [P, Hkv, 128]).
    Returns dict(final_norm [m + n, H], logits [n, vocab], k / v: per layer [m + n, Hkv * 128]), fp32."""
    m, n, P = len(text_ids), len(cont), K[0].shape[0]
    f = orc.fault
    ids = list(text_ids) + ([int(t) for t in cont] if f == "start_token_dropped" else [int(start)] + [int(t) for t in cont[:-1]])
    pos = list(text_pos) + list(range(int(start_pos), int(start_pos) + n))
    if ctx and "pos" in ctx:
        pos = ctx["pos"]
    Ly = orc.num_layers
    cache = NaiveCache(Ly)
    if P:
        for i in range(Ly):
            cache.key_cache[i], cache.value_cache[i] = K[i].to(orc.cd), V[i].to(orc.cd)
    orc.ctx = dict(ctx or {}, P=P, m=m, n=n)
    x = orc.embed_tokens(torch.tensor(ids, dtype=torch.long))
    h = orc.llm_forward_inference(x, torch.tensor([m + n], dtype=torch.int), torch.tensor(pos, dtype=torch.long).expand(3, -1),
                                  torch.arange(P, P + m + n), cache, torch.tensor([P], dtype=torch.int), torch.arange(P), True, "und")
    h = h.to(orc.cd)                                         # what lm_head reads (the engine's bf16 final norm)
    logits = orc.lin(h[m:], LM_HEAD, bias=False)
    orc.ctx = None
    return dict(final_norm=h.float(), logits=logits.float(),
                k=[cache.key_cache[i][P:].flatten(1).float() for i in range(Ly)],
                v=[cache.value_cache[i][P:].flatten(1).float() for i in range(Ly)])


_SCORE_ORACLES = {}


def oracle(which, mode):
    """Cached oracles over block_check's synthetic weights: mode precise / bf16 / a VARIANTS name / a FAULTS name."""
    key = (which, mode)
    if key not in _SCORE_ORACLES:
        sd, dims = B.state_dict(which)
        kw = dict(precise=True) if mode == "precise" else {} if mode == "bf16" else VARIANTS[mode] if mode in VARIANTS else dict(fault=mode)
        _SCORE_ORACLES[key] = ScoreOracle(sd, dims, **kw)
    return _SCORE_ORACLES[key]


def logprobs_of(logits, targets):
    """(log-probability, logsumexp fp32, rank int32) of fp32 logit rows holding bf16 values: fp64, rounded to the output
    format; ranks by tests/test_logprob_gpu.py's rule."""
    x = logits.double()
    t = torch.as_tensor(targets, dtype=torch.long)
    lse = torch.logsumexp(x, dim=1)
    xt = x.gather(1, t[:, None])[:, 0]
    idx = torch.arange(x.shape[1])[None, :]
    rank = ((x > xt[:, None]) | ((x == xt[:, None]) & (idx < t[:, None]))).sum(dim=1)
    return (xt - lse).float(), lse.float(), rank.int()


def score(orc, case, questions=None, scene=None, clean=None, only=None):
    """The scoring pass of a case on `orc`, in the engine's packing.  questions: `tokens(case)`; scene: (K, V) per layer
    [>= P, ..]; clean: the clean bf16 result (the faults of _NEEDS_PACKED).  Returns {final_norm [L, H], logits [L - Lq, vocab],
    k{i} / v{i} [L, Hkv * 128], targets, logprobs, lse, ranks, choice_dependence}: choice_dependence is the largest |difference|
    between a question's rows as the pass of its first choice gives them and as the passes of its other choices do.
    only: a set of (question, choice) - those passes alone, each in its place in the packing; returns their logprobs, lse, ranks."""
    questions = questions if questions is not None else tokens(case)
    K, V = scene if scene is not None else scene_rows(case)
    P, f, Ly = case["P"], orc.fault, orc.num_layers
    K, V = [K[i][:P] for i in range(Ly)], [V[i][:P] for i in range(Ly)]
    Lq, L, starts, chs = sizes(case)
    Hkv = orc.dims["llm"]["kv_heads"]
    packed = None
    if f in _NEEDS_PACKED:
        packed = tuple([clean[f"{t}{i}"].view(L, Hkv, 128) for i in range(Ly)] for t in ("k", "v"))
    fn = [None] * L
    ks, vs = [[None] * L for _ in range(Ly)], [[None] * L for _ in range(Ly)]
    logit_rows, dep = [], 0.0
    prev = None
    for j, c, b, n in chs:
        if only is not None and (j, c) not in only:
            prev = (b, n)
            continue
        text, text_pos, start, start_pos, conts = questions[j]
        m, a = len(text), starts[j]
        ctx = {}
        if f == "pos_is_cache_row":
            ctx["pos"] = list(range(P + a, P + a + m)) + list(range(P + b, P + b + n))
        if f == "start_pos_of_question_0":
            start_pos = questions[0][3]
        if packed is not None:
            pick = lambda lo, hi: tuple([t[i][lo:hi] for i in range(Ly)] for t in packed)     # noqa: E731
            a_wrong = starts[j - 1] if j else a               # question 0 has no predecessor: its window is right
            ctx["wrong_question"] = pick(a_wrong, a_wrong + m)
            ctx["previous_choice"] = pick(prev[0], prev[0] + prev[1]) if prev else pick(0, 0)
            ctx["row_0"] = pick(0, 1)
            at = torch.tensor([L - 1 - r for r in list(range(a, a + m)) + list(range(b, b + n))], dtype=torch.long)
            ctx["found"] = tuple([t[i][at] for i in range(Ly)] for t in packed)
        o = one_pass(orc, K, V, text, text_pos, start, start_pos, conts[c], ctx)
        for r in range(m):
            if fn[a + r] is None:
                fn[a + r] = o["final_norm"][r]
                for i in range(Ly):
                    ks[i][a + r], vs[i][a + r] = o["k"][i][r], o["v"][i][r]
            else:
                dep = max([dep, float((fn[a + r] - o["final_norm"][r]).abs().max())]
                          + [float((ks[i][a + r] - o["k"][i][r]).abs().max()) for i in range(Ly)]
                          + [float((vs[i][a + r] - o["v"][i][r]).abs().max()) for i in range(Ly)])
        for r in range(n):
            fn[b + r] = o["final_norm"][m + r]
            for i in range(Ly):
                ks[i][b + r], vs[i][b + r] = o["k"][i][m + r], o["v"][i][m + r]
        logit_rows.append(o["logits"])
        prev = (b, n)
    if only is not None:
        lp, lse, rank = logprobs_of(torch.cat(logit_rows), [int(t) for j, c, b, n in chs if (j, c) in only for t in questions[j][4][c]])
        return dict(logprobs=lp, lse=lse, ranks=rank)
    out = dict(final_norm=torch.stack(fn), logits=torch.cat(logit_rows))
    for i in range(Ly):
        out[f"k{i}"], out[f"v{i}"] = torch.stack(ks[i]), torch.stack(vs[i])
    if f == "kv_rows_from_tail":                             # ... and the cache holds them in that order
        for i in range(Ly):
            out[f"k{i}"], out[f"v{i}"] = out[f"k{i}"].flip(0), out[f"v{i}"].flip(0)
    if f == "first_row_off_by_one":                          # lm_head over the final-norm rows [Lq - 1, L - 1)
        out["logits"] = orc.lin(out["final_norm"][Lq - 1:L - 1].to(orc.cd), LM_HEAD, bias=False).float()
    targets = [int(t) for j, c, b, n in chs for t in questions[j][4][c]]
    used = targets[1:] + targets[-1:] if f == "targets_shifted_one" else targets
    out["targets"] = torch.tensor(targets, dtype=torch.int32)
    out["logprobs"], out["lse"], out["ranks"] = logprobs_of(out["logits"], used)
    out["choice_dependence"] = dep
    return out


KINDS = lambda Ly: ["final_norm", "logits"] + [f"{t}{i}" for i in range(Ly) for t in ("k", "v")]     # noqa: E731


def row_classes(case, kind):
    """{class: rows of output `kind`} (logits: the choice rows only, row r is packed row Lq + r)."""
    Lq, L, starts, chs = sizes(case)
    cls = {"question_edge": [], "choice_edge": [], "tile_start": []}
    for a, (m, _) in zip(starts, case["layout"]):
        if m:
            cls["question_edge"] += [a, a + m - 1]
            cls["tile_start"] += list(range(a + 128, a + m, 128))
    for _, _, b, n in chs:
        cls["choice_edge"] += [b, b + n - 1]
        cls["tile_start"] += list(range(b + 128, b + n, 128))
    if kind == "logits":
        cls = {c: [r - Lq for r in rows if r >= Lq] for c, rows in cls.items()}
    return cls


_REF = {}


def reference(case):
    """(precise result, bf16 result) of a case on the synthetic scene, computed once and shared."""
    key = case_id(case)
    if key not in _REF:
        _REF[key] = (score(oracle(case["dims"], "precise"), case), score(oracle(case["dims"], "bf16"), case))
    return _REF[key]


def run(case, mode):
    """The case on the oracle `mode` (a re-ordering or a fault)."""
    return score(oracle(case["dims"], mode), case, clean=reference(case)[1] if mode in _NEEDS_PACKED else None)


def judge(case, got, ref2, M, what="engine"):
    """verdict on every output kind.  got: {kind: [rows, C]}.  Returns (ok, {kind: verdict}, message)."""
    prec, ref = ref2
    Lq = sizes(case)[0]
    res, msgs, ok = {}, [], True
    for name in KINDS(dims_of(case)["llm"]["layers"]):
        v = verdict(got[name].float().cpu(), ref[name], prec[name], None, row_classes(case, name), M)
        res[name] = v
        if not v["ok"]:
            ok = False
            off = Lq if name == "logits" else 0
            msgs.append(B.explain(f"{case_id(case)} {name} ({what})", v, M) + "; packed rows: " + ", ".join(str(r + off) for r, _, _ in v["offenders"][:8]))
    return ok, res, "\n".join(msgs)


def offenders(case, res):
    """The packed rows any verdict of `res` names."""
    Lq = sizes(case)[0]
    return {r + (Lq if name == "logits" else 0) for name, v in res.items() for r, _, _ in v["offenders"]}


def worst(res):
    return max(v["ratio_max"] for v in res.values()), max(v["ratio_med"] for v in res.values())


# ------------------------------------------------------------------------------------------------ the exact checks
def exact_scores(logits, targets, logprobs, ranks, lse=None, top_ids=None, top_vals=None, top_logprobs=None):
    """Log-probabilities, logsumexp, ranks and top-k entries against the logit rows THEY were computed from (host tensors; logits
    bf16 or fp32 holding bf16 values).  logprobs / lse: fp64, within tests/test_logprob_gpu.py's bound 1e-4 + 2^-22 |x_t - max|;
    ranks: exact; top_ids and the bits of top_vals: tests/test_topk_gpu.py's stable descending sort of the keys;
    top_logprobs == top_vals - lse in fp32, to the bit.  Returns the list of what failed (empty: all hold)."""
    import test_logprob_gpu as LP
    import test_topk_gpu as TK
    x = logits.detach().cpu().to(torch.bfloat16)
    assert torch.equal(x.float(), logits.detach().cpu().float()), "the logit rows are bf16 values"
    t = torch.as_tensor(targets).detach().cpu().int()
    want_lp, want_lse, want_rank, gap = LP.reference(x, t)
    bound = 1e-4 + 2.0 ** -22 * gap.abs()
    bad = []
    if not torch.equal(torch.as_tensor(ranks).cpu().int(), want_rank):
        rows = (torch.as_tensor(ranks).cpu().int() != want_rank).nonzero().flatten().tolist()
        bad.append(f"ranks differ in rows {rows[:8]}")
    for name, got, want in (("logprobs", logprobs, want_lp), ("lse", lse, want_lse)):
        if got is None:
            continue
        err = (got.detach().cpu().double() - want.float().double()).abs()
        if not bool((err <= bound).all()):
            rows = (err > bound).nonzero().flatten().tolist()
            bad.append(f"{name} off by up to {float(err.max()):.3e} (bound {float(bound.min()):.1e}) in rows {rows[:8]}")
    if top_ids is not None:
        k = top_ids.shape[1]
        want_idx, want_bits = TK.reference(x, k)
        if not torch.equal(top_ids.cpu().int(), want_idx):
            bad.append("top_ids differ from the stable key sort")
        if not torch.equal(top_vals.detach().cpu().float().view(torch.int32), want_bits):
            bad.append("top values differ in bits from the selected logits")
        if top_logprobs is not None and not torch.equal(top_logprobs.cpu().view(torch.int32),
                                                        (top_vals.cpu().float() - lse.cpu().float()[:, None]).view(torch.int32)):
            bad.append("top_logprobs != top values - lse in fp32")
    return bad


def check_dicts(dicts, res, seg_lens):
    """G2VLM._score_dicts' contract: dict s of `dicts` is the slice [off_s, off_s + n_s) of the pass's tensors `res` = (logprobs,
    ranks[, lse, top ids, top values]), bit for bit; total is the fp64 sum of its logprobs; top_logprobs = top values - lse in
    fp32.  Returns the list of what failed."""
    res = [t.detach().cpu() for t in res]
    bits = lambda t: t.contiguous().view(torch.int32)        # noqa: E731
    bad, off = [], 0
    if len(dicts) != len(seg_lens):
        return [f"{len(dicts)} dicts for {len(seg_lens)} segments"]
    for s, (d, n) in enumerate(zip(dicts, seg_lens)):
        want = dict(logprobs=res[0][off:off + n], ranks=res[1][off:off + n])
        if len(res) > 2:
            want.update(top_ids=res[3][off:off + n], top_logprobs=res[4][off:off + n] - res[2][off:off + n, None])
        if set(d) - {"ids"} != set(want) | {"total"}:
            bad.append(f"segment {s}: keys {sorted(d)}")
            continue
        for k, w in want.items():
            if d[k].shape != w.shape or d[k].dtype != w.dtype or not torch.equal(bits(d[k]), bits(w)):
                bad.append(f"segment {s}: {k} is not rows [{off}, {off + n}) of the pass")
        if d["total"] != float(want["logprobs"].double().sum()):
            bad.append(f"segment {s}: total {d['total']} is not the fp64 sum of its logprobs")
        off += n
    return bad


# ------------------------------------------------------------------------------------------------ column (b)
_MARGIN = {}


def margin_scene(golden_dir):
    """chat_real2_margin as the e2e scoring tests use it, on the bf16 oracle: the scene's cache (system prompt, views, images -
    no question), the three questions of tests/test_score_questions_e2e_gpu.py behind it and their 3, 3 and 2 choices (the first
    question's own greedy token stands in as its reference id: the layout is what matters)."""
    if "scene" not in _MARGIN:
        from safetensors.torch import load_file
        from oracle import synth
        with open(os.path.join(golden_dir, "chat_real2_margin.json")) as fh:
            meta = json.load(fh)
        ref = [int(t) for t in load_file(os.path.join(golden_dir, "chat_real2_margin.safetensors"))["ref.ids"].tolist()]
        dims = meta["dims"]
        sd = synth.peaked_lm_head(synth.synth_state_dict(dims, seed=meta["seed"]), meta["head_sigma"], meta["head_seed"])
        tok = synth.FakeTokenizer(dims["llm"]["vocab"])
        nt = tok.new_token_ids
        imgs = synth.synth_images(meta["n"], meta["h"], meta["w"], meta["seed"])
        orc = OracleG2VLM(sd, dims)
        cache = NaiveCache(orc.num_layers)
        sys_p = "<|im_start|>system\nYou are a helpful assistant.<|im_end|>\n<|im_start|>user\n"
        gi, lens, rope = orc.prepare_prompts([0], [0], [sys_p], tok, nt)
        orc.forward_cache_update_text(cache, **gi)
        gi, lens, rope = orc.prepare_dino_images(lens, rope, imgs, nt)
        orc.forward_cache_update_dino(cache, gi)
        for i in range(meta["n"]):
            gen = torch.Generator(); gen.manual_seed(1234 + i)
            pv, thw = vit_patchify(torch.randn((1, 3, meta["vit_grid"][0] * 14, meta["vit_grid"][1] * 14), generator=gen))
            gi, lens, rope = orc.prepare_vit_image(lens, rope, pv, thw, nt)
            orc.forward_cache_update_vit(cache, gi)
        start = tok.encode("<|im_start|>user\\your text<|im_end|>\n<|im_start|>assistant\n", add_special_tokens=False)[-1]
        V = dims["llm"]["vocab"]
        other = [(ref[0] + 1 + 7 * i) % V for i in range(9)]
        conts = [[ref[:1], ref[:1], other[:4]], [ref[:5], ref, other], [ref[:9], [9, 8]]]
        questions = []
        for p, cs in zip([meta["prompt"] + " and how wide is the door", meta["prompt"], meta["prompt"]], conts):
            gq, _, qrope = orc.prepare_prompts(lens, rope, [p + "<|im_end|>\n<|im_start|>assistant"], tok, nt)
            questions.append((gq["packed_text_ids"].tolist(), gq["packed_text_position_ids"][0].tolist(), int(start), int(qrope[0]), cs))
        P = int(lens[0])
        K, V_ = [cache.key_cache[i] for i in range(orc.num_layers)], [cache.value_cache[i] for i in range(orc.num_layers)]
        assert K[0].shape[0] == P
        case = dict(kind="questions", dims="margin", P=P, layout=tuple((len(q[0]), tuple(len(c) for c in q[4])) for q in questions),
                    top_k=0, cap="larger", exact_only=False)
        _MARGIN["scene"] = (sd, dims, case, questions, (K, V_), ref)
    return _MARGIN["scene"]


def lp_shift(fault, golden_dir):
    """Column (b) of DESIGN 6s: the largest |lp - clean lp| over the 71 reference tokens (the second choice of the second of
    three questions) when `fault` is planted in the bf16 oracle's scoring of chat_real2_margin - what the e2e tests would have
    to see.  Returns (shift, P)."""
    sd, dims, case, questions, scene, ref = margin_scene(golden_dir)
    Lq, L, starts, chs = sizes(case)
    lo = sum(n for j, c, b, n in chs if (j, c) < (1, 1))
    if "clean" not in _MARGIN:
        _MARGIN["clean"] = score(ScoreOracle(sd, dims), case, questions, scene)
    clean = _MARGIN["clean"]
    assert clean["ranks"][lo:lo + 71].tolist() == [0] * 71 and clean["targets"][lo:lo + 71].tolist() == ref
    # the fixture question's 71-token choice alone under the fault, in its place in the packing (what it finds in the cache
    # comes from the clean pass); a targets / first-row fault moves the packed rows, so the whole tail is scored
    whole = fault in ("targets_shifted_one", "first_row_off_by_one")
    bad = score(ScoreOracle(sd, dims, fault=fault), case, questions, scene, clean, only=None if whole else {(1, 1)})
    got = bad["logprobs"][lo:lo + 71] if whole else bad["logprobs"]
    return float((got.double() - clean["logprobs"][lo:lo + 71].double()).abs().max()), case["P"]
