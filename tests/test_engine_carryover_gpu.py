"""GPU: a long-lived model computes what a fresh model computes.

One G2VLM keeps, across calls, attention plans by windows (Engine._tiles), RoPE2D and DINO position tables, zero buffers, memoised
index tensors (G2VLM._idx_cache, cleared at 256 entries), the scoring plans (Engine._score_plans, 32 kept), the captured decode
step (Engine._decode_cached) and, below them, hip.py's per-stream scratch: the skinny GEMM's tickets, the argmax, logprob and top-k
tickets, the cloud workspaces, the resize tables.  The product serves scenes of changing sizes and modes from one such model.

A fixed, seeded "day in the life" runs through ONE model on the tiny dims of tests/golden/chat_tiny (built as tests/test_e2e_gpu.py
builds it): reconstructions of three shapes, greedy chat from the captured graph, scored choices, scored questions with top-k, fp8
weights, fp8 KV, back to bf16, several questions over one scene, three scenes decoded together, and the first reconstruction once
more.  Every step's outputs - points, poses, confidences, token ids, log-probabilities, ranks, top-k ids - equal, bit for bit, the
same call on a model built for that step alone; a second run of the whole day on the same model gives the same bits again; and so
does the first call after the index cache has been cleared and the scoring plans evicted.  The DINOv3 reconstruction of the issue's
list is left out: a model has ONE geometry encoder, and the tiny fixture's is DINOv2 (tests/test_e2e_gpu.py covers DINOv3 on its
own model).  No tolerance anywhere: the kernels are run-to-run bit-identical."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from oracle import synth  # noqa: E402  (inputs only)
from test_e2e_gpu import build, load  # noqa: E402
from test_score_e2e_gpu import ChoiceTokenizer  # noqa: E402
from test_shared_prefix_e2e_gpu import capture_ids, transform_over, vit_inputs  # noqa: E402

STEPS = 10                                                   # tokens per answer: every step well under a second
PROMPTS = ["\nHow far is the chair?", "\nWhat colour is the door?\nAnswer in one word.", "\nIs there a table?"]


def tensors_of(x):
    """every tensor of a result (dicts, lists, tuples), on the host, in a fixed order; other leaves as they are"""
    if torch.is_tensor(x):
        return [x.detach().cpu()]
    if isinstance(x, dict):
        return [t for k in sorted(x) for t in tensors_of(x[k])]
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in tensors_of(v)]
    return [x]


def same(a, b):
    a, b = tensors_of(a), tensors_of(b)
    if len(a) != len(b):
        return False
    for u, v in zip(a, b):
        if torch.is_tensor(u) != torch.is_tensor(v):
            return False
        if torch.is_tensor(u):
            if u.dtype != v.dtype or u.shape != v.shape or not torch.equal(u.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)):
                return False
        elif u != v:
            return False
    return True


class Day:
    def __init__(self, golden_dir):
        self.meta, _ = load(golden_dir, "chat_tiny")
        self.dims, self.seed = self.meta["dims"], self.meta["seed"]
        V = self.dims["llm"]["vocab"]
        self.table = {"near": [17, 40, 9], "two metres": [33, 7, 120, 250, 5], "far": [200]}
        self.tok = ChoiceTokenizer(V, self.table)
        self.nt = self.tok.new_token_ids
        self.views = {k: synth.synth_images(*k, 7 + i) for i, k in enumerate(((2, 56, 84), (3, 56, 56), (1, 56, 70)))}

    def fresh(self):
        return build(self.dims, self.seed)[0]

    def vit(self, n=1):
        meta = dict(self.meta, n=n)
        return transform_over(vit_inputs(meta))

    # ---- the calls; each returns everything the caller would see
    def recon(self, m, key):
        pred = m.recon(self.tok, self.nt, None, self.views[key])
        return {k: v for k, v in pred.items() if torch.is_tensor(v)}

    def chat(self, m, graph=True, weights="bf16", kv="bf16"):
        m.use_decode_graph, m.decode_weights, m.decode_kv = graph, weights, kv
        got = capture_ids(self.tok)
        try:
            m.chat_with_recon(self.tok, self.nt, self.vit(), None, self.views[(1, 56, 70)], PROMPTS[0], STEPS)
        finally:
            del self.tok.decode                              # the instance attribute capture_ids set: back to the class's decode
            m.use_decode_graph, m.decode_weights, m.decode_kv = True, "bf16", "bf16"
        return got

    def choices(self, m):
        return m.chat_with_recon_choices(self.tok, self.nt, self.vit(), None, self.views[(1, 56, 70)], PROMPTS[0], list(self.table))

    def questions_scored(self, m):
        return m.chat_with_recon_questions_choices(self.tok, self.nt, self.vit(), None, self.views[(1, 56, 70)], PROMPTS, list(self.table),
                                                   top_k=3)

    def questions(self, m):
        got = capture_ids(self.tok)
        try:
            m.chat_with_recon_questions(self.tok, self.nt, self.vit(), None, self.views[(1, 56, 70)], PROMPTS, STEPS)
        finally:
            del self.tok.decode
        return got

    def batch(self, m):
        got = capture_ids(self.tok)
        scenes = [(self.views[(1, 56, 70)], p) for p in PROMPTS]
        try:
            m.chat_with_recon_batch(self.tok, self.nt, self.vit(3), None, scenes, STEPS)
        finally:
            del self.tok.decode
        return got

    def steps(self):
        return [("recon 2 x 56 x 84", lambda m: self.recon(m, (2, 56, 84))),
                ("chat, greedy, graph", lambda m: self.chat(m)),
                ("recon 3 x 56 x 56", lambda m: self.recon(m, (3, 56, 56))),
                ("score_continuations", self.choices),
                ("score_questions top_k 3", self.questions_scored),
                ("recon 2 x 56 x 84 again", lambda m: self.recon(m, (2, 56, 84))),
                ("chat, fp8 weights", lambda m: self.chat(m, weights="fp8")),
                ("chat, fp8 kv", lambda m: self.chat(m, kv="fp8")),
                ("chat, bf16 again", lambda m: self.chat(m)),
                ("chat, eager", lambda m: self.chat(m, graph=False)),
                ("shared-prefix questions", self.questions),
                ("batched decode, 3 slots", self.batch),
                ("the first recon once more", lambda m: self.recon(m, (2, 56, 84)))]


@pytest.fixture(scope="module")
def day(golden_dir):
    """the day on one long-lived model: (Day, the model, every step's result)"""
    d = Day(golden_dir)
    model = d.fresh()
    return d, model, [(name, call(model)) for name, call in d.steps()]


def test_every_step_equals_the_same_call_on_a_fresh_model(day):
    d, _, lived = day
    for (name, call), (_, got) in zip(d.steps(), lived):
        want = call(d.fresh())
        assert len(tensors_of(want)) > 0, name
        assert same(got, want), f"step '{name}': the long-lived model and a fresh one disagree"
    # the steps are not vacuous: answers of STEPS - 1 ids (the start token dropped) unless eos came first, three of them where three are asked
    ids = dict(lived)
    assert len(ids["chat, greedy, graph"]) == 1 and 0 <= len(ids["chat, greedy, graph"][0]) <= STEPS
    assert len(ids["shared-prefix questions"]) == 3 and len(ids["batched decode, 3 slots"]) == 3
    assert ids["chat, greedy, graph"] == ids["chat, bf16 again"]
    assert same(ids["recon 2 x 56 x 84"], ids["the first recon once more"]) and same(ids["recon 2 x 56 x 84"], ids["recon 2 x 56 x 84 again"])
    best, scores, details = ids["score_continuations"]
    assert len(scores) == 3 and [len(x["logprobs"]) for x in details] == [4, 6, 2]
    assert [len(q[2]) for q in ids["score_questions top_k 3"]] == [3, 3, 3] and ids["score_questions top_k 3"][0][2][0]["top_ids"].shape == (4, 3)


def test_a_second_day_on_the_same_model_gives_the_same_bits(day):
    d, model, lived = day
    for (name, call), (_, first) in zip(d.steps(), lived):
        assert same(call(model), first), f"step '{name}' changed on its second run through the long-lived model"


def test_the_first_call_again_after_the_caches_have_turned_over(day):
    """Distinct continuations in a loop push G2VLM._idx_cache through its 256-entry clear and Engine._score_plans past its 32 kept
    plans (their attention plans leave Engine._tiles with them); then the first call again."""
    d, model, _ = day
    eng = model.engine
    past, gi = model._chat_prefill(d.tok, d.nt, d.vit(), None, d.views[(1, 56, 70)], PROMPTS[1])
    first_conts = [[9, 8, 7], [300, 2]]
    first = model.score_continuations(past, gi, first_conts, top_k=2)
    fresh = d.fresh()
    fpast, fgi = fresh._chat_prefill(d.tok, d.nt, d.vit(), None, d.views[(1, 56, 70)], PROMPTS[1])
    assert same(first, fresh.score_continuations(fpast, fgi, first_conts, top_k=2))
    V = d.dims["llm"]["vocab"]
    sizes, cleared, plans_seen = [len(model._idx_cache)], 0, set()
    for i in range(120):
        a, b = 1 + i % 12, 1 + i // 12                       # 120 distinct (a, b): 120 distinct window sets
        conts = [[(5 + i + j) % V for j in range(a)], [(11 + 3 * i + j) % V for j in range(b)]]
        model.score_continuations(past, gi, conts)
        plans_seen.add((a, b))
        sizes.append(len(model._idx_cache))
        cleared += sizes[-1] < sizes[-2]
        assert len(eng._score_plans) <= eng.SCORE_PLANS_KEPT
    assert cleared >= 1, ("the index cache never reached its clear", sizes[-5:])
    assert len(plans_seen) > eng.SCORE_PLANS_KEPT == len(eng._score_plans)
    assert same(model.score_continuations(past, gi, first_conts, top_k=2), first)
    assert past.length == fpast.length
    name, call = d.steps()[0]
    assert same(call(model), call(fresh)), "the first reconstruction after the caches turned over"
