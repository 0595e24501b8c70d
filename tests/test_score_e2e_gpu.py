"""GPU, end to end: scoring given continuations (G2VLM.score_continuations / chat_with_recon_choices, Engine.score_rows) on the
chat_real2_margin network: real widths, 2 layers, the reference's 71 greedy ids and its bf16 logits of every step in the golden
file, top-1 / top-2 gap >= 4 bf16 ulp at every step.

Measured on an MI355X: figures in the docstrings below and in DESIGN 6g."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from oracle import synth  # noqa: E402  (checker only)
from test_e2e_gpu import load  # noqa: E402
from test_fp8_decode_e2e_gpu import decode_logits  # noqa: E402
from test_shared_prefix_e2e_gpu import transform_over, vit_inputs  # noqa: E402


@pytest.fixture(scope="module")
def scene(golden_dir):
    meta, g = load(golden_dir, "chat_real2_margin")
    dims = meta["dims"]
    from g2vlm_amd.g2vlm_utils import build_model, configs_from_dims
    sd = synth.peaked_lm_head(synth.synth_state_dict(dims, seed=meta["seed"]), meta["head_sigma"], meta["head_seed"])
    model = build_model(*configs_from_dims(dims), sd, "cuda")
    tok = synth.FakeTokenizer(dims["llm"]["vocab"])
    imgs = synth.synth_images(meta["n"], meta["h"], meta["w"], meta["seed"])
    ref = [int(v) for v in g["ref.ids"].tolist()]
    assert len(ref) == 71 and meta["min_margin_ulp"] >= 4.0
    return meta, g, model, tok, imgs, ref


def prefill(model, tok, meta, imgs):
    return model._chat_prefill(tok, tok.new_token_ids, transform_over(vit_inputs(meta)), None, imgs, meta["prompt"])


def logit_ulp(g):
    """bf16 ulp of the largest logit of the reference's run."""
    top = float(g["ref.logits"].float().abs().max())
    return 2.0 ** (math.floor(math.log2(top)) - 7)


def test_scores_against_the_reference(scene):
    """log_softmax(ref.logits[t].double())[ref.ids[t]] for the 71 reference ids against the teacher-forced scores; every rank
    0.  The allowance is measured, not fixed: the eager batch-1 decode fed the same ids deviates from the reference by at most
    d, the scored path may deviate by 2 d + 1e-3 (two bf16 evaluations of one network in different summation orders).
    Measured: d = 3.14e-2, scored path 3.67e-2, allowed 6.38e-2."""
    meta, g, model, tok, imgs, ref = scene
    want = torch.log_softmax(g["ref.logits"][:71].double(), dim=-1).gather(1, torch.tensor(ref)[:, None])[:, 0]
    past, gi = prefill(model, tok, meta, imgs)
    (got,) = model.score_continuations(past, gi, [ref])
    assert got["logprobs"].shape == (71,) and got["logprobs"].dtype == torch.float32 and got["ranks"].shape == (71,)
    start = int(gi["packed_start_tokens"][0])
    _, ids, lg = decode_logits(model, tok, meta, imgs, 71, use_graph=False, force_ids=[start] + ref[:-1])
    assert ids[1:] == ref                                    # the decode the fixture pins, teacher-forced or not
    dec = torch.log_softmax(torch.stack(lg, 0).double(), dim=-1).gather(1, torch.tensor(ref)[:, None])[:, 0]
    d = float((dec - want).abs().max())
    dev = float((got["logprobs"].double() - want).abs().max())
    print(f"[score e2e] max |lp - reference| over 71 steps: decode path d = {d:.3e}, scored path {dev:.3e}, allowed {2 * d + 1e-3:.3e}; "
          f"total {got['total']:.4f} vs reference {float(want.sum()):.4f}")
    assert got["ranks"].tolist() == [0] * 71
    assert dev <= 2 * d + 1e-3, (dev, d)
    assert got["total"] == float(got["logprobs"].double().sum())


def test_batching_changes_nothing_that_matters(scene):
    """The reference continuation alone, as the middle one of three (beside its own first 5 ids and 9 other ids) and as each of
    64 copies: identical ranks, log-probabilities within the kernel bound (1e-4: every target is its row's maximum) plus 2 bf16
    ulp of the largest logit (the lm_head GEMM's route changes with the row count).  The 5-id prefix scores as the first 5
    tokens of the full continuation: nothing leaks from later rows or from another segment."""
    meta, g, model, tok, imgs, ref = scene
    tol = 1e-4 + 2 * logit_ulp(g)
    past, gi = prefill(model, tok, meta, imgs)
    (alone,) = model.score_continuations(past, gi, [ref])
    other = [(ref[0] + 1 + 7 * i) % meta["dims"]["llm"]["vocab"] for i in range(9)]
    three = model.score_continuations(past, gi, [ref[:5], ref, other])
    copies = model.score_continuations(past, gi, [ref] * 64)
    worst = 0.0
    for name, got in [("middle of three", three[1])] + [(f"copy {j}", c) for j, c in enumerate(copies)]:
        assert got["ranks"].tolist() == alone["ranks"].tolist(), name
        e = float((got["logprobs"] - alone["logprobs"]).abs().max())
        worst = max(worst, e)
        assert e <= tol, (name, e, tol)
    assert three[0]["ranks"].tolist() == alone["ranks"][:5].tolist()
    e5 = float((three[0]["logprobs"] - alone["logprobs"][:5]).abs().max())
    assert e5 <= tol, (e5, tol)
    assert len(three[2]["logprobs"]) == 9 and bool(torch.isfinite(three[2]["logprobs"]).all()) and max(three[2]["ranks"].tolist()) > 0
    print(f"[score e2e] batching: max |lp - lp alone| {worst:.3e} (prefix of 5: {e5:.3e}), allowed {tol:.3e}")


def test_the_cache_is_left_alone(scene):
    meta, g, model, tok, imgs, ref = scene
    past, gi = prefill(model, tok, meta, imgs)
    n = past.length
    snap = [(past.k[i][:n].clone(), past.v[i][:n].clone()) for i in range(past.num_layers)]
    model.score_continuations(past, gi, [ref, ref[:3]])
    assert past.length == n
    for i, (k, v) in enumerate(snap):
        assert torch.equal(past.k[i][:n], k) and torch.equal(past.v[i][:n], v), i
    ids = model.generate_text(past_key_values=past, max_length=meta["max_length"], end_token_id=tok.new_token_ids["eos_token_id"], **gi)
    assert ids[1:, 0].tolist() == ref


class ChoiceTokenizer(synth.FakeTokenizer):
    def __init__(self, vocab, table):
        super().__init__(vocab)
        self.table = table

    def encode(self, text, add_special_tokens=False):
        if text in self.table:
            assert add_special_tokens is False
            return list(self.table[text])
        return super().encode(text, add_special_tokens)


def test_chat_with_recon_choices(scene):
    """Three answers that share their tokens 2-4: the reference's first 4 ids and two that differ from it in the first token.
    The first-token rank is 0 for the reference's and above 0 for the others; the winner is the reference's."""
    meta, g, model, tok, imgs, ref = scene
    V = meta["dims"]["llm"]["vocab"]
    table = {"wrong one": [(ref[0] + 1) % V] + ref[1:4], "right": ref[:4], "wrong two": [(ref[0] + 977) % V] + ref[1:4]}
    ctok = ChoiceTokenizer(V, table)
    eos = ctok.new_token_ids["eos_token_id"]
    args = (ctok, ctok.new_token_ids, transform_over(vit_inputs(meta)), None, imgs, meta["prompt"], list(table))
    best, scores, details = model.chat_with_recon_choices(*args)
    assert best == 1 and len(scores) == len(details) == 3
    for j, (text, d) in enumerate(zip(table, details)):
        assert d["ids"] == table[text] + [eos] and len(d["logprobs"]) == 5
        assert d["total"] == float(d["logprobs"].double().sum()) and scores[j] == d["total"]
    assert int(details[1]["ranks"][0]) == 0 and int(details[0]["ranks"][0]) > 0 and int(details[2]["ranks"][0]) > 0
    assert float(details[1]["logprobs"][0]) > max(float(details[0]["logprobs"][0]), float(details[2]["logprobs"][0]))
    assert scores[1] > max(scores[0], scores[2])
    args = (ctok, ctok.new_token_ids, transform_over(vit_inputs(meta)), None, imgs, meta["prompt"], list(table))
    best_n, scores_n, details_n = model.chat_with_recon_choices(*args, append_eos=False, normalize=True)
    assert best_n == 1
    for d, dn, s in zip(details, details_n, scores_n):
        assert dn["ids"] == d["ids"][:-1] and s == dn["total"] / 4
        assert torch.equal(dn["ranks"], d["ranks"][:4])


def test_modes_do_not_leak(scene):
    """decode_weights = "fp8" and decode_kv = "fp8" leave the scores bit-identical: scoring is a prefill."""
    meta, g, model, tok, imgs, ref = scene
    conts = [ref, ref[:5], [5, 6, 7]]

    def run():
        past, gi = prefill(model, tok, meta, imgs)
        return model.score_continuations(past, gi, conts)
    off = run()
    model.decode_weights, model.decode_kv = "fp8", "fp8"
    try:
        assert model.engine.decode_weights == "fp8" and model.engine.decode_kv == "fp8"
        on = run()
    finally:
        model.decode_weights, model.decode_kv = "bf16", "bf16"
    for a, b in zip(off, on):
        assert torch.equal(a["logprobs"], b["logprobs"]) and torch.equal(a["ranks"], b["ranks"]) and a["total"] == b["total"]
