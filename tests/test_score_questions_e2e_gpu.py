"""GPU, end to end: the choices of several questions about one scene scored in one pass, with top-k tokens
(G2VLM.score_questions / chat_with_recon_questions_choices, Engine.score_questions) on the chat_real2_margin network, as
tests/test_score_e2e_gpu.py uses it: real widths, 2 layers, the reference's 71 greedy ids and its bf16 logits of every step in
the golden file, top-1 / top-2 gap >= 4 bf16 ulp at every step.  Three prompts; the fixture's question is the second and the
third, another question the first.

Which choices carry the allowance 2 d + 1e-3.  d is measured on the fixture's greedy tokens: every target is its row's maximum
by at least 4 bf16 ulp, so a one-ulp step of the top logit between two evaluations moves x_t and the logsumexp together and
the log-probability by (1 - p) ulp.  The allowance is therefore applied to every choice that is greedy with that margin: the
reference continuation and its prefixes under the fixture question, and under the other question its own greedy continuation
(the per-question decode's), cut before the first step whose top-1 / top-2 gap on the per-question path is below 4 ulp.  Every
question also gets a choice of unlikely tokens (ranks in the hundreds, log-probabilities near -30): they exercise ranks, top-k
and the leak check, and their logits of magnitude 16 .. 32 have a bf16 ulp of 0.125 - one ulp is twice the allowance - so they
are held to tests/test_score_e2e_gpu.py's batching bound instead, 1e-4 + 2 bf16 ulp of the largest logit.

Measured on an MI355X: figures in the docstrings below and in DESIGN 6h."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from test_fp8_decode_e2e_gpu import decode_logits  # noqa: E402
from test_score_e2e_gpu import ChoiceTokenizer, logit_ulp, prefill, scene  # noqa: E402, F401  (scene: the module's fixture)
from test_shared_prefix_e2e_gpu import transform_over, vit_inputs  # noqa: E402

TOP_K = 5
LOGPROB_BOUND = 1e-4                                          # tests/test_logprob_gpu.py's bound where the target is the row's maximum
SUFFIX = "<|im_end|>\n<|im_start|>assistant"


def prompts_of(meta):
    return [meta["prompt"] + " and how wide is the door", meta["prompt"], meta["prompt"]]


def greedy_with_margin(model, tok, meta, imgs, g, prompt, steps=6):
    """The per-question path's own greedy continuation of `prompt`, cut before the first step whose top-1 / top-2 logit gap
    (on that path) is below 4 bf16 ulp - the property the fixture guarantees for its own question; at least one token."""
    args = (tok, tok.new_token_ids, transform_over(vit_inputs(meta)), None, imgs, prompt)
    past, gi = model._chat_prefill(*args)
    ids = model.generate_text(past_key_values=past, max_length=steps + 1, end_token_id=None, **gi)[1:, 0].tolist()
    past, gi = model._chat_prefill(*args[:2], transform_over(vit_inputs(meta)), *args[3:])
    (d,) = model.score_continuations(past, gi, [ids], top_k=2)
    gap = (d["top_logprobs"][:, 0] - d["top_logprobs"][:, 1]).tolist()
    keep = next((i for i, (r, m) in enumerate(zip(d["ranks"].tolist(), gap)) if r != 0 or m < 4 * logit_ulp(g)), len(ids))
    print(f"[questions e2e] the other question's greedy ids {ids}, top-1 / top-2 gaps {[round(m, 3) for m in gap]}: {max(keep, 1)} kept")
    return ids[:max(keep, 1)]


def continuations_of(meta, ref, g0):
    """Per question (choices, which of them are greedy with margin)."""
    V = meta["dims"]["llm"]["vocab"]
    other = [(ref[0] + 1 + 7 * i) % V for i in range(9)]
    return [([g0, g0[:1], other[:4]], (True, True, False)), ([ref[:5], ref, other], (True, True, False)), ([ref[:9], [9, 8]], (True, False))]


def scene_cache(model, tok, meta, imgs):
    """The scene alone - system prompt, geometry views, ViT images - and its (lens, rope)."""
    past, newlens, new_rope = model._chat_geometry(tok, tok.new_token_ids, None, imgs)
    return model._chat_vit(past, newlens, new_rope, tok.new_token_ids, transform_over(vit_inputs(meta)), imgs)


def questions_behind(model, tok, newlens, new_rope, prompts, conts):
    out = []
    for p, c in zip(prompts, conts):
        ti, qlens, qrope = model.prepare_prompts_pure_text(newlens, new_rope, [p + SUFFIX], tok, tok.new_token_ids)
        out.append((ti, model.prepare_start_tokens(qlens, qrope, tok, tok.new_token_ids), c))
    return out


def same_bits(a, b):
    return all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k])) and a["total"] == b["total"] and a.keys() == b.keys()


@pytest.fixture(scope="module")
def shared(scene):
    """The scene's cache, the three questions behind it, one score_questions pass with top-k, and d: how far the eager batch-1
    decode fed the reference's ids is from the reference."""
    meta, g, model, tok, imgs, ref = scene
    past, newlens, new_rope = scene_cache(model, tok, meta, imgs)
    n = past.length
    snap = [(past.k[i][:n].clone(), past.v[i][:n].clone()) for i in range(past.num_layers)]
    g0 = greedy_with_margin(model, tok, meta, imgs, g, prompts_of(meta)[0])
    conts = continuations_of(meta, ref, g0)
    qs = questions_behind(model, tok, newlens, new_rope, prompts_of(meta), [c for c, _ in conts])
    got = model.score_questions(past, qs, top_k=TOP_K)
    want = torch.log_softmax(g["ref.logits"][:71].double(), dim=-1).gather(1, torch.tensor(ref)[:, None])[:, 0]
    _, gi = prefill(model, tok, meta, imgs)
    _, ids, lg = decode_logits(model, tok, meta, imgs, 71, use_graph=False, force_ids=[int(gi["packed_start_tokens"][0])] + ref[:-1])
    assert ids[1:] == ref
    dec = torch.log_softmax(torch.stack(lg, 0).double(), dim=-1).gather(1, torch.tensor(ref)[:, None])[:, 0]
    return dict(conts=[c for c, _ in conts], greedy=[f for _, f in conts], past=past, n=n, snap=snap, lens=newlens, rope=new_rope, qs=qs, got=got, want=want, d=float((dec - want).abs().max()))


def test_scores_against_the_reference(scene, shared):
    """The fixture question's reference continuation, scored as one of three choices of the second of three questions, against
    log_softmax(ref.logits.double())[ref.ids]; every rank 0.  Allowed: 2 d + 1e-3, d the measured deviation of the eager batch-1
    decode from the reference (a second bf16 evaluation of one network in another summation order).
    Measured: d = 3.14e-2, the three-question pass 3.67e-2, allowed 6.38e-2."""
    meta, g, model, tok, imgs, ref = scene
    got, d = shared["got"][1][1], shared["d"]
    assert [len(q) for q in shared["got"]] == [3, 3, 2]
    assert got["logprobs"].shape == (71,) and got["logprobs"].dtype == torch.float32 and got["ranks"].dtype == torch.int32
    dev = float((got["logprobs"].double() - shared["want"]).abs().max())
    print(f"[questions e2e] max |lp - reference| over 71 steps: decode path d = {d:.3e}, three-question pass {dev:.3e}, "
          f"allowed {2 * d + 1e-3:.3e}; total {got['total']:.4f} vs reference {float(shared['want'].sum()):.4f}")
    assert got["ranks"].tolist() == [0] * 71
    assert dev <= 2 * d + 1e-3, (dev, d)
    assert got["total"] == float(got["logprobs"].double().sum())


def test_against_the_per_question_path(scene, shared):
    """chat_with_recon_questions_choices against chat_with_recon_choices for every prompt alone (its own prefill of scene and
    question, score_rows).  Greedy choices with margin (module docstring): log-probabilities within 2 d + 1e-3 and equal ranks,
    all 0.  The choices of unlikely tokens: within 1e-4 + 2 bf16 ulp of the largest logit.  The same winner everywhere.
    Measured: greedy choices 4.39e-2 (allowed 6.38e-2), unlikely choices 2.62e-1 (allowed 5.00e-1)."""
    meta, g, model, tok, imgs, ref = scene
    conts = shared["conts"]
    names = [[f"c{j}{c}" for c in range(len(cs))] for j, cs in enumerate(conts)]
    ctok = ChoiceTokenizer(meta["dims"]["llm"]["vocab"], {nm: ids for ns, cs in zip(names, conts) for nm, ids in zip(ns, cs)})
    nt, prompts = ctok.new_token_ids, prompts_of(meta)
    res = model.chat_with_recon_questions_choices(ctok, nt, transform_over(vit_inputs(meta)), None, imgs, prompts, names, append_eos=False,
                                                  top_k=TOP_K)
    tol, tol_low, worst, worst_low = 2 * shared["d"] + 1e-3, 1e-4 + 2 * logit_ulp(g), 0.0, 0.0
    assert len(res) == 3
    for j, (best, scores, details) in enumerate(res):
        best1, scores1, details1 = model.chat_with_recon_choices(ctok, nt, transform_over(vit_inputs(meta)), None, imgs, prompts[j], names[j],
                                                                 append_eos=False)
        assert len(details) == len(details1) == len(conts[j])
        for c, (a, b) in enumerate(zip(details, details1)):
            assert a["ids"] == b["ids"] == conts[j][c] and a["total"] == float(a["logprobs"].double().sum())
            assert same_bits({k: v for k, v in a.items() if k != "ids"}, shared["got"][j][c])     # the public pass is score_questions'
            e = float((a["logprobs"] - b["logprobs"]).abs().max())
            print(f"[questions e2e] question {j} choice {c}: {len(conts[j][c])} tokens, ranks {a['ranks'].tolist()[:9]} / {b['ranks'].tolist()[:9]}, "
                  f"lowest lp {float(b['logprobs'].min()):.2f}, max |lp one pass - lp alone| {e:.3e}")
            if shared["greedy"][j][c]:
                worst = max(worst, e)
                assert a["ranks"].tolist() == b["ranks"].tolist() == [0] * len(conts[j][c]), (j, c)
            else:
                worst_low = max(worst_low, e)
                assert min(a["ranks"].tolist()) > 0 and min(b["ranks"].tolist()) > 0
        assert scores == [d["total"] for d in details] and best == best1
    assert res[1][0] == 0 and res[1][1][2] < res[1][1][1] < res[1][1][0]      # totals: the first 5 reference tokens, all 71, 9 others
    print(f"[questions e2e] max |lp one pass - lp per question|: greedy choices {worst:.3e}, allowed {tol:.3e}; "
          f"unlikely choices {worst_low:.3e}, allowed {tol_low:.3e}")
    assert worst <= tol, (worst, tol)
    assert worst_low <= tol_low, (worst_low, tol_low)


def test_nothing_leaks_from_the_other_questions(scene, shared):
    """Other ids of the same lengths in the other two questions and in their choices: the fixture question's log-probabilities,
    ranks and top-k keep their bits."""
    meta, g, model, tok, imgs, ref = scene
    V = meta["dims"]["llm"]["vocab"]
    qs = []
    for j, (ti, gi, conts) in enumerate(shared["qs"]):
        if j != 1:
            ti = dict(ti, packed_text_ids=(ti["packed_text_ids"] + 1 + 3 * torch.arange(ti["packed_text_ids"].numel())) % V)
            conts = [[(t + 11) % V for t in c] for c in conts]
        qs.append((ti, gi, conts))
    got = model.score_questions(shared["past"], qs, top_k=TOP_K)
    for a, b in zip(got[1], shared["got"][1]):
        assert same_bits(a, b)
    assert not same_bits(got[0][0], shared["got"][0][0])       # the other questions' scores did move


def test_top_k(scene, shared):
    """top_ids[:, 0] is the reference continuation itself and top_logprobs[:, 0] its log-probability (twice the logprob kernel's
    bound: both are x_max - logsumexp); a target of rank r < k sits in column r; the columns descend; top_k = 5 leaves
    logprobs and ranks as top_k = 0 gives them, in score_continuations too."""
    meta, g, model, tok, imgs, ref = scene
    d = shared["got"][1][1]
    assert d["top_ids"].shape == (71, TOP_K) and d["top_ids"].dtype == torch.int32 and d["top_logprobs"].dtype == torch.float32
    assert d["top_ids"][:, 0].tolist() == ref
    e = float((d["top_logprobs"][:, 0] - d["logprobs"]).abs().max())
    print(f"[questions e2e] max |top_logprobs[:, 0] - logprobs| over the reference continuation: {e:.3e}, allowed {2 * LOGPROB_BOUND:.1e}")
    assert e <= 2 * LOGPROB_BOUND
    conts, seen = shared["conts"], 0
    for dicts, cs in zip(shared["got"], conts):
        for dd, c in zip(dicts, cs):
            assert bool((dd["top_logprobs"][:, :-1] >= dd["top_logprobs"][:, 1:]).all()) and bool((dd["top_logprobs"] <= 0).all())
            assert bool(((dd["top_ids"] >= 0) & (dd["top_ids"] < meta["dims"]["llm"]["vocab"])).all())
            for p, (t, r) in enumerate(zip(c, dd["ranks"].tolist())):
                if r < TOP_K:
                    assert int(dd["top_ids"][p, r]) == t
                    seen += 1
                else:
                    assert t not in dd["top_ids"][p].tolist()
    assert seen >= 71 + 5 + 9
    assert any(r >= TOP_K for dicts in shared["got"] for dd in dicts for r in dd["ranks"].tolist())
    plain = model.score_questions(shared["past"], shared["qs"])
    for a_q, b_q in zip(plain, shared["got"]):
        for a, b in zip(a_q, b_q):
            assert set(a) == {"logprobs", "ranks", "total"}
            assert torch.equal(a["logprobs"], b["logprobs"]) and torch.equal(a["ranks"], b["ranks"]) and a["total"] == b["total"]
    past, gi = prefill(model, tok, meta, imgs)
    zero = model.score_continuations(past, gi, conts[1])
    five = model.score_continuations(past, gi, conts[1], top_k=TOP_K)
    for a, b in zip(zero, five):
        assert set(a) == {"logprobs", "ranks", "total"} and set(b) == set(a) | {"top_ids", "top_logprobs"}
        assert torch.equal(a["logprobs"], b["logprobs"]) and torch.equal(a["ranks"], b["ranks"]) and a["total"] == b["total"]
    assert five[1]["top_ids"][:, 0].tolist() == ref


def test_modes_do_not_leak(scene, shared):
    """decode_weights = "fp8" and decode_kv = "fp8" leave everything bit-identical: scoring is a prefill."""
    meta, g, model, tok, imgs, ref = scene
    model.decode_weights, model.decode_kv = "fp8", "fp8"
    try:
        assert model.engine.decode_weights == "fp8" and model.engine.decode_kv == "fp8"
        on = model.score_questions(shared["past"], shared["qs"], top_k=TOP_K)
    finally:
        model.decode_weights, model.decode_kv = "bf16", "bf16"
    for a_q, b_q in zip(on, shared["got"]):
        for a, b in zip(a_q, b_q):
            assert same_bits(a, b)


def test_the_scene_cache_is_left_alone(scene, shared):
    """After all of the above the scene's cache has its length and its bits, and the fixture question decoded over it
    (generate_text_shared) gives the fixture's ids."""
    meta, g, model, tok, imgs, ref = scene
    past, n = shared["past"], shared["n"]
    model.score_questions(past, shared["qs"], top_k=TOP_K)
    assert past.length == n
    for i, (k, v) in enumerate(shared["snap"]):
        assert torch.equal(past.k[i][:n], k) and torch.equal(past.v[i][:n], v), i
    from g2vlm_amd.engine import KVCache
    past, gi = model._chat_question(past, shared["lens"], shared["rope"], tok, tok.new_token_ids, meta["prompt"])
    m = past.length - n
    suf = KVCache(past.num_layers, past.hkv, "cuda", capacity=m)
    for i in range(past.num_layers):
        suf.k[i].copy_(past.k[i][n:n + m]); suf.v[i].copy_(past.v[i][n:n + m])
    suf.length, past.length = m, n
    (ids,) = model.generate_text_shared(past, [(suf, gi)], meta["max_length"], end_token_id=tok.new_token_ids["eos_token_id"])
    assert ids[1:, 0].tolist() == ref
    assert past.length == n
