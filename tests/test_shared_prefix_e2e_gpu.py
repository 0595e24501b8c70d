"""GPU, end to end: several questions about one scene (G2VLM.chat_with_recon_questions / generate_text_shared /
Engine.decode_begin_shared).  The scene is prefilled once, every question's rows are prefilled on top of it as
chat_with_recon does, and all questions decode together over the one copy of the scene's rows."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from oracle import synth  # noqa: E402  (checker only)
from oracle.g2vlm_oracle import vit_patchify  # noqa: E402
from test_e2e_gpu import _decode_single, _near_tie, build, load, rel  # noqa: E402


def vit_inputs(meta):
    out = []
    for i in range(meta["n"]):
        gen = torch.Generator(); gen.manual_seed(1234 + i)
        out.append(vit_patchify(torch.randn((1, 3, meta["vit_grid"][0] * 14, meta["vit_grid"][1] * 14), generator=gen)))
    return out


def transform_over(queue):
    it = iter(queue)

    def image_transform(_imgs):
        pv, thw = next(it)
        return pv, torch.tensor([list(thw)])
    return image_transform


def capture_ids(tok):
    """tok.decode records the ids it is given (one list per answer) instead of decoding them."""
    got = []
    tok.decode = lambda ids: got.append([int(v) for v in ids]) or ""
    return got


def shared_vs_single(model, tok, meta, imgs, prompts, steps, use_graph):
    """Every question's shared-prefix decode gives the ids of its own batch-1 decode (a flip only at a near-tie of the
    batch-1 logits); returns the shared ids."""
    eng = model.engine
    singles = []
    for p in prompts:
        past, gi = model._chat_prefill(tok, tok.new_token_ids, transform_over(vit_inputs(meta)), None, imgs, p)
        singles.append(_decode_single(model, past, gi, steps))
    past, qs = model.prefill_questions(tok, tok.new_token_ids, transform_over(vit_inputs(meta)), None, imgs, prompts)
    plen = past.length
    k0, v0 = past.k[0][:plen].clone(), past.v[-1][:plen].clone()
    st = eng.decode_begin_shared(past, [q for q, _ in qs], [int(g["packed_start_tokens"][0]) for _, g in qs],
                                 [int(g["packed_query_position_ids"][0, 0]) for _, g in qs], steps, use_graph=use_graph)
    B = len(prompts)
    ids = [[t] for t in st["tok"].tolist()]
    alive = [True] * B
    for s in range(steps):
        tok_ = eng.decode_step_batch(st).tolist()
        lg = st["logits"].float().cpu()
        for j in range(B):
            if not alive[j]:
                continue
            ref_ids, ref_lg = singles[j]
            assert rel(lg[j], ref_lg[s]) < 3e-2, (j, s, rel(lg[j], ref_lg[s]))
            ids[j].append(tok_[j])
            if tok_[j] != ref_ids[s + 1]:
                assert _near_tie(ref_lg[s], tok_[j]), f"question {j} step {s}: {tok_[j]} vs {ref_ids[s + 1]} is not a near-tie flip"
                alive[j] = False
    for j in range(B):
        assert ids[j][0] == singles[j][0][0]
    # the shared rows are never written; each question's suffix rows sit in front of its decoded ones
    assert past.length == plen and torch.equal(past.k[0][:plen], k0) and torch.equal(past.v[-1][:plen], v0)
    for j, (q, _) in enumerate(qs):
        assert torch.equal(st["k"][0][j, :q.length], q.k[0][:q.length])
    assert st["len"].tolist() == [q.length + 1 + steps for q, _ in qs]
    return ids


def test_questions_are_token_exact_with_margin(golden_dir):
    """chat_real2_margin (top-1 / top-2 gap >= 4 bf16 ulp at every reference step): the golden question asked twice
    around another one returns exactly the reference's ids in both golden slots, graph replay and eager."""
    meta, g = load(golden_dir, "chat_real2_margin")
    dims = meta["dims"]
    from g2vlm_amd.g2vlm_utils import build_model, configs_from_dims
    sd = synth.peaked_lm_head(synth.synth_state_dict(dims, seed=meta["seed"]), meta["head_sigma"], meta["head_seed"])
    model = build_model(*configs_from_dims(dims), sd, "cuda")
    tok = synth.FakeTokenizer(dims["llm"]["vocab"])
    imgs = synth.synth_images(meta["n"], meta["h"], meta["w"], meta["seed"])
    ref = g["ref.ids"].tolist()
    prompts = [meta["prompt"], meta["prompt"] + " and how wide is the door", meta["prompt"]]
    for use_graph in (True, False):
        model.use_decode_graph = use_graph
        dec = tok.decode
        got = capture_ids(tok)
        model.chat_with_recon_questions(tok, tok.new_token_ids, transform_over(vit_inputs(meta)), None, imgs, prompts, meta["max_length"])
        tok.decode = dec
        assert len(got) == 3
        for j in (0, 2):
            assert got[j] == ref, (use_graph, j, next((i for i, (a, b) in enumerate(zip(got[j], ref)) if a != b), None))
    model.use_decode_graph = True


@pytest.mark.parametrize("name", ["chat_tiny", "chat_real2"])
def test_questions_match_their_single_decodes(golden_dir, name):
    meta, g = load(golden_dir, name)
    dims = meta["dims"]
    model, _ = build(dims, meta["seed"])
    tok = synth.FakeTokenizer(dims["llm"]["vocab"])
    imgs = synth.synth_images(meta["n"], meta["h"], meta["w"], meta["seed"])
    prompts = [meta["prompt"], meta["prompt"] + " and how large is the room in square metres", "x", meta["prompt"]]
    steps = meta["max_length"] - 1
    ids_e = shared_vs_single(model, tok, meta, imgs, prompts, steps, use_graph=False)
    ids_g = shared_vs_single(model, tok, meta, imgs, prompts, steps, use_graph=True)
    assert ids_e == ids_g, "graph replay and eager shared decode disagree"
    assert ids_e[0] == ids_e[3]


def test_questions_api_behaviour(golden_dir):
    """The scene's cache keeps its length and bits, so a second call on it repeats the ids; sampling is valid and repeats
    for a re-seeded model; bad arguments are refused before any prefill; decode_begin_shared allocates the same bytes
    whatever the prefix length."""
    meta, _ = load(golden_dir, "chat_tiny")
    dims = meta["dims"]
    model, _ = build(dims, meta["seed"])
    tok = synth.FakeTokenizer(dims["llm"]["vocab"])
    imgs = synth.synth_images(meta["n"], meta["h"], meta["w"], meta["seed"])
    eos = tok.new_token_ids["eos_token_id"]
    prompts = [meta["prompt"], "what is left of the door", meta["prompt"] + " in metres"]
    past, qs = model.prefill_questions(tok, tok.new_token_ids, transform_over(vit_inputs(meta)), None, imgs, prompts)
    plen = past.length
    snap = [(past.k[i][:plen].clone(), past.v[i][:plen].clone()) for i in range(past.num_layers)]
    a = model.generate_text_shared(past, qs, meta["max_length"], end_token_id=eos)
    assert past.length == plen
    assert all(torch.equal(past.k[i][:plen], k) and torch.equal(past.v[i][:plen], v) for i, (k, v) in enumerate(snap))
    b = model.generate_text_shared(past, qs, meta["max_length"], end_token_id=eos)
    assert [t.tolist() for t in a] == [t.tolist() for t in b]
    assert len(a) == 3 and all(1 <= t.shape[0] <= meta["max_length"] for t in a)

    # do_sample: valid ids, reproducible for the same seed
    draws = []
    for _ in range(2):
        model.sample_seed = 77
        draws.append([t.tolist() for t in model.generate_text_shared(past, qs, 12, do_sample=True, temperature=0.8)])
    assert draws[0] == draws[1]
    assert all(0 <= v[0] < dims["llm"]["vocab"] for t in draws[0] for v in t)
    assert past.length == plen

    # refused before any prefill
    ran = []
    orig = model._chat_geometry
    model._chat_geometry = lambda *a_, **k_: ran.append(1) or orig(*a_, **k_)
    for bad in (dict(prompts=[]), dict(prompts=["q"] * 65), dict(prompts=["q"], do_sample=True, temperature=0.0),
                dict(prompts=["q"], do_sample=True, temperature=-1.0)):
        with pytest.raises(ValueError):
            model.chat_with_recon_questions(tok, tok.new_token_ids, transform_over(vit_inputs(meta)), None, imgs,
                                            max_length=4, **bad)
    assert not ran
    model._chat_geometry = orig

    # bytes allocated by decode_begin_shared: independent of the prefix length (same B, same cap_s)
    from g2vlm_amd.engine import KVCache
    eng = model.engine
    L, Hkv = dims["llm"]["layers"], dims["llm"]["kv_heads"]
    sizes = []
    for n in (64, 6000):
        pre = KVCache(L, Hkv, "cuda", capacity=n)
        for i in range(L):
            pre.k[i].normal_(); pre.v[i].normal_()
        pre.length = n
        torch.cuda.synchronize()
        m0 = torch.cuda.memory_allocated()
        st = eng.decode_begin_shared(pre, [q for q, _ in qs], [1] * 3, [n + 5] * 3, 16, use_graph=False)
        torch.cuda.synchronize()
        sizes.append(torch.cuda.memory_allocated() - m0)
        eng.decode_step_batch(st)
        del st
    assert sizes[0] == sizes[1] and sizes[0] > 0, sizes


def test_full_size_questions_match_copied_prefix_batch():
    """Full width and depth (28 und layers, vocab 151 936, one 518x518 view + one ViT image) and B = 6 questions: at G = 6
    that is more slots than one 32-column group holds.  The shared decode's ids equal generate_text_batch's over copied
    prefixes at every step up to a near-tie flip (judged on the copied-prefix logits); graph replay == eager."""
    from g2vlm_amd.g2vlm_utils import build_model, configs_from_dims
    from g2vlm_amd.synthetic import REAL_DIMS, SyntheticStateDict
    dims, dev = REAL_DIMS, torch.device("cuda", 0)
    model = build_model(*configs_from_dims(dims), SyntheticStateDict(dims, dev, seed=0), dev)
    tok = synth.FakeTokenizer(dims["llm"]["vocab"])
    g = torch.Generator(); g.manual_seed(21)
    view = torch.rand((1, 3, 518, 518), generator=g)
    pv = vit_patchify(torch.randn((1, 3, 392, 392), generator=g))
    prompts = ["How far is the chair from the door?", "How big is the room?", "What is left of the door?",
               "Count the windows.", "Describe the layout of this room and count the windows you can see.", "Is the lamp on?"]

    def image_transform(_imgs):
        return pv[0], torch.tensor([list(pv[1])])
    eng, steps, B = model.engine, 10, len(prompts)
    past, qs = model.prefill_questions(tok, tok.new_token_ids, image_transform, None, view, prompts)
    plen = past.length
    # the copied-prefix reference: each question's whole cache, as chat_with_recon would have it
    full = []
    from g2vlm_amd.engine import KVCache
    for q, gi in qs:
        c = KVCache(past.num_layers, past.hkv, "cuda", capacity=plen + q.length)
        for i in range(past.num_layers):
            c.k[i][:plen].copy_(past.k[i][:plen]); c.v[i][:plen].copy_(past.v[i][:plen])
            c.k[i][plen:plen + q.length].copy_(q.k[i][:q.length]); c.v[i][plen:plen + q.length].copy_(q.v[i][:q.length])
        c.length = plen + q.length
        full.append((c, gi))
    starts = [int(gi["packed_start_tokens"][0]) for _, gi in qs]
    poss = [int(gi["packed_query_position_ids"][0, 0]) for _, gi in qs]
    ref = eng.decode_begin_batch([c for c, _ in full], starts, poss, steps, use_graph=False)
    ref_ids, ref_lg = [[t] for t in ref["tok"].tolist()], []
    for _ in range(steps):
        t = eng.decode_step_batch(ref).tolist()
        ref_lg.append(ref["logits"].float().cpu())
        for j in range(B):
            ref_ids[j].append(t[j])
    del ref
    runs = []
    for use_graph in (False, True):
        st = eng.decode_begin_shared(past, [q for q, _ in qs], starts, poss, steps, use_graph=use_graph)
        ids = [[t] for t in st["tok"].tolist()]
        alive = [True] * B
        for s in range(steps):
            t = eng.decode_step_batch(st).tolist()
            for j in range(B):
                ids[j].append(t[j])
                if alive[j] and t[j] != ref_ids[j][s + 1]:
                    assert _near_tie(ref_lg[s][j], t[j]), f"question {j} step {s}: {t[j]} vs {ref_ids[j][s + 1]}"
                    alive[j] = False
        runs.append(ids)
        del st
    assert runs[0] == runs[1], "graph replay and eager shared decode disagree"
    assert all(0 <= t < dims["llm"]["vocab"] for ids in runs[0] for t in ids)
    assert past.length == plen
