"""GPU, end to end: FP8 (e4m3) weight-only decode (Engine.decode_weights = "fp8", csrc/decode_fp8.hip).

The network under test is sd_q: the chat_real2_margin inputs (real widths, 2 layers, 71 steps), lm_head rows rescaled by
synth.peaked_lm_head, then every und-expert *_proj.weight and lm_head.weight replaced by dequantize(quantize(.)).
Representable input is lossless (tests/test_fp8_decode_cpu.py), so a bf16 model and an fp8 model built from sd_q are the same
network: the fp8 engine can be held to the reference's restatement (oracle/g2vlm_oracle.py) token for token with no
quantisation allowance and no near-tie escape.

Measured on an MI355X: figures in the docstrings below and in DESIGN 6e."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from oracle import synth  # noqa: E402  (checker only)
from oracle.g2vlm_oracle import OracleG2VLM  # noqa: E402
from g2vlm_amd.quant import dequantize_rows, quantize_rows_e4m3  # noqa: E402
from test_e2e_gpu import build, load, rel, run_recon  # noqa: E402
from test_shared_prefix_e2e_gpu import capture_ids, transform_over, vit_inputs  # noqa: E402

HEAD_SEED = 11        # searched on the CPU over seeds 0-24: top-1 / top-2 gap >= 10 bf16 ulp at every oracle step on sd_q, 7 distinct ids
                      # (the fixture's own head_seed 19 has a 2-ulp step once the weights are quantised)


def is_decode_weight(k):
    return k == "language_model.lm_head.weight" or (k.startswith("language_model.") and k.endswith("_proj.weight") and "_moe_geo" not in k)


def quantised(sd):
    n = 0
    for k in list(sd):
        if is_decode_weight(k):
            sd[k] = dequantize_rows(*quantize_rows_e4m3(sd[k])).float()
            n += 1
    return sd, n


def make_model(sd, dims, decode_weights):
    from g2vlm_amd.g2vlm_utils import build_model, configs_from_dims
    return build_model(*configs_from_dims(dims), dict(sd), "cuda", decode_weights=decode_weights)


def margins_in_ulp(logits):
    """per step: (top1 - top2) of the bf16 logits in units of top1's bf16 ulp"""
    top2 = logits.to(torch.bfloat16).float().topk(2, dim=-1).values
    _, e = torch.frexp(top2[:, 0].abs())
    return (top2[:, 0] - top2[:, 1]) / torch.pow(2.0, (e - 8).float())


@pytest.fixture(scope="module")
def margin(golden_dir):
    meta, _ = load(golden_dir, "chat_real2_margin")
    dims = meta["dims"]
    sd, n = quantised(synth.peaked_lm_head(synth.synth_state_dict(dims, seed=meta["seed"]), meta["head_sigma"], HEAD_SEED))
    assert n == 7 * dims["llm"]["layers"] + 1
    tok = synth.FakeTokenizer(dims["llm"]["vocab"])
    imgs = synth.synth_images(meta["n"], meta["h"], meta["w"], meta["seed"])
    return meta, dims, sd, tok, imgs


def decode_logits(model, tok, meta, imgs, steps, use_graph, force_ids=None):
    """(prefilled cache snapshot, ids, per-step logits) of a batch-1 engine decode; force_ids: feed these tokens instead of
    the step's own argmax (teacher forcing, eager only)."""
    eng = model.engine
    past, gi = model._chat_prefill(tok, tok.new_token_ids, transform_over(vit_inputs(meta)), None, imgs, meta["prompt"])
    n = past.length
    snap = [(past.k[i][:n].clone(), past.v[i][:n].clone()) for i in range(past.num_layers)]
    st = eng.decode_begin(past, int(gi["packed_start_tokens"][0]), int(gi["packed_query_position_ids"][0, 0]), steps, use_graph=use_graph)
    ids, lg = [int(st["tok"][0])], []
    for s in range(steps):
        if force_ids is not None:
            st["tok"].fill_(force_ids[s])
        ids.append(int(eng.decode_step(st)[0]))
        lg.append(st["logits"].float().cpu().clone())
    eng.decode_end(st)
    return snap, ids, lg


def test_fp8_is_token_exact_against_the_references_restatement(margin):
    """OracleG2VLM(sd_q).chat_with_recon on the CPU gives the ids; its own logits must hold a top-1 / top-2 gap >= 4 bf16 ulp
    at all 71 steps over >= 7 distinct ids before they are trusted.  The fp8 model returns exactly these ids: batch-1 graph
    replay and eager, the batched step (the scene twice around another one) and shared-prefix decode.  No near-tie escape."""
    meta, dims, sd, tok, imgs = margin
    ids, lg = OracleG2VLM(sd, dims).chat_with_recon(tok, tok.new_token_ids, imgs, vit_inputs(meta), meta["prompt"], meta["max_length"],
                                                    return_logits=True)
    m = margins_in_ulp(torch.stack(lg, 0))
    print(f"[fp8 e2e] oracle on sd_q: {len(lg)} steps, min margin {float(m.min()):.2f} ulp, {len(set(ids))} distinct ids")
    assert len(lg) >= 71 and float(m.min()) >= 4.0 and len(set(ids)) >= 7, (len(lg), float(m.min()), len(set(ids)))
    ref = [int(v) for v in ids[1:]]                           # the public entry points drop the start token

    model = make_model(sd, dims, "fp8")
    assert model.decode_weights == "fp8" and model.engine.decode_weights == "fp8"
    for use_graph in (True, False):
        model.use_decode_graph = use_graph
        dec = tok.decode
        got = capture_ids(tok)
        model.chat_with_recon(tok, tok.new_token_ids, transform_over(vit_inputs(meta)), None, images=imgs, prompt=meta["prompt"],
                              max_length=meta["max_length"])
        tok.decode = dec
        assert got[0] == ref, (use_graph, next((i for i, (a, b) in enumerate(zip(got[0], ref)) if a != b), None))
    model.use_decode_graph = True

    eos = tok.new_token_ids["eos_token_id"]
    prompts = [meta["prompt"], meta["prompt"] + " and how wide is the door", meta["prompt"]]
    pairs = [model._chat_prefill(tok, tok.new_token_ids, transform_over(vit_inputs(meta)), None, imgs, p) for p in prompts]
    outs = model.generate_text_batch([p for p, _ in pairs], [gi for _, gi in pairs], meta["max_length"], end_token_id=eos)
    for j in (0, 2):
        assert outs[j][1:, 0].tolist() == ref, ("batched", j)

    for use_graph in (True, False):
        model.use_decode_graph = use_graph
        dec = tok.decode
        got = capture_ids(tok)
        model.chat_with_recon_questions(tok, tok.new_token_ids, transform_over(vit_inputs(meta)), None, imgs, prompts, meta["max_length"])
        tok.decode = dec
        assert len(got) == 3
        for j in (0, 2):
            assert got[j] == ref, ("shared", use_graph, j)
    model.use_decode_graph = True


def test_same_network_two_encodings(margin):
    """The bf16 model on sd_q and the fp8 model on sd_q: every prefill cache row bit-identical (prefill keeps its bf16
    weights and kernels), per-step logits within rel 3e-2 (the project's bound for two decode pipelines that differ in
    summation order), identical ids.  Measured: rel 2.9e-3 median, 4.1e-3 max over 71 steps."""
    meta, dims, sd, tok, imgs = margin
    steps = meta["max_length"] - 1
    a = make_model(sd, dims, "bf16")
    b = make_model(sd, dims, "fp8")
    snap_a, ids_a, lg_a = decode_logits(a, tok, meta, imgs, steps, use_graph=False)
    snap_b, ids_b, lg_b = decode_logits(b, tok, meta, imgs, steps, use_graph=False)
    assert len(snap_a) == len(snap_b) == dims["llm"]["layers"]
    for (ka, va), (kb, vb) in zip(snap_a, snap_b):
        assert torch.equal(ka, kb) and torch.equal(va, vb)
    rels = [rel(x, y) for x, y in zip(lg_b, lg_a)]
    print(f"[fp8 e2e] same network, bf16 vs fp8 logits over {steps} steps: max rel {max(rels):.3e}, median {sorted(rels)[len(rels) // 2]:.3e}")
    assert max(rels) < 3e-2, max(rels)
    assert ids_a == ids_b


def test_nothing_else_moves(golden_dir, margin):
    """recon with the mode on is bit-identical to the mode off; switching the mode off again returns the bits of a model that
    never enabled it (the captured graph is dropped and rebuilt); decode_gen = 1 and "fp8" exclude each other."""
    meta_r, _ = load(golden_dir, "recon_real2_2v_56x84")
    model, _ = build(meta_r["dims"], meta_r["seed"])
    tok_r = synth.FakeTokenizer(meta_r["dims"]["llm"]["vocab"])
    imgs_r = synth.synth_images(meta_r["n"], meta_r["h"], meta_r["w"], meta_r["seed"])
    _, off = run_recon(model, tok_r, imgs_r)
    model.decode_weights = "fp8"
    assert "L0.und.qkv.w8" in model.weights.t and "lm_head.ws" in model.weights.t and "L0.geo.qkv.w8" not in model.weights.t
    _, on = run_recon(model, tok_r, imgs_r)
    assert set(on) == set(off)
    for k in off:
        assert torch.equal(on[k], off[k]), k

    meta, dims, sd, tok, imgs = margin
    steps = 12
    never = make_model(sd, dims, "bf16")
    _, ids0, lg0 = decode_logits(never, tok, meta, imgs, steps, use_graph=True)
    m = make_model(sd, dims, "bf16")
    m.decode_weights = "fp8"
    _, ids8, _ = decode_logits(m, tok, meta, imgs, steps, use_graph=True)
    assert any(k[-1] == "fp8" for k in m.engine._decode_cached)
    m.decode_weights = "bf16"
    assert not m.engine._decode_cached                          # the captured fp8 step is gone
    _, ids1, lg1 = decode_logits(m, tok, meta, imgs, steps, use_graph=True)
    assert ids1 == ids0 == ids8
    assert all(torch.equal(x, y) for x, y in zip(lg1, lg0))

    m.engine.decode_gen = 1
    with pytest.raises(ValueError):
        m.engine.decode_weights = "fp8"
    with pytest.raises(ValueError):
        m.decode_weights = "fp8"
    assert m.decode_weights == "bf16" and m.engine.decode_weights == "bf16"
    m.engine.decode_gen = 2
    m.decode_weights = "fp8"
    with pytest.raises(ValueError):
        m.engine.decode_gen = 1
    assert m.engine.decode_gen == 2
    with pytest.raises(ValueError):
        m.decode_weights = "int4"


def test_quantisation_error_is_what_one_expects(golden_dir):
    """The fp8 model built from the UNQUANTISED chat_real2 weights against the bf16 model on the same weights, the fp8 decode
    fed the bf16 decode's tokens.  One Linear on Gaussian weights loses 2.65e-2 rel-L2 (2^-4 / sqrt(3) x ~0.75; measured on
    the CPU at 2048 x 1536 and 1536 x 8960); with n = 4 layers + 1 Linears on the path, independent errors and a factor 2 for
    the residual path's uneven weighting, step-0 logits must satisfy rel < 2.65e-2 sqrt(n) 2 = 0.159 at 2 layers.
    Reported, not gated beyond that.  Measured: rel 4.35e-2 at step 0, 4.40e-2 median, 4.79e-2 max; the argmax agrees at 16 of 19
    steps."""
    meta, _ = load(golden_dir, "chat_real2")
    dims = meta["dims"]
    sd = synth.synth_state_dict(dims, seed=meta["seed"])
    tok = synth.FakeTokenizer(dims["llm"]["vocab"])
    imgs = synth.synth_images(meta["n"], meta["h"], meta["w"], meta["seed"])
    steps = meta["max_length"] - 1
    _, ids_a, lg_a = decode_logits(make_model(sd, dims, "bf16"), tok, meta, imgs, steps, use_graph=False)
    _, ids_b, lg_b = decode_logits(make_model(sd, dims, "fp8"), tok, meta, imgs, steps, use_graph=False, force_ids=ids_a)
    rels = [rel(y, x) for x, y in zip(lg_a, lg_b)]
    same = sum(int(x == y) for x, y in zip(ids_a[1:], ids_b[1:]))
    n = 4 * dims["llm"]["layers"] + 1
    bound = 2.65e-2 * n ** 0.5 * 2
    print(f"[fp8 e2e] quantisation error on chat_real2 ({dims['llm']['layers']} layers): logits rel-L2 step 0 {rels[0]:.3e}, "
          f"median {sorted(rels)[len(rels) // 2]:.3e}, max {max(rels):.3e}; argmax agrees at {same} of {steps} teacher-forced steps; "
          f"sanity bound {bound:.3e}")
    assert rels[0] < bound, (rels[0], bound)
