"""GPU: every block of g2vlm_amd/engine.py, token by token, against the precise oracle (tests/block_check.py).

The engine's block entry points - llm_forward(num_layers=), dino_layers(num_layers=), decoder(depth=), vit_forward(num_layers=)
- are called directly at depth 1 and 2 with inputs taken from the precise oracle's run, and every output row (the residual
stream's update, the routed final norm, each layer's new K/V cache rows, DINO's final LN, the decoders' out-projection, the
ViT merger's output) is compared in the reference's packed row order with block_check.verdict: max and median per-row error
against the precise oracle within M = 1.395 x the bf16 oracle's own (M is measured on the oracle alone,
tests/test_block_check_cpu.py).  The bf16 oracle runs alongside on the host.  The layouts (positions, cache rows, token and
marker indexes) come from the model's own prepare_* methods and are asserted equal to the oracle's.

What the cases are after: the `split` row of the routed norms and of groups()' A[r0:] / C[r0:] / res[r0:], kv_rows, the
per-layer ls1 / ls2 and weight names (depth 2), und_rounding, the window tuples (llm_forward's single window, its `windows`
form with two images of different grids, DINO's H1 windows whose last 5N rows get no attention, the decoders' per-view self
windows and the cross plan onto view 0), rope2d's per-view positions, and - at the real widths - the und expert reached
through the skinny GEMM (text prefill: one live group) and through the tiled two-group launch (geo prefill), asserted with
hip.gemm_route.

Measured on MI355X, largest over the cases of a block (max e / max b, median e / median b), all within M = 1.395:
  MoT 1.275 / 1.057 (18 cases), DINO 1.371 / 1.112 (24), point decoder 1.079 / 1.022 (8), global points decoder 1.010 / 1.018 (8),
  ViT 1.004 / 1.028 (4).  62 cases in 4.6 s, the slowest 0.4 s.  The module prints the ratios of every case and output.
"""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_check as B  # noqa: E402

DEV = "cuda"
RATIOS = {}


def i32(t):
    return t.to(torch.int32).contiguous().to(DEV)


@pytest.fixture(scope="module")
def tiny():
    from g2vlm_amd.g2vlm_utils import build_model, configs_from_dims
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd, dims = B.state_dict("tiny")
    return build_model(*configs_from_dims(dims), sd, DEV)


@pytest.fixture(scope="module")
def engines(tiny):
    """{"tiny": the model's engine, "real": an engine over the real-width weights (made on first use)}"""
    made = {"tiny": tiny.engine}

    def get(which):
        if which not in made:
            from g2vlm_amd.engine import Engine
            from g2vlm_amd.weights import Weights
            sd, dims = B.state_dict(which)
            made[which] = Engine(Weights(sd, dims, torch.device(DEV)), dims)
        return made[which]
    return get


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    worst = {}
    for cid, res in RATIOS.items():
        block = cid.split("_")[0] if not cid.startswith("mot") else "mot"
        w = worst.setdefault(block, [0.0, 0.0])
        w[0] = max([w[0]] + [v[0] for v in res.values()])
        w[1] = max([w[1]] + [v[1] for v in res.values()])
    print("\n[blocks] largest (max e / max b, median e / median b) per block: " + json.dumps({k: [round(x, 3) for x in v] for k, v in worst.items()}))


def same_layout(mine, theirs, keys):
    for k in keys:
        assert torch.equal(mine[k].long().cpu(), theirs[k].long().cpu()), k


def kv_rows_of(cache, depth, first, last):
    out = {}
    for i in range(depth):
        out[f"k{i}"] = cache.k[i][first:last].flatten(1).clone()
        out[f"v{i}"] = cache.v[i][first:last].flatten(1).clone()
    return out


def text_prefill(model, eng, inp, depth):
    """The 8-row causal text prefill on the und expert into an empty cache: (cache, outputs)."""
    from g2vlm_amd.decode import KVCache
    gi, nl, nr = model.prepare_prompts_addbos([0], [0], [B.PROMPT], B.TOK, B.NT)
    same_layout(gi, inp["text_gi"], ("packed_text_ids", "packed_text_position_ids", "packed_text_indexes", "text_token_lens"))
    Lc = eng.dims["llm"]
    cache = KVCache(Lc["layers"], Lc["kv_heads"], DEV)
    x = inp["text_x"].to(DEV).clone()
    fn = eng.llm_forward(x, 0, i32(gi["packed_text_position_ids"]), i32(gi["packed_text_indexes"]), cache, 0, causal=True, und_rounding=1,
                         num_layers=depth)
    assert cache.length == 8
    return cache, (nl, nr), dict(stream=x, final_norm=fn, **kv_rows_of(cache, depth, 0, 8))


def run_engine(case, model, eng, inp):
    from g2vlm_amd import hip, host
    k, depth = case["kind"], case["depth"]
    if k == "mot_text":
        return text_prefill(model, eng, inp, depth)[2]
    if k == "mot_geo":
        cache, (nl, nr), _ = text_prefill(model, eng, inp, depth)
        N, P = case["N"], case["gh"] * case["gw"]
        imgs = B.synth.synth_images(N, case["gh"] * 14, case["gw"] * 14, B.SEED)
        gi, _, _ = model.prepare_dino_images_pi3(nl, nr, imgs, None, B.NT)
        same_layout(gi, inp["gi"], ("packed_text_ids", "packed_text_indexes", "packed_dino_token_indexes", "packed_position_ids",
                                    "packed_indexes", "packed_seqlens", "key_values_lens", "dino_token_seqlens"))
        geo, text = gi["packed_dino_token_indexes"].long().cpu(), gi["packed_text_indexes"].long().cpu()
        perm = torch.cat([geo, text])                            # the engine's row order: geo rows first, und rows last
        x = inp["x"][perm].to(DEV)
        tot = 8 + perm.numel()
        fn = eng.llm_forward(x, N * P, i32(gi["packed_position_ids"].cpu()[:, perm]), i32(gi["packed_indexes"].cpu()[perm]), cache, 8,
                             causal=False, und_rounding=0, num_layers=depth)
        assert cache.length == tot
        back = lambda t: torch.empty_like(t).index_copy_(0, perm.to(DEV), t)     # noqa: E731
        if case["dims"] == "real":
            # what this case is for: the und expert's few rows ride the tiled two-group launch here and the skinny kernel
            # in the text prefill (one live group) - a two-group launch has ONE form, so the routes differ between the stages
            Lc, w = eng.dims["llm"], eng.w
            nqkv = (Lc["heads"] + 2 * Lc["kv_heads"]) * 128
            h = torch.empty((perm.numel(), Lc["hidden"]), dtype=torch.bfloat16, device=DEV)
            q = torch.empty((perm.numel(), nqkv), dtype=torch.bfloat16, device=DEV)
            grp = lambda tag, r0, m: dict(A=h[r0:], W=w[f"L0.{tag}.qkv.w"], bias=w[f"L0.{tag}.qkv.b"], C=q[r0:], M=m)   # noqa: E731
            two = hip.gemm_route([grp("geo", 0, N * P), grp("und", N * P, 2 * N)], nqkv, Lc["hidden"], hip.EPI_BF16, out_ld=nqkv)
            one = hip.gemm_route([grp("und", 0, 8)], nqkv, Lc["hidden"], hip.EPI_BF16, out_ld=nqkv)
            print(f"\n[blocks] real widths, qkv GEMM: geo + und prefill -> {two}, text prefill -> {one}", end="")
            assert one[0] == "skinny" and two[0] != "skinny", (one, two)
        return dict(stream=back(x), final_norm=back(fn), **kv_rows_of(cache, depth, 8, tot))
    if k == "mot_multi":
        cache, (nl, nr), _ = text_prefill(model, eng, inp, depth)
        wins, off = [], 0
        for gi, grid in zip(inp["gis"], case["grids"]):
            # the bookkeeping G2VLM.prepare_vit_images does for one image
            mine, nl0, nr0 = host.prepare_image_tokens(nl[0], nr[0], [grid], B.NT, merge=2)
            same_layout(mine, gi, ("packed_text_ids", "packed_text_indexes", "packed_position_ids", "packed_indexes", "packed_seqlens"))
            assert torch.equal(mine["packed_token_indexes"], gi["packed_vit_token_indexes"])
            nl, nr = [nl0], [nr0]
            S = int(gi["packed_seqlens"].sum())
            wins.append((off, S, 0, 8 + off + S, False))         # G2VLM.forward_cache_update_vit_multi's window of image j
            off += S
        x = torch.cat(inp["xs"]).to(DEV)
        fn = eng.llm_forward(x, 0, i32(torch.cat([g["packed_position_ids"] for g in inp["gis"]], -1)),
                             i32(torch.cat([g["packed_indexes"] for g in inp["gis"]])), cache, 8, causal=False, und_rounding=1,
                             num_layers=depth, windows=tuple(wins))
        return dict(stream=x, final_norm=fn, **kv_rows_of(cache, depth, 8, 8 + off))
    if k == "dino":
        x = inp["x"].to(DEV).clone()
        nw, wl = B.dino_windows(case)
        ln = eng.dino_layers(x, nw, wl, num_layers=depth)
        return dict(stream=x, final_ln=ln)
    if k == "dec":
        N, P = case["N"], case["gh"] * case["gw"]
        hidden = inp["hidden"].to(DEV)
        ctx = hidden[:P] if case["name"] == "global_points_decoder" else None
        return dict(out=eng.decoder(case["name"], hidden, N, case["gh"], case["gw"], context=ctx, depth=depth))
    V = eng.dims["vit"]
    kp = eng.w["vit.patch.w"].shape[1]
    pad = lambda pv: torch.nn.functional.pad(pv, (0, kp - pv.shape[1]))           # noqa: E731  (the host's zero-pad of K)
    rot = lambda g: host.vit_rot_pos(*g, V["embed"] // V["heads"])                # noqa: E731
    if case["form"] == "stacked":                                # two images of one grid in one pass (n_images)
        g = case["grids"][0]
        cos, sin = rot(g)
        return dict(out=eng.vit_forward(torch.cat([pad(pv) for pv in inp["pvs"]]).to(DEV), g, cos.repeat(2, 1).to(DEV), sin.repeat(2, 1).to(DEV),
                                        depth, n_images=2))
    outs = []
    for pv, g in zip(inp["pvs"], case["grids"]):                 # a pass takes one grid: two grids are two passes of one engine
        cos, sin = rot(g)
        outs.append(eng.vit_forward(pad(pv).to(DEV), g, cos.to(DEV), sin.to(DEV), depth))
    return dict(out=torch.cat(outs))


@pytest.mark.parametrize("case", B.CASES, ids=B.case_id)
def test_block_rows_against_the_precise_oracle(case, tiny, engines):
    inp, prec, ref = B.reference(case)
    with torch.no_grad():
        got = run_engine(case, tiny, engines(case["dims"]), inp)
    torch.cuda.synchronize()
    got = {k: v.float().cpu() for k, v in got.items()}
    assert set(got) == set(prec)
    for k, v in got.items():
        assert v.shape == prec[k].shape and bool(torch.isfinite(v).all()), k
    ok, res, msg = B.judge(case, got, B.M)
    RATIOS[B.case_id(case)] = {k: (v["ratio_max"], v["ratio_med"]) for k, v in res.items()}
    print(f"\n[blocks] {B.case_id(case)}: " + ", ".join(f"{k} {v['ratio_max']:.2f} / {v['ratio_med']:.2f}" for k, v in res.items()), end="")
    assert ok, msg
