"""GPU: the DINOv3 encoder (g2vlm_amd/modeling/dinov3/dinov3_model.py), row by row, against the precise oracle
(tests/dinov3_block_check.py).

DINOv3ViTModel.embed, run_layers(num_layers=1 / 2) and forward(num_layers=) are called directly.  The layers' input is the
precise oracle's fp32 embedding, uploaded; cos / sin are the model's own _rope_rows, asserted equal to the oracle's tables
expanded with identity rows.  Every output row - the token matrix of embed (cls / register rows bit for bit), the residual
stream's update after `depth` layers, the final LayerNorm of all T rows, forward's [N, P, C] - is judged with
block_check.verdict at M = 1.419 x the round_qk bf16 oracle's own per-row error (M is measured on the oracle alone,
tests/test_dinov3_block_check_cpu.py).  The precise and bf16 oracles run on the host alongside.

What the cases are after: the zero block of the concatenated qkv bias (and a config with a k bias, one without a proj bias), the
RoPE rows (1 + R identity rows per view, non-square grids, per view), the [cls | registers | patches] row order with R = 0 and
4, the zero-padded im2col K (patch 14), per-view, H1, single and sharded windows - under H1 the last N (1 + R) rows are in no
window and rely on a buffer zeroed once before the layer loop (depth 2) -, plain and gated MLP, per-layer weights (depth 2),
the [:, 1 + R:] slice, and at the real widths (hidden 1024, T = 138) a qkv GEMM that is not the skinny kernel.

Also held to bit equality: a second run_layers call on the same model (cached plan and RoPE rows), and under H1 the final
LayerNorm of the uncovered rows between a depth-2 run and one whose covered rows hold other pixels.

Measured on MI355X, largest over the cases (max e / max b, median e / median b), all within M = 1.419: embed 1.000 / 1.000,
stream 1.233 / 1.123, final_ln 1.332 / 1.144, forward 1.228 / 1.087; the real-width case 1.01 / 1.00, its qkv GEMM `128x128`.
222 tests in 4.0 s, the slowest 0.5 s.  The module prints the ratios of every case and the largest per output.
"""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dinov3_block_check as B  # noqa: E402

DEV = "cuda"
RATIOS = {}
_MODELS = {}


def model_for(cfg_name):
    if cfg_name not in _MODELS:
        from g2vlm_amd.modeling.dinov3 import DINOv3ViTConfig, DINOv3ViTModel
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        _MODELS[cfg_name] = DINOv3ViTModel(DINOv3ViTConfig(**B.config(cfg_name))).load_state_dict(B.state_dict(cfg_name), DEV)
    return _MODELS[cfg_name]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    worst = {}
    for res in RATIOS.values():
        for name, (mx, md) in res.items():
            w = worst.setdefault(name, [0.0, 0.0])
            w[0], w[1] = max(w[0], mx), max(w[1], md)
    print("\n[dinov3 blocks] largest (max e / max b, median e / median b) per output: "
          + json.dumps({k: [round(x, 3) for x in v] for k, v in worst.items()}))
    _MODELS.clear()


def layers_on_engine(model, case, x_in, cos, sin):
    """run_layers on a fresh copy of x_in -> (stream, final_ln)"""
    g = B.geom(case)
    x = x_in.to(DEV).clone()
    ln = model.run_layers(x, cos[g["lo"]:].contiguous(), sin[g["lo"]:].contiguous(), B.windows(case), num_layers=case["depth"])
    return x, ln


def run_engine(case, model, inp):
    from g2vlm_amd import hip
    g = B.geom(case)
    out = {}
    if B.has(case, "embed"):
        out["embed"], gh, gw = model.embed(inp["images"])
        assert (gh, gw) == (case["gh"], case["gw"])
    if case["kind"] == "embed":
        return out
    cos, sin = model._rope_rows(g["N"], case["gh"], case["gw"])
    want_cos, want_sin = B.rope(case)
    assert torch.equal(cos.cpu(), want_cos) and torch.equal(sin.cpu(), want_sin)
    out["stream"], out["final_ln"] = layers_on_engine(model, case, inp["x"], cos, sin)
    again = layers_on_engine(model, case, inp["x"], cos, sin)              # cached plan and rope rows: the same bits
    assert torch.equal(again[0], out["stream"]) and torch.equal(again[1], out["final_ln"])
    if B.has(case, "forward"):
        out["forward"] = model.forward(inp["images"], B.windows(case), num_layers=case["depth"]).reshape(g["N"] * g["P"], -1)
    if case["cfg"] == "real":
        C, T = model.config.hidden_size, g["T"]
        h = torch.empty((T, C), dtype=torch.bfloat16, device=DEV)
        qkv = torch.empty((T, 3 * C), dtype=torch.bfloat16, device=DEV)
        route = hip.gemm_route([dict(A=h, W=model.w["0.qkv.w"], bias=model.w["0.qkv.b"], C=qkv, M=T)], 3 * C, C, hip.EPI_BF16, out_ld=3 * C)
        print(f"\n[dinov3 blocks] real widths, qkv GEMM of {T} rows -> {route}", end="")
        assert route[0] != "skinny", route
    return out


@pytest.mark.parametrize("case", B.CASES, ids=B.case_id)
def test_encoder_rows_against_the_precise_oracle(case):
    inp, prec, _, _ = B.reference(case)
    got = run_engine(case, model_for(case["cfg"]), inp)
    torch.cuda.synchronize()
    got = {k: v.float().cpu() for k, v in got.items()}
    assert set(got) == set(prec)
    for k, v in got.items():
        assert v.shape == prec[k].shape and bool(torch.isfinite(v).all()), k
    ok, res, msg = B.judge(case, got, B.M)
    RATIOS[B.case_id(case)] = {k: (v["ratio_max"], v["ratio_med"]) for k, v in res.items()}
    print(f"\n[dinov3 blocks] {B.case_id(case)}: " + ", ".join(f"{k} {v['ratio_max']:.2f} / {v['ratio_med']:.2f}" for k, v in res.items()), end="")
    assert ok, msg


H1_D2 = [c for c in B.CASES if c["kind"] == "layers" and c["window"] == "h1" and c["depth"] == 2 and c["cfg"] in ("r4", "r0_gated")]


@pytest.mark.parametrize("case", H1_D2, ids=B.case_id)
def test_an_uncovered_row_never_mixes_with_anything(case):
    """Under H1 the rows [N P, N S) are in no window: their attention output is zero in every layer, so nothing of another row
    reaches them.  With other pixels in the covered rows their final LayerNorm keeps its bits."""
    model, g = model_for(case["cfg"]), B.geom(case)
    inp = B.reference(case)[0]
    cos, sin = model._rope_rows(g["N"], case["gh"], case["gw"])
    _, ln = layers_on_engine(model, case, inp["x"], cos, sin)
    tail = g["N"] * g["P"]
    other, _, _ = model.embed(B.images(case, seed=B.SEED + 1))
    x2 = other.clone()
    x2[tail:] = inp["x"].to(DEV)[tail:]
    assert not torch.equal(x2[:tail].cpu(), inp["x"][:tail])
    _, ln2 = layers_on_engine(model, case, x2, cos, sin)
    assert torch.equal(ln2[tail:], ln[tail:]) and not torch.equal(ln2[:tail], ln[:tail])
