"""CPU restatement of the reference's DINOv3 encoder (modeling/dinov3/dinov3_model.py) - TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this; the product (g2vlm_amd/) never
does.  Pinned: `tests/test_oracle_golden.py::test_dinov3_oracle_matches_reference` holds it bit-exact against outputs of
the reference module itself (run in the build container by oracle/gen_golden_dinov3.py through oracle/ref_shim.py: bf16
CPU autocast standing in for CUDA autocast, flash-attn 2.7.4 - third party, absent - replaced by the fp32-softmax varlen
restatement of ref_shim, which takes the fp32 rotated q/k as they are).

Every function cites the reference lines it follows.  Arithmetic dtype: Linears / conv bf16 (fp32 accumulate), LayerNorm,
LayerScale, RoPE and the residual stream fp32 - what autocast(bf16) does to the fp32 module.
"""
import math

import torch
import torch.nn.functional as F

from oracle.g2vlm_oracle import varlen_attention


def default_config(**kw):
    """configuration_dinov3_vit.py:108-160 (the fields the forward reads)"""
    c = dict(patch_size=16, hidden_size=384, intermediate_size=1536, num_hidden_layers=12, num_attention_heads=6,
             hidden_act="gelu", layer_norm_eps=1e-5, rope_theta=100.0, query_bias=True, key_bias=False, value_bias=True,
             proj_bias=True, mlp_bias=True, layerscale_value=1.0, use_gated_mlp=False, num_register_tokens=0)
    c.update(kw)
    return c


def synth_state_dict(cfg, seed):
    """Seeded weights under the reference's parameter names (module tree of DINOv3ViTModel, :491-500).  Linear / conv
    N(0, 0.02), biases N(0, 0.02) so they matter, norms near identity, LayerScale around layerscale_value."""
    g = torch.Generator(); g.manual_seed(seed)
    C, I, ps, R = cfg["hidden_size"], cfg["intermediate_size"], cfg["patch_size"], cfg["num_register_tokens"]
    n = lambda *s, sc=0.02: torch.randn(*s, generator=g) * sc
    sd = {"embeddings.cls_token": n(1, 1, C), "embeddings.mask_token": torch.zeros(1, 1, C),
          "embeddings.register_tokens": n(1, R, C),
          "embeddings.patch_embeddings.weight": n(C, 3, ps, ps), "embeddings.patch_embeddings.bias": n(C),
          "norm.weight": 1 + n(C, sc=0.1), "norm.bias": n(C, sc=0.1)}
    for i in range(cfg["num_hidden_layers"]):
        p = f"layer.{i}."
        for nm in ("norm1", "norm2"):
            sd[p + nm + ".weight"], sd[p + nm + ".bias"] = 1 + n(C, sc=0.1), n(C, sc=0.1)
        for nm, has_b in (("q_proj", cfg["query_bias"]), ("k_proj", cfg["key_bias"]), ("v_proj", cfg["value_bias"]),
                          ("o_proj", cfg["proj_bias"])):
            sd[p + f"attention.{nm}.weight"] = n(C, C, sc=C ** -0.5)
            if has_b:
                sd[p + f"attention.{nm}.bias"] = n(C)
        sd[p + "layer_scale1.lambda1"] = cfg["layerscale_value"] * (1 + n(C, sc=0.1))
        sd[p + "layer_scale2.lambda1"] = cfg["layerscale_value"] * (1 + n(C, sc=0.1))
        names = ("gate_proj", "up_proj") if cfg["use_gated_mlp"] else ("up_proj",)
        for nm in names:
            sd[p + f"mlp.{nm}.weight"] = n(I, C, sc=C ** -0.5)
            if cfg["mlp_bias"]:
                sd[p + f"mlp.{nm}.bias"] = n(I)
        sd[p + "mlp.down_proj.weight"] = n(C, I, sc=I ** -0.5)
        if cfg["mlp_bias"]:
            sd[p + "mlp.down_proj.bias"] = n(C)
    return sd


def synth_images(n, h, w, seed):
    g = torch.Generator(); g.manual_seed(seed)
    return torch.randn((n, 3, h, w), generator=g)


class Ops:
    """The sums of the encoder, overridable as OracleG2VLM.lin / varlen are: a subclass may take them in another order or plant
    a fault (tests/dinov3_block_check.py); the defaults are the reference's.

    precise: the same graph with fp32 weights and activations and fp64 attention - the yardstick every bf16 run is measured
    against.  round_qk: the rotated q/k are rounded to bf16 before attention, which the reference does not do (it hands fp32 to
    the attention) and a real flash kernel must: the engine's one documented deviation, so its specification is round_qk=True."""

    def __init__(self, precise=False, round_qk=False):
        self.precise, self.round_qk = precise, round_qk
        self.cd = torch.float32 if precise else torch.bfloat16          # "autocast" compute dtype

    def lin(self, x, sd, name):
        """nn.Linear under autocast: bf16 operands, bf16 out"""
        b = sd.get(name + ".bias")
        return F.linear(x.to(self.cd), sd[name + ".weight"].to(self.cd), None if b is None else b.to(self.cd))

    def patch_embed(self, pixel_values, sd, ps):
        """the patch Conv2d under autocast -> [B, P, C]"""
        w, b = sd["embeddings.patch_embeddings.weight"].to(self.cd), sd["embeddings.patch_embeddings.bias"].to(self.cd)
        return F.conv2d(pixel_values.float().to(self.cd), w, b, stride=ps).flatten(2).transpose(1, 2)

    def varlen(self, q, k, v, cu):
        """flash_attn_varlen_func on the windows [cu[i], cu[i+1]); rows in no window are 0"""
        return varlen_attention(q, k, v, cu, cu, False, precise=self.precise)


BF16, PRECISE = Ops(), Ops(precise=True)


def rope_cos_sin(gh, gw, head_dim, base):
    """get_patches_center_coordinates (:72-97) + DINOv3ViTRopePositionEmbedding.forward, eval mode (:144-176)"""
    ch = torch.arange(0.5, gh, dtype=torch.float32) / gh
    cw = torch.arange(0.5, gw, dtype=torch.float32) / gw
    coords = torch.stack(torch.meshgrid(ch, cw, indexing="ij"), dim=-1).flatten(0, 1)
    coords = 2.0 * coords - 1.0
    inv_freq = 1 / base ** torch.arange(0, 1, 4 / head_dim, dtype=torch.float32)
    angles = 2 * math.pi * coords[:, :, None] * inv_freq[None, None, :]
    angles = angles.flatten(1, 2).tile(2)
    return torch.cos(angles), torch.sin(angles)


def rotate_half(x):
    """:179-183"""
    x1, x2 = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def rope_rows(cos, sin, n_prefix, n_views):
    """The [P, D] tables as one row per token of the flat [n_views * (n_prefix + P)] axis: identity rows (cos 1, sin 0) for the
    prefix tokens.  apply_rotary_pos_emb (:216-246) lets the prefix tokens pass through and rotates the patch tokens;
    t * 1 + rotate_half(t) * 0 is t, so one row-wise rotation with these tables gives the same values."""
    D = cos.shape[1]
    return (torch.cat([torch.ones(n_prefix, D), cos], 0).repeat(n_views, 1),
            torch.cat([torch.zeros(n_prefix, D), sin], 0).repeat(n_views, 1))


def rope_apply(t, cos, sin):
    """apply_rotary_pos_emb (:216-246) on [T, H, D] with per-row tables [T, D]: bf16 q/k rotate in fp32, the result is fp32"""
    cos, sin = cos[:, None, :], sin[:, None, :]
    return (t * cos) + (rotate_half(t) * sin)


def embeddings(sd, cfg, pixel_values, ops=BF16):
    """DINOv3ViTEmbeddings.forward (:51-69): conv under autocast -> bf16, cls / registers fp32, cat -> fp32"""
    pe = ops.patch_embed(pixel_values, sd, cfg["patch_size"])
    B = pixel_values.shape[0]
    return torch.cat([sd["embeddings.cls_token"].expand(B, -1, -1), sd["embeddings.register_tokens"].expand(B, -1, -1), pe], dim=1)


def layer(sd, cfg, i, x, cos, sin, cu, ops=BF16):
    """DINOv3ViTLayer.forward (:407-439) with DINOv3ViTAttention.forward (:272-317) and the MLPs (:358-385) on flat token rows
    x [T, C] with their RoPE rows cos / sin [T, D] (rope_rows).  Tokens meet only in the attention, whose windows `cu` are on
    this row axis, so any run of rows stands for the reference's [B, S, C] batch."""
    C, nh = cfg["hidden_size"], cfg["num_attention_heads"]
    eps, p = cfg["layer_norm_eps"], f"layer.{i}."
    T = x.shape[0]
    h = F.layer_norm(x.float(), (C,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps)
    q = ops.lin(h, sd, p + "attention.q_proj").view(T, nh, -1)
    k = ops.lin(h, sd, p + "attention.k_proj").view(T, nh, -1)
    v = ops.lin(h, sd, p + "attention.v_proj").view(T, nh, -1)
    q, k = rope_apply(q, cos, sin), rope_apply(k, cos, sin)
    if ops.round_qk:
        q, k = q.to(torch.bfloat16).float(), k.to(torch.bfloat16).float()
    ctx = ops.varlen(q, k, v, cu).reshape(T, -1)                              # fp32 in -> fp32 out (ref_shim convention)
    a = ops.lin(ctx, sd, p + "attention.o_proj")
    x = a * sd[p + "layer_scale1.lambda1"] + x
    h = F.layer_norm(x.float(), (C,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps)
    if cfg["use_gated_mlp"]:
        m = ops.lin(F.silu(ops.lin(h, sd, p + "mlp.gate_proj")) * ops.lin(h, sd, p + "mlp.up_proj"), sd, p + "mlp.down_proj")
    else:
        m = ops.lin(F.gelu(ops.lin(h, sd, p + "mlp.up_proj")), sd, p + "mlp.down_proj")
    return m * sd[p + "layer_scale2.lambda1"] + x


def final_norm(sd, cfg, x):
    """the model's `norm` (:536-541) on every row"""
    return F.layer_norm(x.float(), (cfg["hidden_size"],), sd["norm.weight"], sd["norm.bias"], cfg["layer_norm_eps"])


def run_layers(sd, cfg, x, cos, sin, cu, num_layers=None, ops=BF16):
    """`num_layers` layers and the final LayerNorm on flat token rows.  Returns (streams: the fp32 residual stream after each
    layer, final LayerNorm of all T rows)."""
    cu = [int(v) for v in (cu.tolist() if torch.is_tensor(cu) else cu)]
    streams = []
    for i in range(cfg["num_hidden_layers"] if num_layers is None else num_layers):
        x = layer(sd, cfg, i, x, cos, sin, cu, ops)
        streams.append(x)
    return streams, final_norm(sd, cfg, x)


def taps(sd, cfg, pixel_values, cu_seqlens, num_layers=None, ops=BF16):
    """DINOv3ViTModel.forward (:506-543) with its intermediate results: dict(embed: the token matrix after `embeddings`
    [B * S, C], streams: the residual stream after each layer, final_ln: the final LayerNorm of all B * S rows,
    patch_tokens: what the reference returns, [B, P, C])."""
    ps, R = cfg["patch_size"], cfg["num_register_tokens"]
    emb = embeddings(sd, cfg, pixel_values, ops)
    B, S, C = emb.shape
    gh, gw = pixel_values.shape[2] // ps, pixel_values.shape[3] // ps
    cos, sin = rope_rows(*rope_cos_sin(gh, gw, C // cfg["num_attention_heads"], cfg["rope_theta"]), 1 + R, B)
    x = emb.reshape(B * S, C)
    streams, out = run_layers(sd, cfg, x, cos, sin, cu_seqlens, num_layers, ops)
    return dict(embed=x, streams=streams, final_ln=out, patch_tokens=out.reshape(B, S, C)[:, 1 + R:])


def forward(sd, cfg, pixel_values, cu_seqlens, num_layers=None, precise=False):
    """DINOv3ViTModel.forward (:506-543) -> patch tokens fp32 [B, P, C]; precise: fp32 Linears, fp64 attention (Ops)"""
    return taps(sd, cfg, pixel_values, cu_seqlens, num_layers, PRECISE if precise else BF16)["patch_tokens"]
