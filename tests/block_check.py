"""Token-by-token check of the engine's blocks (g2vlm_amd/engine.py) against the precise oracle.  Helper, no tests; CPU only.

The kernels are held to fp64 one by one; this module is about what strings them together: which rows go to which expert, where
a window starts and ends, which cache row a K/V row lands in, which layer's gamma is read.  Such a slip is wrong in ONE row or
a few, and a global norm over T rows hides it.  So every row is measured on its own.

Per-row error.  Both sides of a comparison get the same fp32 block input x_in.  For a residual stream y the UPDATE
d = y - x_in is compared, e_r = |d_got[r] - d_prec[r]| / |d_prec[r]| (2-norms over the row): the stream itself, and a small
layer-scale gamma, would dilute an error of the update by |d| / |y|.  Outputs that are no residual update (a final norm, an
out-projection, K/V cache rows) are compared as they are.  Where the precise row is exactly zero the error is the absolute
|d_got[r]| and the row is listed under `absolute` in the verdict: such a row passes only if the bf16 oracle's own absolute
error covers it, which for a row that must be zero means it has to be zero.

Verdict.  b_r is the bf16 oracle's own per-row error against the precise result.  `verdict` demands
    max_r e_r <= M max_r b_r   and   median_r e_r <= M median_r b_r
and names the rows with e_r > M max_r b_r with their class (CLASSES below): first / last row of a view or window, the rows
on either side of the MoT split, CLS / register rows, H1 rows, marker / text rows, the rest.

Reference and its precision.  The precise side is OracleG2VLM(precise=True): fp32 weights and activations, fp64 attention.
Its own rounding is 2^-24 per fp32 operation; over the K <= 8960 terms of the longest dot product a pairwise / blocked fp32
sum stays below sqrt(K) 2^-24 ~ 2^-17.4 relative (and fp64 attention adds 2^-53 terms).  The bf16 flow rounds every Linear's
input, weight and output to 2^-9 relative (half an ulp of an 8-bit significand); the measured b_r are 2e-3 .. 8e-3 = 2^-9 ..
2^-7.  2^-7 / 2^-17.4 > 2^10: the reference's own error is more than 2^10 below the noise being compared.

The margin M is measured on the reference alone (tests/test_block_check_cpu.py re-measures it and asserts the constant):
the bf16 oracle's blocks are run under legitimate re-orderings of their fp32 sums (VARIANTS: every Linear's K summed in 2 /
4 / 8 chunks, attention as an fp32 online softmax over tiles of 32 / 64 / 128 keys); for each variant and case the two ratios
max e / max b and median e / median b are taken, M_TABLE holds the largest per variant and M = SLACK x the largest of all.
Nothing measured on the engine enters M.

FAULTS: a bf16 oracle with one named glue fault planted, each wrong in the way the engine's glue could be.
"""
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import dims as D, synth  # noqa: E402
from oracle.g2vlm_oracle import NaiveCache, OracleG2VLM, mrope_tables, vit_patchify  # noqa: E402

SLACK = 1.25                     # tests/test_e2e_gpu.py::SLACK: what two correct bf16 evaluations may differ by
# largest (max e / max b, median e / median b) of each re-ordering over every case of CASES and every output, measured by
# tests/test_block_check_cpu.py::test_the_margin_reproduces on the oracle alone
M_TABLE = {
    "k2": (1.109, 1.075),
    "k4": (1.063, 1.038),
    "k8": (1.063, 1.019),
    "t32": (1.064, 1.114),
    "t64": (1.116, 1.114),
    "t128": (1.116, 1.114),
}
M = 1.395
SEED = 31
PROMPT = "Reconst"               # bos + 7 bytes: the 8-row text prefix
TOK = synth.FakeTokenizer(D.TINY["llm"]["vocab"])
NT = TOK.new_token_ids


def real_dims():
    """Real widths, one layer each; no decoder block (the MoT case is all these weights are for)."""
    d = D.reduced(1, 1, 1, vocab=2048)
    d["dec"] = dict(depth=0, heads=16)
    return d


# ------------------------------------------------------------------------------------------------ per-row error and verdict
def row_errors(got, prec, x_in=None):
    """(e [T] float64, absolute [T] bool): per-row error of `got` against `prec` - of the update got - x_in where x_in is
    given - relative to the precise row's norm; absolute where that norm is exactly zero."""
    g, p = got.double().reshape(got.shape[0], -1), prec.double().reshape(prec.shape[0], -1)
    if x_in is not None:
        x = x_in.double().reshape(p.shape)
        g, p = g - x, p - x
    num, den = (g - p).norm(dim=1), p.norm(dim=1)
    absolute = den == 0
    return torch.where(absolute, num, num / den.clamp_min(1e-300)), absolute


def class_of(classes, r):
    names = [c for c, rows in classes.items() if r in rows]
    return "+".join(names) if names else "rest"


def verdict(got, bf16_ref, precise, x_in, classes, M):
    """See the module docstring.  classes: {name: iterable of rows}; a row in none of them is `rest`.
    Returns dict(ok, ratio_max, ratio_med, max_e, max_b, med_e, med_b, offenders [(row, class, e_r)], absolute [rows],
    per_class {name: (max e, max b)})."""
    e, ab = row_errors(got, precise, x_in)
    b, _ = row_errors(bf16_ref, precise, x_in)
    classes = {c: set(int(r) for r in rows) for c, rows in classes.items()}
    rel = ~ab
    out = dict(absolute=[int(r) for r in ab.nonzero().flatten()], offenders=[])
    ok = True
    if bool(ab.any()):
        lim = M * float(b[ab].max())
        for r in ab.nonzero().flatten().tolist():
            if float(e[r]) > lim:
                ok = False
                out["offenders"].append((r, class_of(classes, r) + " (absolute)", float(e[r])))
    max_e, max_b = float(e[rel].max()), float(b[rel].max())
    med_e, med_b = float(e[rel].median()), float(b[rel].median())
    ok = ok and max_e <= M * max_b and med_e <= M * med_b
    for r in (rel & (e > M * max_b)).nonzero().flatten().tolist():
        out["offenders"].append((r, class_of(classes, r), float(e[r])))
    per = {}
    T = e.numel()
    named = set().union(*classes.values()) if classes else set()
    for c, rows in list(classes.items()) + [("rest", set(range(T)) - named)]:
        idx = torch.tensor(sorted(r for r in rows if not bool(ab[r])), dtype=torch.long)
        if idx.numel():
            per[c] = (float(e[idx].max()), float(b[idx].max()))
    div = lambda a, b_: a / b_ if b_ > 0 else (0.0 if a == 0 else float("inf"))     # noqa: E731
    out.update(ok=ok, ratio_max=div(max_e, max_b), ratio_med=div(med_e, med_b), max_e=max_e, max_b=max_b, med_e=med_e, med_b=med_b,
               per_class=per)
    return out


def explain(name, v, M):
    rows = ", ".join(f"row {r} [{c}] e = {e:.3e}" for r, c, e in v["offenders"][:8])
    return (f"{name}: max e / max b = {v['ratio_max']:.2f}, median e / median b = {v['ratio_med']:.2f} (M = {M}); max b = {v['max_b']:.3e}, "
            f"median b = {v['med_b']:.3e}; offending rows: {rows or 'none (the median)'}; per class (max e, max b): "
            + ", ".join(f"{c} ({a:.2e}, {b:.2e})" for c, (a, b) in v["per_class"].items()))


# ------------------------------------------------------------------------------------------------ re-orderings and faults
def online_softmax_attention(q, k, v, tile, causal_offset=None):
    """q [H, Lq, d], k / v [H, Lk, d] fp32: softmax(q k^T / sqrt d) v as a running max / sum over tiles of `tile` keys."""
    Hh, Lq, d = q.shape
    m = torch.full((Hh, Lq, 1), float("-inf"))
    l = torch.zeros((Hh, Lq, 1))
    o = torch.zeros((Hh, Lq, v.shape[-1]))
    row = torch.arange(Lq).view(-1, 1)
    for s in range(0, k.shape[1], tile):
        sc = torch.matmul(q, k[:, s:s + tile].transpose(1, 2)) / math.sqrt(d)
        if causal_offset is not None:
            col = torch.arange(s, min(s + tile, k.shape[1])).view(1, -1)
            sc = sc.masked_fill(col > row + causal_offset, float("-inf"))
        mn = torch.maximum(m, sc.max(-1, keepdim=True).values)
        mn_safe = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
        a = torch.exp(m - mn_safe)
        p = torch.exp(sc - mn_safe)
        l = l * a + p.sum(-1, keepdim=True)
        o = o * a + torch.matmul(p, v[:, s:s + tile])
        m = mn
    return o / l


class Reordered(OracleG2VLM):
    """The bf16 oracle with its fp32 sums taken in another legitimate order: every Linear's K in `k_chunks` chunks that are
    summed one after the other, attention as an online softmax over tiles of `tile` keys.  None: the oracle's own."""

    def __init__(self, sd, dims, k_chunks=None, tile=None):
        super().__init__(sd, dims, precise=False)
        self.k_chunks, self.tile = k_chunks, tile

    def lin(self, x, name, bias=True):
        if self.k_chunks is None:
            return super().lin(x, name, bias)
        w = self.sd[name + ".weight"].to(self.cd).float()
        xb = x.to(self.cd).float()
        K = w.shape[1]
        step = -(-K // self.k_chunks)
        acc = None
        for s in range(0, K, step):
            part = F.linear(xb[..., s:s + step], w[:, s:s + step])
            acc = part if acc is None else acc + part
        if bias and name + ".bias" in self.sd:
            acc = acc + self.sd[name + ".bias"].to(self.cd).float()
        return acc.to(self.cd)

    def varlen(self, q, k, v, cu_q, cu_k, causal):
        if self.tile is None:
            return super().varlen(q, k, v, cu_q, cu_k, causal)
        out = torch.zeros_like(q)
        rep = q.shape[1] // k.shape[1]
        for i in range(len(cu_q) - 1):
            qs, qe, ks, ke = int(cu_q[i]), int(cu_q[i + 1]), int(cu_k[i]), int(cu_k[i + 1])
            if qe <= qs:
                continue
            qi = q[qs:qe].float().transpose(0, 1)
            ki = k[ks:ke].float().transpose(0, 1).repeat_interleave(rep, dim=0)
            vi = v[ks:ke].float().transpose(0, 1).repeat_interleave(rep, dim=0)
            o = online_softmax_attention(qi, ki, vi, self.tile, (ke - ks) - (qe - qs) if causal else None)
            out[qs:qe] = o.transpose(0, 1).to(q.dtype)
        return out

    def sdpa(self, q, k, v):
        if self.tile is None:
            return super().sdpa(q, k, v)
        b, h = q.shape[:2]
        o = online_softmax_attention(q.float().flatten(0, 1), k.float().flatten(0, 1), v.float().flatten(0, 1), self.tile)
        return o.view(b, h, *o.shape[1:]).to(q.dtype)


VARIANTS = {"k2": dict(k_chunks=2), "k4": dict(k_chunks=4), "k8": dict(k_chunks=8),
            "t32": dict(tile=32), "t64": dict(tile=64), "t128": dict(tile=128)}

# fault -> the case kinds it can be planted in
FAULTS = {
    "split_off_by_one": ("mot_geo",),                 # the first und row goes through the geo expert in layer 0
    "window_drops_last_key": ("dino", "dec"),         # every DINO / decoder self window one key short
    "h1_fixed": ("dino",),                            # DINO windows of P + 5 rows (window_len == P cases only)
    # the last patch of each view takes its left neighbour's 2-D position.  Decoders only (RoPE2D, base 100: the step is up to
    # 1 rad).  In the MoT the grid's w index turns the 24 slowest mRoPE pairs (theta 1e6): one step is at most 1e6^(-40/64) =
    # 1.8e-4 rad, a twentieth of a bf16 half-ulp (2^-9) - no bf16 output can show it (measured: every ratio 1.00 +- 0.05)
    "rope_pos_last_patch": ("dec",),
    "kv_row_early": ("mot_text", "mot_geo", "mot_multi"),   # the last new K/V row written one cache row early
    "wrong_layer_gamma": ("mot_geo", "dino"),         # layer 1 uses layer 0's ls1 (depth 2 only)
    "und_bias_dropped": ("mot_text", "mot_geo", "mot_multi"),   # the und group's qkv bias left out
    "context_own_view": ("dec",),                     # cross-attention onto each view's own tokens (context decoder, N > 1)
    "und_rounding_flipped": ("mot_text", "mot_geo", "mot_multi"),   # the text rows' q/k-norm rounding flag inverted
}
ROW_LOCAL = ("split_off_by_one", "window_drops_last_key", "h1_fixed", "rope_pos_last_patch", "wrong_layer_gamma", "und_bias_dropped")


def fault_applies(fault, case):
    if case["kind"] not in FAULTS[fault]:
        return False
    if fault == "h1_fixed":
        return case["window"] == "P"
    if fault == "wrong_layer_gamma":
        return case["depth"] == 2
    if fault == "context_own_view":
        return case["name"] == "global_points_decoder" and case["N"] > 1
    return True


class Faulty(OracleG2VLM):
    """The bf16 oracle with ONE glue fault planted.  Faults of a block's inputs (positions, windows, context) are planted by
    the drivers below, which ask `orc.fault`."""

    def __init__(self, sd, dims, fault):
        assert fault in FAULTS
        if fault == "wrong_layer_gamma":
            sd = dict(sd)
            sd["language_model.model.layers.1.ls1.gamma"] = sd["language_model.model.layers.0.ls1.gamma"]
            sd["dino_model.encoder.layer.1.layer_scale1.lambda1"] = sd["dino_model.encoder.layer.0.layer_scale1.lambda1"]
        super().__init__(sd, dims, precise=False)
        self.fault = fault
        self._self_attn = False

    def _layer(self, i, x, **kw):
        if self.fault == "split_off_by_one" and i == 0 and kw["mode"] == "geo":
            kw = dict(kw, geo_idx=torch.cat([kw["geo_idx"], kw["text_idx"][:1]]), text_idx=kw["text_idx"][1:])
        return super()._layer(i, x, **kw)

    def lin(self, x, name, bias=True):
        if self.fault == "und_bias_dropped" and name.rsplit(".", 1)[-1] in ("q_proj", "k_proj", "v_proj") and ".self_attn." in name:
            bias = False
        return super().lin(x, name, bias)

    def rms(self, x, name):
        if self.fault == "und_rounding_flipped" and name.rsplit(".", 1)[-1] in ("q_norm", "k_norm"):
            # und mode hands bf16 in (the normalised value is rounded to bf16), geo mode fp32 holding bf16 values (it is not)
            x = x.float() if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)
        return super().rms(x, name)

    def merge_kv(self, i, k, v, cache, query_lens, packed_query_indexes, key_values_lens, packed_key_value_indexes):
        if self.fault != "kv_row_early":
            return super().merge_kv(i, k, v, cache, query_lens, packed_query_indexes, key_values_lens, packed_key_value_indexes)
        past = cache is not None and cache.key_cache[i] is not None
        n_past = int(sum(key_values_lens)) if past else 0
        tot = n_past + int(sum(query_lens))
        mk, mv = k.new_zeros((tot,) + tuple(k.shape[1:])), v.new_zeros((tot,) + tuple(v.shape[1:]))
        if past:
            mk[packed_key_value_indexes] = cache.key_cache[i]; mv[packed_key_value_indexes] = cache.value_cache[i]
        idx = packed_query_indexes.long() - (0 if past else int(packed_query_indexes.min()))
        mk[idx[:-1]] = k[:-1]; mv[idx[:-1]] = v[:-1]
        if idx.numel() > 1:
            mk[idx[-1] - 1] = k[-1]; mv[idx[-1] - 1] = v[-1]        # one row early: over its neighbour; its own row stays empty
        return mk, mv, (key_values_lens + query_lens) if past else query_lens

    def varlen(self, q, k, v, cu_q, cu_k, causal):
        if self.fault == "window_drops_last_key" and cu_q is cu_k:             # the DINO windows
            keep = torch.ones(k.shape[0], dtype=torch.bool)
            keep[cu_k[1:].long() - 1] = False
            cu_k = cu_k - torch.arange(len(cu_k))
            k, v = k[keep], v[keep]
        return super().varlen(q, k, v, cu_q, cu_k, causal)

    def _self_attn_rope(self, x, p, pos):
        self._self_attn = True
        try:
            return super()._self_attn_rope(x, p, pos)
        finally:
            self._self_attn = False

    def sdpa(self, q, k, v):
        if self.fault == "window_drops_last_key" and self._self_attn:
            k, v = k[:, :, :-1], v[:, :, :-1]
        return super().sdpa(q, k, v)


def last_patch_left(pos2d, gw):
    """rope_pos_last_patch on [.., P, 2] (y, x) grid positions: the last patch takes (y, x - 1)."""
    pos2d = pos2d.clone()
    pos2d[..., -1, :] = pos2d[..., -2, :]
    return pos2d


# ------------------------------------------------------------------------------------------------ the cases of the GPU module
def _mot(kind, depth, dims="tiny", **kw):
    return dict(kind=kind, depth=depth, dims=dims, **kw)


def case_id(c):
    k = c["kind"]
    if k == "mot_text":
        s = f"mot_text_{c['dims']}"
    elif k == "mot_geo":
        s = f"mot_geo_{c['dims']}_{c['N']}v_{c['gh']}x{c['gw']}"
    elif k == "mot_multi":
        s = "mot_multi"
    elif k == "dino":
        s = f"dino_{c['N']}v_{c['gh']}x{c['gw']}_w{c['window']}"
    elif k == "dec":
        s = f"{c['name'].split('_')[0]}_{c['N']}v_{c['gh']}x{c['gw']}"
    else:
        s = f"vit_{c['form']}"
    return f"{s}_d{c['depth']}"


GRIDS = ((2, 3), (4, 5))          # 28 x 42 (P = 6) and 56 x 70 (P = 20)
CASES = []
for _d in (1, 2):
    CASES.append(_mot("mot_text", _d))
    for _n in (1, 2, 3):
        for _g in GRIDS:
            CASES.append(_mot("mot_geo", _d, N=_n, gh=_g[0], gw=_g[1]))
    CASES.append(_mot("mot_multi", _d, grids=((1, 4, 4), (1, 4, 6))))
CASES.append(_mot("mot_text", 1, dims="real"))
CASES.append(_mot("mot_geo", 1, dims="real", N=2, gh=2, gw=3))
for _d in (1, 2):
    for _n in (1, 2, 3):
        for _g in GRIDS:
            for _w in ("P", "all"):
                CASES.append(dict(kind="dino", depth=_d, dims="tiny", N=_n, gh=_g[0], gw=_g[1], window=_w))
    for _name in ("point_decoder", "global_points_decoder"):
        for _n in (1, 3):
            for _g in GRIDS:
                CASES.append(dict(kind="dec", depth=_d, dims="tiny", name=_name, N=_n, gh=_g[0], gw=_g[1]))
    for _form in ("two_grids", "stacked"):
        CASES.append(dict(kind="vit", depth=_d, dims="tiny", form=_form, grids=((1, 4, 4), (1, 4, 6)) if _form == "two_grids" else ((1, 4, 6),) * 2))
# recon_tiny518_2v's token count: what the global bounds of tests/test_e2e_gpu.py are set against (CPU only, faults' column b).
# No text case: the existing suite holds the text prefill's K/V to bit equality, a bound no fault passes
BIG = {"mot_geo": _mot("mot_geo", 2, N=2, gh=21, gw=37),
       "dino": dict(kind="dino", depth=2, dims="tiny", N=2, gh=21, gw=37, window="P"),
       "dec": dict(kind="dec", depth=2, dims="tiny", name="global_points_decoder", N=2, gh=21, gw=37)}

_SD = {}


def state_dict(which):
    if which not in _SD:
        dims = D.TINY if which == "tiny" else real_dims()
        _SD[which] = (synth.synth_state_dict(dims, seed=SEED, threads=1 if which == "tiny" else 8), dims)
    return _SD[which]


def vit_pixels(grid, seed):
    t, gh, gw = grid
    pv, g = vit_patchify(synth.synth_images(1, gh * 14, gw * 14, seed))
    assert tuple(g) == tuple(grid)
    return pv


# ---- drivers: one block on an oracle (precise, bf16, re-ordered or faulty), outputs in the reference's packed order
def mot_run(orc, x, query_lens, pos_ids, q_idx, cache, kv_lens, kv_idx, causal, mode, geo_idx, text_idx, depth):
    """Qwen2VLModel.forward_inference for `depth` layers (OracleG2VLM.llm_forward_inference, which returns the final norm
    only).  Returns (residual stream, routed final norm)."""
    cos, sin = mrope_tables(pos_ids, orc.dims["llm"]["theta"])
    for i in range(depth):
        x = orc._layer(i, x, cos=cos, sin=sin, query_lens=query_lens, packed_query_indexes=q_idx, cache=cache,
                       key_values_lens=kv_lens, packed_key_value_indexes=kv_idx, is_causal=causal, mode=mode, geo_idx=geo_idx,
                       text_idx=text_idx)
    p = "language_model.model."
    if mode == "und":
        return x, orc.rms(x, p + "norm")
    out = torch.zeros_like(x)
    out[text_idx] = orc.rms(x[text_idx], p + "norm")
    out[geo_idx] = orc.rms(x[geo_idx], p + "norm_moe_geo")
    return x, out


def _view_last_rows(geo_idx):
    """Last patch row of each view in the packed sequence: where the run of consecutive geo indexes ends."""
    g = geo_idx.long()
    ends = torch.cat([(g[1:] != g[:-1] + 1), torch.tensor([True])])
    return g[ends].tolist()


def _kv_outputs(out, cache, depth, first):
    for i in range(depth):
        out[f"k{i}"] = cache.key_cache[i][first:].flatten(1)
        out[f"v{i}"] = cache.value_cache[i][first:].flatten(1)


def _text_prefix(orc, inp, depth):
    gi = inp["text_gi"]
    cache = NaiveCache(orc.num_layers)
    y, fn = mot_run(orc, inp["text_x"], gi["text_token_lens"], gi["packed_text_position_ids"], gi["packed_text_indexes"], cache,
                    gi["key_values_lens"], gi["packed_key_value_indexes"], True, "und", None, None, depth)
    return cache, y, fn


def inputs(case, prec):
    """What a case's block is fed, from the precise oracle `prec` (so no error of an earlier stage is inherited), and the
    layouts from the oracle's restatement of the prepare_* methods (the GPU module asserts the model's own give the same)."""
    k = case["kind"]
    inp = {}
    if k.startswith("mot"):
        gi, nl, nr = prec.prepare_prompts([0], [0], [PROMPT], TOK, NT, bos=True)
        assert int(gi["text_token_lens"][0]) == 8
        inp.update(text_gi=gi, text_x=prec.embed_tokens(gi["packed_text_ids"]), after_text=(nl, nr))
    if k == "dec":
        # the decoders' input: the geo rows of the precise MoT prefill's last hidden state
        full = dict(case, kind="mot_geo", depth=prec.num_layers)
        minp = inputs(full, prec)
        last = run(full, prec, minp)["final_norm"]
        return dict(hidden=last[minp["gi"]["packed_dino_token_indexes"]].contiguous())
    if k in ("mot_geo", "dino"):
        imgs = synth.synth_images(case["N"], case["gh"] * 14, case["gw"] * 14, SEED)
    if k == "mot_geo":
        gi, _, _ = prec.prepare_dino_images(*inp["after_text"], imgs, NT)
        seq = prec.embed_tokens(gi["packed_text_ids"]).new_zeros((int(gi["packed_seqlens"].sum()), prec.hidden_size))
        seq[gi["packed_text_indexes"]] = prec.embed_tokens(gi["packed_text_ids"])
        cu = F.pad(torch.cumsum(gi["dino_token_seqlens"], 0), (1, 0))
        tok = prec.dino_forward(gi["packed_dino_images"], cu)
        seq[gi["packed_dino_token_indexes"]] = prec.lin(tok.reshape(-1, tok.shape[-1]), "dino2llm").float()
        inp.update(gi=gi, x=seq)
    if k == "mot_multi":
        nl, nr = inp["after_text"]
        inp["gis"], inp["xs"] = [], []
        for j, grid in enumerate(case["grids"]):
            pv = vit_pixels(grid, SEED + j)
            gi, nl, nr = prec.prepare_vit_image(nl, nr, pv, grid, NT)
            emb = prec.embed_tokens(gi["packed_text_ids"])
            seq = emb.new_zeros((int(gi["packed_seqlens"].sum()), prec.hidden_size))
            seq[gi["packed_text_indexes"]] = emb
            seq[gi["packed_vit_token_indexes"]] = prec.vit_forward(pv, grid).float()
            inp["gis"].append(gi); inp["xs"].append(seq)
    if k == "dino":
        mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1); std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
        emb = prec.dino_embeddings((imgs - mean) / std)
        inp["x"] = emb.reshape(-1, emb.shape[-1]).contiguous()
    if k == "vit":
        inp["pvs"] = [vit_pixels(g, SEED + j) for j, g in enumerate(case["grids"])]
    return inp


def dino_windows(case):
    """(n_windows, window_len) as Engine.dino_layers takes them."""
    N, P = case["N"], case["gh"] * case["gw"]
    return (N, P) if case["window"] == "P" else (1, N * (P + 5))


def run(case, orc, inp):
    """The case's block on `orc`.  Returns {output name: [rows, C]} in the reference's packed order."""
    k, depth = case["kind"], case["depth"]
    fault = getattr(orc, "fault", None)
    out = {}
    if k == "mot_text":
        cache, out["stream"], out["final_norm"] = _text_prefix(orc, inp, depth)
        _kv_outputs(out, cache, depth, 0)
    elif k == "mot_geo":
        cache, _, _ = _text_prefix(orc, inp, depth)
        gi = inp["gi"]
        out["stream"], out["final_norm"] = mot_run(orc, inp["x"], gi["packed_seqlens"], gi["packed_position_ids"], gi["packed_indexes"],
                                                   cache, gi["key_values_lens"], gi["packed_key_value_indexes"], False, "geo",
                                                   gi["packed_dino_token_indexes"], gi["packed_text_indexes"], depth)
        _kv_outputs(out, cache, depth, 8)
    elif k == "mot_multi":
        cache, _, _ = _text_prefix(orc, inp, depth)
        ys, fns = [], []
        for gi, x in zip(inp["gis"], inp["xs"]):                   # stage by stage, as the reference runs the images
            y, fn = mot_run(orc, x, gi["packed_seqlens"], gi["packed_position_ids"], gi["packed_indexes"], cache, gi["key_values_lens"],
                            gi["packed_key_value_indexes"], False, "und", None, None, depth)
            ys.append(y); fns.append(fn)
        out["stream"], out["final_norm"] = torch.cat(ys), torch.cat(fns)
        _kv_outputs(out, cache, depth, 8)
    elif k == "dino":
        N, P = case["N"], case["gh"] * case["gw"]
        nw, wl = dino_windows(case)
        if fault == "h1_fixed":
            nw, wl = N, P + 5
        cu = torch.arange(nw + 1, dtype=torch.int32) * wl
        x = inp["x"]
        for i in range(depth):
            x = orc.dino_layer(i, x, cu)
        out["stream"] = x
        out["final_ln"] = orc.ln(x, "dino_model.layernorm").to(orc.cd)
    elif k == "dec":
        N, gh, gw = case["N"], case["gh"], case["gw"]
        P = gh * gw
        hidden = inp["hidden"].reshape(N, P, -1)
        pos = torch.cartesian_prod(torch.arange(gh), torch.arange(gw)).view(1, P, 2).expand(N, -1, 2).clone()
        if fault == "rope_pos_last_patch":
            pos = last_patch_left(pos, gw)
        ctx = None
        if case["name"] == "global_points_decoder":
            ctx = hidden.clone() if fault == "context_own_view" else hidden[0:1].repeat(N, 1, 1)
        o = orc.decoder(case["name"], hidden, pos, context=ctx, depth=depth)
        out["out"] = o.reshape(N * P, -1)
    elif k == "vit":
        out["out"] = torch.cat([orc.vit_forward(pv, g, depth) for pv, g in zip(inp["pvs"], case["grids"])])
    return out


# which outputs are residual updates of which input
def x_in_of(case, inp, name):
    if name != "stream":
        return None
    k = case["kind"]
    if k == "mot_text":
        return inp["text_x"]
    if k == "mot_multi":
        return torch.cat(inp["xs"])
    return inp["x"]


def row_classes(case, inp, name):
    """{class: rows} of output `name` (rows of the output, in packed order)."""
    k = case["kind"]
    if k == "mot_text":
        return {"first_last": [0, 7]}
    if k == "mot_geo":
        gi = inp["gi"]
        text, geo = gi["packed_text_indexes"].tolist(), gi["packed_dino_token_indexes"].long()
        first = torch.cat([torch.tensor([True]), geo[1:] != geo[:-1] + 1])
        # the engine keeps geo rows first and und rows last: its rows split - 1 / split are the last patch / the first marker
        return {"special": text, "view_edge": geo[first].tolist() + _view_last_rows(geo), "split": [int(geo[-1]), text[0]]}
    if k == "mot_multi":
        sp, edge, off = [], [], 0
        for gi in inp["gis"]:
            S = int(gi["packed_seqlens"].sum())
            sp += [off + t for t in gi["packed_text_indexes"].tolist()]
            v = gi["packed_vit_token_indexes"].tolist()
            edge += [off + v[0], off + v[-1]]
            off += S
        return {"special": sp, "window_edge": edge}
    if k == "dino":
        N, P = case["N"], case["gh"] * case["gw"]
        nw, wl = dino_windows(case)
        cls = {"cls_reg": [v * (P + 5) + j for v in range(N) for j in range(5)],
               "window_edge": [w * wl + j for w in range(nw) for j in (0, wl - 1)],
               "view_edge": [v * (P + 5) + j for v in range(N) for j in (5, P + 4)]}
        if case["window"] == "P":
            cls["h1"] = list(range(N * P, N * (P + 5)))
        return cls
    if k == "dec":
        P = case["gh"] * case["gw"]
        return {"view_edge": [v * P + j for v in range(case["N"]) for j in (0, P - 1)]}
    edge, off = [], 0
    for t, gh, gw in case["grids"]:
        n = t * gh * gw // 4
        edge += [off, off + n - 1]
        off += n
    return {"image_edge": edge}


_ORACLES = {}


def oracle(which, mode, **kw):
    """Cached oracles over the shared synthetic weights: mode precise / bf16 / a VARIANTS name / a FAULTS name."""
    key = (which, mode)
    if key not in _ORACLES:
        sd, dims = state_dict(which)
        if mode in ("precise", "bf16"):
            _ORACLES[key] = OracleG2VLM(sd, dims, precise=mode == "precise")
        elif mode in VARIANTS:
            _ORACLES[key] = Reordered(sd, dims, **VARIANTS[mode])
        else:
            _ORACLES[key] = Faulty(sd, dims, mode)
    return _ORACLES[key]


_REF = {}


def reference(case):
    """(inputs, precise outputs, bf16 outputs) of a case, computed once and shared."""
    key = case_id(case)
    if key not in _REF:
        inp = inputs(case, oracle(case["dims"], "precise"))
        _REF[key] = (inp, run(case, oracle(case["dims"], "precise"), inp), run(case, oracle(case["dims"], "bf16"), inp))
    return _REF[key]


def judge(case, got, M, what="engine"):
    """verdict on every output of a case.  Returns (ok, {output: verdict}, message)."""
    inp, prec, ref = reference(case)
    res, msgs, ok = {}, [], True
    for name in prec:
        v = verdict(got[name].cpu(), ref[name], prec[name], x_in_of(case, inp, name), row_classes(case, inp, name), M)
        res[name] = v
        if not v["ok"]:
            ok = False
            msgs.append(explain(f"{case_id(case)} {name} ({what})", v, M))
    return ok, res, "\n".join(msgs)
