"""Row-by-row check of the DINOv3 encoder (g2vlm_amd/modeling/dinov3/dinov3_model.py) against the precise oracle
(oracle/dinov3_oracle.py), by the method of tests/block_check.py.  Helper, no tests; CPU only.

The encoder's glue is its own: the q/k/v Linears concatenated into one qkv GEMM with a zero block for the absent k bias, RoPE
rows built from patch-centre coordinates with 1 + R identity rows in front of each view, the [cls | R registers | patches] row
order, the zero-padded im2col K, windows that leave the last rows uncovered (hazard H1: those rows rely on a buffer zeroed
once), plain or gated MLP, and the [:, 1 + R:] slice of the result.  A slip in any of these is wrong in one row or a few.

Outputs of a case, each judged row by row with block_check.verdict:
  embed     the token matrix [N S, C] (S = 1 + R + P): cls / register rows must equal the fp32 parameters bit for bit, all rows
            are compared by per-row error;
  stream    the residual stream after `depth` layers; the UPDATE against the shared fp32 input x_in (the precise oracle's
            embedding) is compared;
  final_ln  the final LayerNorm of all T rows;
  forward   DINOv3ViTModel.forward's [N, P, C] from the pixels (clean and H1 windows): what a wrong [:, 1 + R:] shows in.

Yardstick.  b_r is the per-row error of the bf16 oracle with round_qk=True against the precise run (fp32 Linears, fp64
attention): the engine rounds the rotated q/k to bf16 for its attention kernel, the reference does not, and round_qk=True is
that specification.  The plain bf16 oracle's b_r is computed alongside; ROUND_QK_COST records what round_qk alone costs (the
round_qk oracle judged against the plain oracle's b_r).  The precise run's own error is below sqrt(4096) 2^-24 = 2^-18 relative
(the longest dot product here, the real-width MLP), 2^9 under the 2^-9 being compared.

Margin.  M = SLACK x the largest ratio (max e / max b, median e / median b) that the round_qk bf16 oracle shows under the six
re-orderings of its fp32 sums (VARIANTS), over every case and output.  Measured on the oracle alone by
tests/test_dinov3_block_check_cpu.py, which asserts the constants below; nothing measured on the engine enters M.

FAULTS: a round_qk bf16 oracle with ONE glue fault of a kind this model could have.
"""
import json
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from block_check import SLACK, explain, online_softmax_attention, row_errors, verdict  # noqa: E402,F401
from oracle import dinov3_oracle as O3  # noqa: E402

# largest (max e / max b, median e / median b) of each re-ordering over every case of CASES and every output, measured by
# tests/test_dinov3_block_check_cpu.py::test_the_margin_reproduces on the oracle alone
M_TABLE = {
    "k2": (1.110, 1.082),
    "k4": (1.110, 1.021),
    "k8": (1.135, 1.057),
    "t32": (1.046, 1.008),
    "t64": (1.046, 1.024),
    "t128": (1.046, 1.024),
}
M = 1.419
# the round_qk oracle judged against the PLAIN bf16 oracle's b_r: largest (max e / max b, median e / median b) over the cases
ROUND_QK_COST = (1.263, 1.164)
SEED = 31

with open(os.path.join(HERE, "golden", "dinov3_tiny.json")) as _f:
    BASE = json.load(_f)["cfg"]                       # hidden 128, 2 heads (D = 64), MLP 256, 2 layers, R = 4, patch 16
_GATED = dict(use_gated_mlp=True, hidden_act="silu", mlp_bias=False)
CONFIGS = {
    "r4": {}, "r0": dict(num_register_tokens=0),
    "r4_gated": _GATED, "r0_gated": dict(_GATED, num_register_tokens=0),
    "r4_kbias": dict(key_bias=True), "r4_noproj": dict(proj_bias=False),
    "real": dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_hidden_layers=1),
    "p14": dict(patch_size=14),                       # K = 588 -> kpad 640: the only case whose im2col pad is not empty
}
GRIDS = ((2, 3), (4, 5))                              # non-square: a transposed grid must show
WINDOWS = ("clean", "h1", "all", "shard")


def config(name):
    return dict(BASE, **CONFIGS[name])


def case_id(c):
    if c["kind"] == "embed":
        return f"{c['cfg']}_{c['N']}v_{c['gh']}x{c['gw']}_embed"
    return f"{c['cfg']}_{c['N']}v_{c['gh']}x{c['gw']}_{c['window']}_d{c['depth']}"


def _layers(cfg, N, g, depth, window):
    return dict(kind="layers", cfg=cfg, N=N, gh=g[0], gw=g[1], depth=depth, window=window)


CASES = []
for _c in ("r4", "r0", "r4_gated", "r0_gated"):
    for _g in GRIDS:
        for _n in (1, 2, 3):
            for _d in (1, 2):
                for _w in WINDOWS:
                    if _w != "shard" or _n > 1:
                        CASES.append(_layers(_c, _n, _g, _d, _w))
for _c in ("r4_kbias", "r4_noproj"):
    for _g in GRIDS:
        for _d in (1, 2):
            for _w in WINDOWS:
                CASES.append(_layers(_c, 2, _g, _d, _w))
CASES.append(_layers("real", 2, (8, 8), 1, "h1"))     # T = 138 rows at the real widths
CASES.append(dict(kind="embed", cfg="p14", N=2, gh=2, gw=3))
# 2-view cases of the golden fixtures' grids, the faults' column (b): tests/golden/dinov3_tiny (48 x 64 pixels, 12 patches a view,
# T = 34) and the largest, dinov3_real2 (224 x 224, 196 patches a view, T = 402; here at the tiny widths).  CPU only
BIG = (_layers("r4", 2, (3, 4), 2, "h1"), _layers("r4", 2, (14, 14), 2, "h1"))


# ------------------------------------------------------------------------------------------------ geometry of a case
def geom(case):
    """N, R, P, S, lo (first row of the flat [N S] axis the layers run on), T (rows they run on)."""
    cfg = config(case["cfg"])
    N, R, P = case["N"], cfg["num_register_tokens"], case["gh"] * case["gw"]
    S = 1 + R + P
    lo = S if case.get("window") == "shard" else 0
    return dict(N=N, R=R, P=P, S=S, lo=lo, T=N * S - lo)


def windows(case, fault=None):
    """cu on the row axis of the case: clean per-view windows of S; H1 windows of P (what the reference's callers pass: the
    last N (1 + R) rows uncovered); one window over all rows; `shard`: the rows of views 1.. with H1 windows counted from the
    first of them, as g2vlm_amd/sharded.py calls run_layers."""
    g = geom(case)
    w, nv = case["window"], g["T"] // g["S"]
    if w == "all":
        return [0, g["T"]]
    if w == "clean" or fault == "h1_fixed":
        return [i * g["S"] for i in range(nv + 1)]
    return [i * g["P"] for i in range(nv + 1)]


def rope(case, fault=None):
    """cos / sin rows [N S, D] of all views (the caller slices [lo:])."""
    cfg, g = config(case["cfg"]), geom(case)
    gh, gw, N, R, P = case["gh"], case["gw"], g["N"], g["R"], g["P"]
    D = cfg["hidden_size"] // cfg["num_attention_heads"]
    if fault == "rope_grid_transposed":
        gh, gw = gw, gh
    cos, sin = O3.rope_cos_sin(gh, gw, D, cfg["rope_theta"])
    if fault == "rope_not_per_view":
        # view n's grid rows are n gh .. (n + 1) gh - 1 of one tall image on view 0's scale (row centres / gh): view 0 keeps
        # its angles, the others' row coordinate runs on past 1
        ch = torch.arange(0.5, N * gh, dtype=torch.float32) / gh
        cw = torch.arange(0.5, gw, dtype=torch.float32) / gw
        coords = 2.0 * torch.stack(torch.meshgrid(ch, cw, indexing="ij"), dim=-1).flatten(0, 1) - 1.0
        inv_freq = 1 / cfg["rope_theta"] ** torch.arange(0, 1, 4 / D, dtype=torch.float32)
        ang = (2 * torch.pi * coords[:, :, None] * inv_freq[None, None, :]).flatten(1, 2).tile(2)
        one, zero = torch.ones(1 + R, D), torch.zeros(1 + R, D)
        return (torch.cat([torch.cat([one, torch.cos(ang[n * P:(n + 1) * P])]) for n in range(N)]),
                torch.cat([torch.cat([zero, torch.sin(ang[n * P:(n + 1) * P])]) for n in range(N)]))
    if fault == "prefix_rows_rotated":
        return (torch.cat([cos[:1].expand(1 + R, -1), cos]).repeat(N, 1), torch.cat([sin[:1].expand(1 + R, -1), sin]).repeat(N, 1))
    if fault == "rope_prefix_off_by_R":
        one, zero = torch.ones(1, D), torch.zeros(1, D)
        return (torch.cat([one, cos, one.expand(R, -1)]).repeat(N, 1), torch.cat([zero, sin, zero.expand(R, -1)]).repeat(N, 1))
    return O3.rope_rows(cos, sin, 1 + R, N)


# ------------------------------------------------------------------------------------------------ re-orderings and faults
class Reordered(O3.Ops):
    """The round_qk bf16 oracle with its fp32 sums in another legitimate order: every Linear's K (the patch conv's too) in
    `k_chunks` chunks summed one after the other, attention as an fp32 online softmax over tiles of `tile` keys."""

    def __init__(self, k_chunks=None, tile=None):
        super().__init__(precise=False, round_qk=True)
        self.k_chunks, self.tile = k_chunks, tile

    def _chunked(self, xb, w, b):
        K = w.shape[1]
        step = -(-K // self.k_chunks)
        acc = None
        for s in range(0, K, step):
            part = F.linear(xb[..., s:s + step], w[:, s:s + step])
            acc = part if acc is None else acc + part
        return (acc if b is None else acc + b.to(self.cd).float()).to(self.cd)

    def lin(self, x, sd, name):
        if self.k_chunks is None:
            return super().lin(x, sd, name)
        return self._chunked(x.to(self.cd).float(), sd[name + ".weight"].to(self.cd).float(), sd.get(name + ".bias"))

    def patch_embed(self, pixel_values, sd, ps):
        if self.k_chunks is None:
            return super().patch_embed(pixel_values, sd, ps)
        cols = F.unfold(pixel_values.float().to(self.cd).float(), ps, stride=ps).transpose(1, 2)        # [B, P, 3 ps ps]
        w = sd["embeddings.patch_embeddings.weight"]
        return self._chunked(cols, w.reshape(w.shape[0], -1).to(self.cd).float(), sd["embeddings.patch_embeddings.bias"])

    def varlen(self, q, k, v, cu):
        if self.tile is None:
            return super().varlen(q, k, v, cu)
        out = torch.zeros_like(q)
        for s, e in zip(cu[:-1], cu[1:]):
            if e > s:
                o = online_softmax_attention(*(t[s:e].float().transpose(0, 1) for t in (q, k, v)), self.tile)
                out[s:e] = o.transpose(0, 1).to(q.dtype)
        return out


VARIANTS = {"k2": dict(k_chunks=2), "k4": dict(k_chunks=4), "k8": dict(k_chunks=8),
            "t32": dict(tile=32), "t64": dict(tile=64), "t128": dict(tile=128)}

FAULTS = (
    "window_drops_last_key",        # every window one key short
    "h1_fixed",                     # windows of S where the caller asked for P
    "prefix_rows_rotated",          # cls / registers get the first patch's angles, not identity rows
    "rope_prefix_off_by_R",         # patch angles start after 1 row, not after 1 + R
    "rope_grid_transposed",         # gh and gw swapped
    "rope_not_per_view",            # view n > 0 continues the grid-row index of view 0
    "k_takes_v_bias",               # qkv bias [q | v | 0] for [q | 0 | v]: the zero block misplaced
    "o_bias_dropped",
    "wrong_layer_gamma",            # layer 1 reads layer 0's layer_scale1
    "uncovered_rows_stale",         # the uncovered rows keep the previous layer's attention output instead of zero
    "registers_after_patches",      # row order [cls | patches | regs]
    "output_slice_off_by_one",      # [:, R:] of the rows
)
# every one of them is wrong in some rows and right (or differently wrong) in others: none may be missed
ROW_LOCAL = FAULTS


def has(case, name):
    """Which outputs a case has."""
    if case["kind"] == "embed":
        return name == "embed"
    if name == "embed":
        return case["window"] == "clean" and case["depth"] == 1
    if name == "forward":
        return case["window"] in ("clean", "h1")
    return True


OUTPUTS = ("embed", "stream", "final_ln", "forward")


def fault_applies(fault, case):
    """Whether the fault changes anything the case computes (where it does not, the faulty run IS the clean one)."""
    cfg, g = config(case["cfg"]), geom(case)
    if fault == "registers_after_patches":
        return g["R"] > 0 and (has(case, "embed") or has(case, "forward"))
    if case["kind"] == "embed":
        return False
    w, d = case["window"], case["depth"]
    if fault == "rope_grid_transposed":
        return case["gh"] != case["gw"]               # on a square grid the swapped call builds the same table
    if fault == "rope_not_per_view":
        # the angles of a view n > 0 are read only for its patch rows that lie inside a window: under H1 the covered rows
        # [0, N P) may end before the first patch row of view 1 (N = 2, R = 4, P = 6: 12 covered rows, the row is 16)
        cu = windows(case)
        return any(cu[0] <= v * g["S"] + 1 + g["R"] + p - g["lo"] < cu[-1] for v in range(1, g["N"]) for p in range(g["P"]))
    return {"h1_fixed": w in ("h1", "shard"), "rope_prefix_off_by_R": g["R"] > 0,
            "k_takes_v_bias": not cfg["key_bias"], "o_bias_dropped": cfg["proj_bias"], "wrong_layer_gamma": d == 2,
            "uncovered_rows_stale": d == 2 and w in ("h1", "shard"), "output_slice_off_by_one": has(case, "forward")}.get(fault, True)


class Faulty(O3.Ops):
    """The round_qk bf16 oracle with ONE fault planted.  Faults of what the layers are fed (RoPE rows, windows, row order, the
    weights read, the slice) are planted by rope / windows / run, which ask `ops.fault`."""

    def __init__(self, fault):
        assert fault in FAULTS
        super().__init__(precise=False, round_qk=True)
        self.fault, self._stale = fault, None

    def begin(self):
        self._stale = None

    def lin(self, x, sd, name):
        leaf = name.rsplit(".", 1)[-1]
        if self.fault == "o_bias_dropped" and leaf == "o_proj":
            sd = {name + ".weight": sd[name + ".weight"]}
        if self.fault == "k_takes_v_bias" and leaf in ("k_proj", "v_proj"):
            vb = sd.get(name.rsplit(".", 1)[0] + ".v_proj.bias")
            sd = {name + ".weight": sd[name + ".weight"]}
            if leaf == "k_proj" and vb is not None:
                sd[name + ".bias"] = vb
        return super().lin(x, sd, name)

    def varlen(self, q, k, v, cu):
        if self.fault == "window_drops_last_key":
            out = torch.zeros_like(q)
            for s, e in zip(cu[:-1], cu[1:]):
                if e > s:
                    out[s:e] = O3.varlen_attention(q[s:e], k[s:e - 1], v[s:e - 1], [0, e - s], [0, e - s - 1], False) if e - s > 1 else 0
            return out
        out = super().varlen(q, k, v, cu)
        if self.fault == "uncovered_rows_stale":
            # a buffer that is not zeroed: the uncovered tail holds what the previous layer's attention left in the buffer, here
            # its output for the n rows in front of the tail
            n = q.shape[0] - cu[-1]
            if n > 0:
                stale, self._stale = self._stale, out[cu[-1] - n:cu[-1]].clone()
                if stale is not None:
                    out[cu[-1]:] = stale
        return out


# ------------------------------------------------------------------------------------------------ the cases
_SD, _OPS = {}, {}


def state_dict(cfg_name):
    if cfg_name not in _SD:
        _SD[cfg_name] = O3.synth_state_dict(config(cfg_name), SEED)
    return _SD[cfg_name]


def images(case, seed=SEED):
    ps = config(case["cfg"])["patch_size"]
    return O3.synth_images(case["N"], case["gh"] * ps, case["gw"] * ps, seed)


def ops(mode):
    """precise / plain (the reference's bf16 flow) / bf16 (round_qk: the engine's specification) / a VARIANTS or FAULTS name"""
    if mode not in _OPS:
        if mode in ("precise", "plain", "bf16"):
            _OPS[mode] = O3.Ops(precise=mode == "precise", round_qk=mode == "bf16")
        elif mode in VARIANTS:
            _OPS[mode] = Reordered(**VARIANTS[mode])
        else:
            _OPS[mode] = Faulty(mode)
    return _OPS[mode]


def inputs(case):
    """pixels and the layers' shared fp32 input: the rows [lo:] of the PRECISE oracle's embedding."""
    cfg = config(case["cfg"])
    img = images(case)
    emb = O3.embeddings(state_dict(case["cfg"]), cfg, img, O3.PRECISE)
    return dict(images=img, x=emb.reshape(-1, emb.shape[-1])[geom(case)["lo"]:].contiguous())


def run(case, o, inp):
    """The case on the Ops `o`.  Returns {output name: [rows, C]}."""
    cfg, g, sd = config(case["cfg"]), geom(case), state_dict(case["cfg"])
    fault = getattr(o, "fault", None)
    N, R, P, S = g["N"], g["R"], g["P"], g["S"]
    out = {}

    def embed():
        x = O3.embeddings(sd, cfg, inp["images"], o)
        if fault == "registers_after_patches":
            x = torch.cat([x[:, :1], x[:, 1 + R:], x[:, 1:1 + R]], 1)
        return x.reshape(N * S, -1)
    if has(case, "embed"):
        out["embed"] = embed()
    if case["kind"] == "embed":
        return out
    if fault == "wrong_layer_gamma":
        sd = dict(sd)
        sd["layer.1.layer_scale1.lambda1"] = sd["layer.0.layer_scale1.lambda1"]
    cos, sin = rope(case, fault)
    cu = windows(case, fault)
    begin = getattr(o, "begin", lambda: None)
    begin()
    streams, out["final_ln"] = O3.run_layers(sd, cfg, inp["x"], cos[g["lo"]:], sin[g["lo"]:], cu, case["depth"], o)
    out["stream"] = streams[-1]
    if has(case, "forward"):
        begin()
        _, ln = O3.run_layers(sd, cfg, embed(), cos, sin, cu, case["depth"], o)
        first = R if fault == "output_slice_off_by_one" else 1 + R
        out["forward"] = ln.reshape(N, S, -1)[:, first:first + P].reshape(N * P, -1)
    return out


def row_classes(case, name):
    """{class: rows} of output `name`: rows of the T-row axis for embed / stream / final_ln, of the [N P] axis for forward
    (each patch row carries the classes of its token row)."""
    g = geom(case)
    N, R, P, S, lo, T = g["N"], g["R"], g["P"], g["S"], g["lo"], g["T"]
    views = range(lo // S, N)
    cls = {"cls": [v * S - lo for v in views], "registers": [v * S + 1 + j - lo for v in views for j in range(R)],
           "view_edge": [v * S + j - lo for v in views for j in (1 + R, S - 1)]}
    if case["kind"] == "layers":
        cu = windows(case)
        cls["window_edge"] = [r for s, e in zip(cu[:-1], cu[1:]) for r in (s, e - 1)]
        cls["uncovered"] = list(range(cu[-1], T))
    if name != "forward":
        return cls
    at = {v * S + 1 + R + p: v * P + p for v in range(N) for p in range(P)}
    return {c: [at[r] for r in rows if r in at] for c, rows in cls.items() if c not in ("cls", "registers")}


def x_in_of(inp, name):
    return inp["x"] if name == "stream" else None


_REF = {}


def reference(case):
    """(inputs, precise outputs, round_qk bf16 outputs, plain bf16 outputs) of a case, computed once and shared."""
    key = case_id(case)
    if key not in _REF:
        inp = inputs(case)
        _REF[key] = (inp,) + tuple(run(case, ops(m), inp) for m in ("precise", "bf16", "plain"))
    return _REF[key]


def judge(case, got, M, what="engine", yardstick="bf16"):
    """verdict on every output of a case.  Returns (ok, {output: verdict}, message)."""
    inp, prec, rq, plain = reference(case)
    ref = rq if yardstick == "bf16" else plain
    res, msgs, ok = {}, [], True
    for name in prec:
        v = verdict(got[name].cpu(), ref[name], prec[name], x_in_of(inp, name), row_classes(case, name), M)
        if name == "embed":
            # the cls / register rows are fp32 parameters, copied: bit equality, not an error bound
            g = geom(case)
            rows = [r for c in ("cls", "registers") for r in row_classes(case, name)[c]]
            bad = [r for r in rows if not torch.equal(got[name][r].cpu().float(), prec[name][r])]
            if bad:
                v["ok"] = False
                v["offenders"] += [(r, ("cls" if r % g["S"] == 0 else "registers") + " (not the parameter's bits)", float("nan")) for r in bad]
        res[name] = v
        if not v["ok"]:
            ok = False
            msgs.append(explain(f"{case_id(case)} {name} ({what})", v, M))
    return ok, res, "\n".join(msgs)
