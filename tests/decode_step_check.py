"""Slot-by-slot check of the decode step (g2vlm_amd/decode.py) against the precise oracle.  Helper, no tests; CPU only.

The kernels of the decode step are held to fp64 one by one; this module is about what strings them together in Decode._step,
_attention, _decode_state, _capture, decode_begin / _end, the slot API and decode_begin_shared: which length the attention gets,
which row the new K / V lands in, which position turns the rope, which layer's gammas are read, what a cached captured state
carries over.  Such a slip is wrong in one slot or one step, in bounds and finite, and greedy ids (the argmax of a logit row
whose top-1 / top-2 gap was made >= 4 bf16 ulp on purpose) do not show it.

A step is a function of a given state.  For one slot,
    (cache rows K_i, V_i [len - 1, Hkv, 128] of every layer as the engine holds them, token id, position)
      -> (logit row [V], the fp32 residual stream row before the final norm, the new K and V row of every layer).
No trajectory is ever compared: before every step the GPU module reads the engine's own tok / pos / row / len and the live cache
rows of every slot, and the oracle evaluates THAT state (`step`).  Argmax near-ties and accumulated bf16 noise cannot enter and
no teacher forcing is needed.  `step` is OracleG2VLM.llm_forward_inference in und mode with query_lens = [1] over a NaiveCache
built from the given rows, then lm_head, as generate_text does; tests/test_decode_step_check_cpu.py holds it to generate_text.

Rows of a verdict (block_check.verdict, block_check.row_errors: not copied) are the (slot, step) pairs of one case, one verdict
per output kind: `logits`, `stream` (compared as the update x - embed[tok]), `k{i}` / `v{i}` (as they are).

Reference and its precision (DESIGN 6o's argument, unchanged).  The precise side is fp32 weights and activations with fp64
attention.  Its own rounding is 2^-24 per fp32 operation; over the K <= 8960 terms of the longest dot product (down_proj) a
blocked fp32 sum stays below sqrt(8960) 2^-24 = 2^-17.4 relative; the fp64 softmax over the longest key count used here (4099
keys: kv_len 4094 + 5 new) adds 4099 2^-53 < 2^-41.  The bf16 flow rounds every Linear's input, weight and output to 2^-9
relative; the measured b_r are 2^-9 .. 2^-7.  2^-7 / 2^-17.4 > 2^10: the reference's own error is more than 2^10 below the noise
being compared.

Encodings.  decode_weights == "fp8": both oracles run on the dequantised network (quant.quantize_rows_e4m3 -> dequantize_rows of
every decode Linear; the quantiser works row by row, so it commutes with the engine's q|k|v concatenation and gate / up
interleave).  decode_kv == "fp8": the given cache is the engine's codes x scales, exactly bf16; the bf16 oracle replaces its new
K / V row by dequant(quant(row)) per kv head before attending to it (the engine attends to what it stores), the
precise oracle does not, so the e4m3 rounding of the appended row is part of b.

Margin.  M_DECODE is measured on the oracle alone (tests/test_decode_step_check_cpu.py re-measures it and asserts the
constants): the bf16 oracle's step under legitimate re-orderings of its fp32 sums (VARIANTS: every Linear's K in 2 / 4 / 8
chunks, attention as an fp32 online softmax over tiles of 32 / 64 / 128 keys, attention as 2 / 4 key splits merged by their
(max, sum) - what the split-KV core does).  Per case and output kind max e / max b and median e / median b; M_TABLE holds the
largest per re-ordering, M_DECODE = SLACK x the largest of all.  Nothing measured on the engine enters it.

FAULTS: the bf16 oracle's step with one named glue fault planted.  MISSES: the ones `verdict` cannot flag at M_DECODE, each at
most one bf16 ulp (or half an e4m3 ulp of one key) by construction.
"""
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import block_check as B  # noqa: E402
from block_check import SLACK, row_errors, verdict  # noqa: E402,F401
from g2vlm_amd.quant import dequantize_rows, quantize_rows_e4m3  # noqa: E402
from oracle import dims as D  # noqa: E402
from oracle.g2vlm_oracle import NaiveCache, OracleG2VLM, varlen_attention  # noqa: E402

# largest (max e / max b, median e / median b) of each re-ordering over every case of CASES and every output kind, measured by
# tests/test_decode_step_check_cpu.py::test_the_margin_reproduces on the oracle alone
M_TABLE = {
    "k2": (1.044, 1.057),
    "k4": (1.051, 1.022),
    "k8": (1.026, 1.026),
    "t32": (1.001, 1.011),
    "t64": (1.010, 1.000),
    "t128": (1.010, 1.000),
    "s2": (1.045, 1.007),
    "s4": (1.045, 1.011),
}
M_DECODE = 1.321
SEED = 47
LM_HEAD = "language_model.lm_head"
P = "language_model.model."


# ------------------------------------------------------------------------------------------------ e4m3 on the host
def roundtrip(x):
    """dequant(quant(x)) of cache rows x [rows, Hkv, 128], per row and kv head (g2vlm_amd/quant.py's encoding)."""
    q, s = quantize_rows_e4m3(x.reshape(-1, 128))
    return dequantize_rows(q, s).view(x.shape).to(x.dtype)


def codes_at_scale_one(x):
    """What a reader sees that takes an appended e4m3 row's codes with scale 1: x / scale(x), rounded to e4m3."""
    q, s = quantize_rows_e4m3(x.reshape(-1, 128))
    return dequantize_rows(q, torch.ones_like(s)).view(x.shape).to(x.dtype)


def is_power_of_two(s):
    """Elementwise: s is a positive normal power of two (fp32)."""
    m, _ = torch.frexp(s.detach().float().cpu())
    return (m == 0.5) & torch.isfinite(s.detach().float().cpu())


def is_decode_weight(k):
    return k == LM_HEAD + ".weight" or (k.startswith("language_model.") and k.endswith("_proj.weight") and "_moe_geo" not in k)


# ------------------------------------------------------------------------------------------------ the argmax's tie rule
def argmax_host(logits):
    """The id g2v_argmax_bf16 / _rows picks for one finite logit row (tests/imageop_check.py states the rule and holds the kernel
    to it): the largest value, -0 == +0, the LOWEST index among equals.  For finite rows that is torch.argmax on the CPU."""
    from imageop_check import argmax_emul
    return argmax_emul(logits.detach().float().cpu().numpy())


# ------------------------------------------------------------------------------------------------ re-orderings and faults
VARIANTS = {"k2": dict(k_chunks=2), "k4": dict(k_chunks=4), "k8": dict(k_chunks=8),
            "t32": dict(tile=32), "t64": dict(tile=64), "t128": dict(tile=128),
            "s2": dict(splits=2), "s4": dict(splits=4)}

# fault -> what a case must have for the fault to be planted in it (fault_applies)
FAULTS = {
    # One key among n at unit-rms keys and O(1) scores carries about 1 / n of the softmax mass, so a key too few or too many moves
    # the attention output by about 1 / n relative: at n > 256 = 2^8 that is under the bf16 half-ulp 2^-9 of the values it is
    # added to and no bf16 output can show it (measured at 4095 keys: every ratio 1.03 .. 1.11).  The length faults are planted
    # where n <= 256, i.e. in every case but the bucket edges, where `len` itself is held by the exact checks alone.
    "len_one_short": "few_keys",           # the token does not attend to its own key
    "len_one_long": "few_keys",            # it attends to the stale row behind its own as well
    "kv_row_early": "own_past",            # the new K / V row written one row early: over the last past row; its own row stays stale
    "kv_row_late": "any",                  # ... one row late: its own row stays stale and is attended to
    "pos_advanced_early": "any",           # q and the new k rotated at pos + 1
    "wrong_layer_qk_gamma": "depth2",      # layer i >= 1 reads layer 0's q_norm / k_norm
    "wrong_layer_ln": "depth2",            # ... layer 0's input / post-attention layernorm
    # the synthetic biases are 2 % of a K / V row: under an e4m3 cache the k / v verdicts cannot see that (b is the e4m3 rounding,
    # 3e-2), and at thousands of keys the one new key and a slightly moved q do not move the attention either
    "qkv_bias_dropped": "bias",
    "final_norm_gamma_of_ln2": "any",      # lm_head's norm reads the last layer's post-attention layernorm gamma
    "slot_reads_neighbour": "slots",       # slot j >= 1 attends to slot j - 1's past rows
    "prefix_last_key_dropped": "shared",
    "suffix_first_key_dropped": "shared",
    "kv8_scale_stale": "kv8",              # the appended row is read back with scale 1
    "kv8_attends_unquantised": "kv8",      # the new key / value is used before quantisation (stored quantised)
    "stale_token": "any",                  # embeds the previous step's id
    "und_rounding_flipped": "any",         # q / k-norm's rounding flag inverted
}
# Faults `verdict` does not flag at M_DECODE, with the largest ratio over their cases.  Each is at most one rounding by construction:
#   und_rounding_flipped     und mode rounds the normalised q / k to bf16 before the gamma, the flipped flag does not: the two
#                            differ by at most half a bf16 ulp (2^-9) per element BEFORE q and k are rounded to bf16 anyway after
#                            the rope, i.e. by at most one ulp of values every clean run rounds at the same place;
#   kv8_attends_unquantised  moves ONE key and one value out of len by at most half an e4m3 ulp (2^-4 relative); the stored row
#                            (what the k / v verdicts compare) is the quantised one either way.  Its weight in the output is
#                            1 / len of the softmax mass at O(1) scores.
MISSES = {"und_rounding_flipped": 1.21, "kv8_attends_unquantised": 1.05}
# no length, row, position, slot, layer or prefix fault may be missed
MUST_FLAG = ("len_one_short", "len_one_long", "kv_row_early", "kv_row_late", "pos_advanced_early", "wrong_layer_qk_gamma",
             "wrong_layer_ln", "slot_reads_neighbour", "prefix_last_key_dropped", "suffix_first_key_dropped")


def fault_applies(fault, case):
    need = FAULTS[fault]
    if need == "depth2":
        return case["dims"] == "tiny"
    if need == "slots":
        return case["family"] in ("slots", "split", "churn") and case["B"] >= 2
    if need == "shared":
        return case["family"] == "shared"
    if need == "kv8":
        return kv8(case)
    if need == "own_past":                               # every slot has a past row of its own in the block it appends to
        return case["family"] != "shared" or min(case["suffix"]) >= 1
    if need == "few_keys":
        return max_keys(case) <= 256
    if need == "bias":
        return not (kv8(case) and max_keys(case) > 256)
    return True


def max_keys(case):
    """The largest key count any step of the case attends to."""
    f = case["family"]
    if f == "shared":
        return case["plen"] + max(case["suffix"]) + case["steps"]
    if f in ("b1", "edge", "reuse"):
        return max(case.get("kv_lens", (case.get("kv_len", 0),))) + case["steps"]
    return max(n for _, n, _, _, _, _ in scenes(case)) + case["steps"]


def split_attention(q, k, v, splits):
    """q [H, 1, d], k / v [H, Lk, d] fp32: the keys in `splits` contiguous parts, each with its own max and sum, merged."""
    Lk, d = k.shape[1], q.shape[-1]
    per = -(-Lk // splits)
    ms, ls, os_ = [], [], []
    for s in range(0, Lk, per):
        sc = torch.matmul(q, k[:, s:s + per].transpose(1, 2)) / math.sqrt(d)
        m = sc.max(-1, keepdim=True).values
        p = torch.exp(sc - m)
        ms.append(m); ls.append(p.sum(-1, keepdim=True)); os_.append(torch.matmul(p, v[:, s:s + per]))
    top = torch.stack(ms).max(0).values
    l = sum(l_ * torch.exp(m - top) for l_, m in zip(ls, ms))
    o = sum(o_ * torch.exp(m - top) for o_, m in zip(os_, ms))
    return o / l


class StepOracle(OracleG2VLM):
    """The oracle of one decode step: precise, bf16, the bf16 one with its fp32 sums re-ordered (k_chunks / tile / splits) or
    with ONE glue fault planted.  kv8: the bf16 flow over an e4m3 cache (module docstring).  Converted weights are kept."""

    def __init__(self, sd, dims, precise=False, k_chunks=None, tile=None, splits=None, fault=None):
        assert fault is None or fault in FAULTS
        L = dims["llm"]["layers"]
        if fault in ("wrong_layer_qk_gamma", "wrong_layer_ln", "final_norm_gamma_of_ln2"):
            sd = dict(sd)
            for i in range(1, L):
                names = ("self_attn.q_norm", "self_attn.k_norm") if fault == "wrong_layer_qk_gamma" else \
                    ("input_layernorm", "post_attention_layernorm") if fault == "wrong_layer_ln" else ()
                for n in names:
                    sd[f"{P}layers.{i}.{n}.weight"] = sd[f"{P}layers.0.{n}.weight"]
            if fault == "final_norm_gamma_of_ln2":
                sd[P + "norm.weight"] = sd[f"{P}layers.{L - 1}.post_attention_layernorm.weight"]
        super().__init__(sd, dims, precise=precise)
        self.k_chunks, self.tile, self.splits, self.fault = k_chunks, tile, splits, fault
        self._w = {}
        self.state, self.layer, self.stream, self.late = None, 0, None, {}

    # ---- Linears: block_check.Reordered's chunked sum, on weights converted once
    def lin(self, x, name, bias=True):
        if self.fault == "qkv_bias_dropped" and name.rsplit(".", 1)[-1] in ("q_proj", "k_proj", "v_proj"):
            bias = False
        if name not in self._w:
            w = self.sd[name + ".weight"].to(self.cd)
            b = self.sd[name + ".bias"].to(self.cd) if name + ".bias" in self.sd else None
            self._w[name] = (w.float() if self.k_chunks else w, b)
        w, b = self._w[name]
        b = b if bias else None
        if self.k_chunks is None:
            return F.linear(x.to(self.cd), w, b)
        xb = x.to(self.cd).float()
        K = w.shape[1]
        per = -(-K // self.k_chunks)
        acc = None
        for s in range(0, K, per):
            part = F.linear(xb[..., s:s + per], w[:, s:s + per])
            acc = part if acc is None else acc + part
        if b is not None:
            acc = acc + b.float()
        return acc.to(self.cd)

    def rms(self, x, name):
        if name == P + "norm":
            self.stream = x.detach().clone()                 # the residual stream before the final norm
        if self.fault == "und_rounding_flipped" and name.rsplit(".", 1)[-1] in ("q_norm", "k_norm"):
            x = x.float() if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)
        return super().rms(x, name)

    def merge_kv(self, i, *a, **kw):
        self.layer = i
        return super().merge_kv(i, *a, **kw)

    # ---- attention: k / v [n + 1, Hkv, 128] are the merged tensors that BECOME the cache; row n is the new one
    def varlen(self, q, k, v, cu_q, cu_k, causal):
        s, f, i = self.state, self.fault, self.layer
        n = k.shape[0] - 1
        assert q.shape[0] == 1 and int(cu_k[-1]) == n + 1
        ak, av = k, v                                        # what is attended to; k / v: what is stored
        if s["kv8"] and not self.precise:
            if f == "kv8_attends_unquantised":
                ak, av = k.clone(), v.clone()
            rt = codes_at_scale_one if f == "kv8_scale_stale" else roundtrip
            k[n:] = rt(k[n:]); v[n:] = rt(v[n:])
        stale = lambda t, r: s[t][i][r:r + 1].to(k.dtype)    # noqa: E731  (rows behind the live length: block rows n, n + 1)
        if f == "len_one_short":
            ak, av = ak[:n], av[:n]
        elif f == "len_one_long":
            ak, av = torch.cat([ak, stale("behind_k", 1)]), torch.cat([av, stale("behind_v", 1)])
        elif f == "kv_row_early":
            k[n - 1] = k[n]; v[n - 1] = v[n]
            k[n:] = stale("behind_k", 0); v[n:] = stale("behind_v", 0)
        elif f == "kv_row_late":
            self.late[i] = (k[n].clone(), v[n].clone())      # lands in row n + 1, which this step does not read
            k[n:] = stale("behind_k", 0); v[n:] = stale("behind_v", 0)
        elif f in ("prefix_last_key_dropped", "suffix_first_key_dropped"):
            drop = s["plen"] - 1 if f == "prefix_last_key_dropped" else s["plen"]
            keep = torch.arange(n + 1) != drop
            ak, av = ak[keep], av[keep]
        cu = torch.tensor([0, ak.shape[0]], dtype=cu_k.dtype)
        if self.tile is None and self.splits is None:
            return varlen_attention(q, ak, av, cu_q, cu, causal, precise=self.precise)
        rep = q.shape[1] // ak.shape[1]
        qi = q.float().transpose(0, 1)
        ki = ak.float().transpose(0, 1).repeat_interleave(rep, dim=0)
        vi = av.float().transpose(0, 1).repeat_interleave(rep, dim=0)
        o = B.online_softmax_attention(qi, ki, vi, self.tile) if self.tile else split_attention(qi, ki, vi, self.splits)
        return o.transpose(0, 1).to(q.dtype)


def step(orc, state, keep_cache=False):
    """One decode step of `orc` on `state` (see `make_state`).  Returns dict(logits [V] fp32, stream [H] fp32, emb [H] fp32,
    k [L, Hkv * 128], v [L, Hkv * 128] fp32, tok: the greedy id; cache: the NaiveCache after the step if keep_cache)."""
    f = orc.fault
    K, V = state["K"], state["V"]
    if f == "slot_reads_neighbour" and state.get("neighbour") is not None:
        K, V = state["neighbour"]["K"], state["neighbour"]["V"]
    n = K[0].shape[0]
    L = orc.num_layers
    cache = NaiveCache(L)
    if n:
        for i in range(L):
            cache.key_cache[i], cache.value_cache[i] = K[i].to(orc.cd), V[i].to(orc.cd)
    tok = state["prev_tok"] if f == "stale_token" else state["tok"]
    pos = state["pos"] + (1 if f == "pos_advanced_early" else 0)
    orc.state = state
    x = orc.embed_tokens(torch.tensor([tok], dtype=torch.long))
    h = orc.llm_forward_inference(x, torch.tensor([1], dtype=torch.int), torch.full((3, 1), pos, dtype=torch.long), torch.tensor([n]),
                                  cache, torch.tensor([n], dtype=torch.int), torch.arange(n), True, "und")
    logits = orc.lin(h, LM_HEAD, bias=False)
    orc.state = None
    return dict(logits=logits[0].float(), stream=orc.stream[0].float(), emb=orc.embed_tokens(torch.tensor([state["tok"]]))[0].float(),
                k=torch.stack([cache.key_cache[i][n].flatten().float() for i in range(L)]),
                v=torch.stack([cache.value_cache[i][n].flatten().float() for i in range(L)]),
                tok=int(torch.argmax(logits[0].float())), cache=cache if keep_cache else None)


def make_state(tok, pos, K, V, behind_k, behind_v, kv8=False, plen=0, prev_tok=0, slot=0, stepno=0):
    """One slot's state before a step.  K / V: per layer bf16 [n, Hkv, 128], every row the slot's attention may read besides the
    new one (a shared prefix first); behind_k / behind_v: per layer [2, Hkv, 128], the rows of the block at and after the one
    the step appends to, as they are before it (stale content)."""
    return dict(tok=int(tok), pos=int(pos), K=K, V=V, behind_k=behind_k, behind_v=behind_v, kv8=bool(kv8), plen=int(plen),
                prev_tok=int(prev_tok), slot=int(slot), step=int(stepno), neighbour=None)


# ------------------------------------------------------------------------------------------------ the cases
def _c(family, dims="tiny", gen=2, graph=True, weights="bf16", kv="bf16", steps=5, **kw):
    return dict(family=family, dims=dims, gen=gen, graph=graph, weights=weights, kv=kv, steps=steps, **kw)


def kv8(case):
    """Whether the case's state keeps an e4m3 cache: decode_kv == "fp8", except under a shared prefix (without effect there)."""
    return case["kv"] == "fp8" and case["family"] != "shared"


def weights_q(case):
    """Whether the case's Linears read e4m3 weights: decode_weights == "fp8", gen 2, and at most 8 slots."""
    return case["weights"] == "fp8" and case["gen"] == 2 and case["B"] <= 8


def case_id(c):
    mode = f"g{c['gen']}{'G' if c['graph'] else 'E'}_w{'8' if c['weights'] == 'fp8' else '16'}k{'8' if c['kv'] == 'fp8' else '16'}"
    f = c["family"]
    if f in ("b1", "edge"):
        s = f"{f}_kv{c['kv_len']}"
    elif f == "reuse":
        s = "reuse_" + "_".join(str(n) for n in c["kv_lens"])
    elif f == "shared":
        s = f"shared_B{c['B']}_p{c['plen']}"
    else:
        s = f"{f}_B{c['B']}_cap{c['cap_rows']}"
    return f"{s}_{c['dims']}_{mode}"


def _lens(B_):
    """Scene lengths of different sizes per slot around the 64-row tile."""
    return [1, 64, 70, 63, 65, 2, 33, 69, 17][:B_]


CASES = []
# batch 1 through decode_begin: every kv_len on the persistent-grid graph path, every mode at kv_len 65
for _n in (1, 63, 64, 65):
    CASES.append(_c("b1", B=1, kv_len=_n))
    CASES.append(_c("b1", B=1, kv_len=_n, kv="fp8"))
for _kw in (dict(gen=1, graph=False), dict(gen=1), dict(graph=False), dict(weights="fp8"), dict(graph=False, kv="fp8"),
            dict(weights="fp8", kv="fp8")):
    CASES.append(_c("b1", B=1, kv_len=65, **_kw))
CASES.append(_c("b1", B=1, kv_len=1, gen=1, graph=False))
for _kw in (dict(gen=1, graph=False), dict(), dict(weights="fp8", kv="fp8")):
    CASES.append(_c("b1", "real", B=1, kv_len=65, **_kw))
# bucket edges: the appended rows end at row 4094 of the 4096 bucket; the 8192 bucket with the new keys crossing row 4096
for _n in (4090, 4094):
    for _kw in (dict(), dict(gen=1, graph=False), dict(kv="fp8")):
        CASES.append(_c("edge", B=1, kv_len=_n, **_kw))
# two answers through ONE cached captured state
CASES.append(_c("reuse", B=1, kv_lens=(200, 37), positions=(211, 90), steps=4))
CASES.append(_c("reuse", B=1, kv_lens=(200, 37), positions=(211, 90), steps=4, kv="fp8"))
# slots: cap_rows no multiple of 64 (100 -> 128 rows per block); the LAST slot but one ends on its block's last usable row
for _kw in (dict(B=2), dict(B=2, gen=1, graph=False), dict(B=8, weights="fp8"), dict(B=8, kv="fp8"), dict(B=8, gen=1),
            dict(B=8, graph=False), dict(B=9, weights="fp8"), dict(B=9, graph=False, kv="fp8"), dict(B=9, gen=1, graph=False),
            dict(B=2, dims="real", weights="fp8"), dict(B=9, dims="real", steps=4)):
    CASES.append(_c("slots", cap_rows=100, **_kw))
# gen 1, B * ((rows // 64 + 3) // 4) * Hkv > 512: qknorm_mrope_cache + decode_attn_batch; and its twin just under the switch
CASES.append(_c("split", B=9, gen=1, graph=False, cap_rows=14400, steps=4))
CASES.append(_c("split", B=9, gen=1, cap_rows=14400, steps=4))
CASES.append(_c("split", B=9, gen=1, cap_rows=14336, steps=4))
# slot churn under a captured graph: slot 1 idled after step 2, another scene set into it before step 4
CASES.append(_c("churn", B=3, cap_rows=100, steps=6))
CASES.append(_c("churn", B=3, cap_rows=100, steps=6, kv="fp8"))
# shared prefix; suffix 0 is the shortest the API accepts (a reserved, empty KVCache); decode_kv = "fp8" is without effect
for _kw in (dict(B=2, plen=1), dict(B=2, plen=63, graph=False, gen=1), dict(B=8, plen=64, weights="fp8"),
            dict(B=8, plen=65, graph=False, kv="fp8"), dict(B=9, plen=65, gen=1), dict(B=9, plen=64, graph=False),
            dict(B=2, plen=65, dims="real")):
    _b = _kw["B"]
    CASES.append(_c("shared", suffix=tuple(([0, 7, 1, 64, 3, 63, 5, 65, 2] if _b > 2 else [1, 6])[:_b]), steps=4, **_kw))

FAMILIES = ("b1", "edge", "reuse", "slots", "split", "churn", "shared")


def cap_of(case):
    """Rows per slot block as decode.py sizes it."""
    f = case["family"]
    if f in ("b1", "edge", "reuse"):
        need = max(case.get("kv_lens", (case.get("kv_len", 0),))) + case["steps"] + 1
        return (need + 4095) // 4096 * 4096
    if f == "shared":
        return (max(case["suffix"]) + case["steps"] + 1 + 63) // 64 * 64
    return (case["cap_rows"] + 63) // 64 * 64


def scenes(case):
    """[(slot, kv_len, start token, position, first step, seed)] the scenes a case decodes, in the order they enter."""
    f, B_, S = case["family"], case["B"], case["steps"]
    V = dims_of(case)["llm"]["vocab"]
    tk = lambda j: (37 * j + 11) % V                         # noqa: E731
    if f in ("b1", "edge"):
        return [(0, case["kv_len"], tk(0), case["kv_len"] + 3, 0, 0)]
    if f == "reuse":
        return [(0, n, tk(a), p, a * S, a) for a, (n, p) in enumerate(zip(case["kv_lens"], case["positions"]))]
    if f == "shared":
        return [(j, n, tk(j), case["plen"] + n + 2 + j, 0, j) for j, n in enumerate(case["suffix"])]
    lens = _lens(B_)
    if f in ("slots", "churn"):                              # one slot ends on its block's last usable row: the next slot's row 0 is adjacent
        lens[0 if f == "churn" else B_ - 2] = cap_of(case) - S - 1
    out = [(j, n, tk(j), n + 5 + j, 0, j) for j, n in enumerate(lens)]
    if f == "churn":
        out.append((1, 9, tk(7), 40, 4, 99))                 # the scene that enters slot 1 before step 4
    return out


def dims_of(case):
    return D.TINY if case["dims"] == "tiny" else B.real_dims()


_VS = {}


def v_sigma(which):
    """The scale of a normed projection: std of layer 0's v_proj over 64 normed token embeddings."""
    if which not in _VS:
        orc = oracle(which, False, "bf16")
        x = orc.embed_tokens(torch.arange(64))
        _VS[which] = float(orc.lin(orc.rms(x, P + "layers.0.input_layernorm"), P + "layers.0.self_attn.v_proj").float().std())
    return _VS[which]


def synth_rows(case, seed, n, what):
    """Seeded synthetic cache rows bf16 [L, n, Hkv, 128]: K rows of unit rms per head (scaled scores O(1), no key carries the
    softmax), V rows at the scale of a normed projection.  `what`: "k" or "v"."""
    Lc = dims_of(case)["llm"]
    g = torch.Generator().manual_seed(SEED * 1000003 + seed * 101 + (0 if what == "k" else 1))
    t = torch.randn((Lc["layers"], n, Lc["kv_heads"], 128), generator=g)
    if what == "k":
        t = t / t.pow(2).mean(-1, keepdim=True).sqrt()
    else:
        t = t * v_sigma(case["dims"])
    return t.to(torch.bfloat16)


def scene_rows(case, seed, n):
    """(K, V) bf16 [L, n + steps + 2, Hkv, 128] of a scene: n live rows, then the stale rows the test pre-fills behind them."""
    m = n + case["steps"] + 2
    return synth_rows(case, seed, m, "k"), synth_rows(case, seed, m, "v")


def prefix_rows(case):
    """(K, V) bf16 [L, plen + 2, Hkv, 128] of a shared prefix: plen live rows and two stale ones behind them."""
    return synth_rows(case, 777, case["plen"] + 2, "k"), synth_rows(case, 777, case["plen"] + 2, "v")


def link_neighbours(states):
    """states: the live slots' states of ONE step.  Gives each its left neighbour (slot_reads_neighbour)."""
    by = {s["slot"]: s for s in states}
    for s in states:
        s["neighbour"] = by.get(s["slot"] - 1)
    return states


def live_slots(case, t):
    """Slots under the verdict at step t."""
    if case["family"] == "churn" and t in (2, 3):
        return [0, 2]
    return list(range(case["B"]))


def synth_record(case):
    """The states of a case with no engine: the synthetic scenes rolled forward by the bf16 oracle (each new row appended as the
    engine would store it, the greedy id fed back).  Only a source of states: every one is then evaluated on its own."""
    orc = oracle(case["dims"], weights_q(case), "bf16")
    L = orc.num_layers
    q8 = kv8(case)
    rt = roundtrip if q8 else (lambda t: t)
    pk, pv = prefix_rows(case) if case["family"] == "shared" else (None, None)
    plen = case.get("plen", 0)
    slots, rec = {}, []
    sc = scenes(case)
    T = case["steps"] * (2 if case["family"] == "reuse" else 1)
    for t in range(T):
        for (j, n, tok, pos, first, seed) in sc:
            if first == t:
                K, V = scene_rows(case, seed, n)
                slots[j] = dict(K=rt(K[:, :n]), V=rt(V[:, :n]), stale_k=rt(K[:, n:]), stale_v=rt(V[:, n:]), tok=tok, pos=pos, prev=0, t0=t)
        states = []
        for j in live_slots(case, t):
            s = slots[j]
            a = t - s["t0"]                                  # rows appended so far
            own_k, own_v = s["K"], s["V"]
            if plen:
                own_k, own_v = torch.cat([pk[:, :plen], own_k], 1), torch.cat([pv[:, :plen], own_v], 1)
            states.append(make_state(s["tok"], s["pos"], list(own_k), list(own_v), list(s["stale_k"][:, a:a + 2]), list(s["stale_v"][:, a:a + 2]),
                                     q8, plen, s["prev"], j, t))
        link_neighbours(states)
        rec.append(states)
        for st_ in states:
            o = step(orc, st_)
            s = slots[st_["slot"]]
            hk = dims_of(case)["llm"]["kv_heads"]
            s["K"] = torch.cat([s["K"], o["k"].view(L, 1, hk, 128).to(torch.bfloat16)], 1)
            s["V"] = torch.cat([s["V"], o["v"].view(L, 1, hk, 128).to(torch.bfloat16)], 1)
            s["prev"], s["tok"], s["pos"] = s["tok"], o["tok"], s["pos"] + 1
    return rec


# ------------------------------------------------------------------------------------------------ oracles, references, verdicts
_SDQ, _ORACLES, _REC, _REF = {}, {}, {}, {}


def state_dict(which, quantised):
    sd, dims = B.state_dict(which)
    if not quantised:
        return sd, dims
    if which not in _SDQ:
        _SDQ[which] = {k: (dequantize_rows(*quantize_rows_e4m3(v)).float() if is_decode_weight(k) else v) for k, v in sd.items()}
    return _SDQ[which], dims


def oracle(which, quantised, mode):
    """Cached step oracles: mode precise / bf16 / a VARIANTS name / a FAULTS name, on the (de)quantised network."""
    key = (which, bool(quantised), mode)
    if key not in _ORACLES:
        sd, dims = state_dict(which, quantised)
        kw = dict(precise=True) if mode == "precise" else {} if mode == "bf16" else VARIANTS[mode] if mode in VARIANTS else dict(fault=mode)
        _ORACLES[key] = StepOracle(sd, dims, **kw)
    return _ORACLES[key]


def run(case, mode, rec):
    """Every recorded state of `rec` through the oracle `mode`.  Returns {kind: [rows, C]} with rows in (step, slot) order."""
    orc = oracle(case["dims"], weights_q(case), mode)
    outs = [step(orc, s) for states in rec for s in states]
    L = orc.num_layers
    res = dict(logits=torch.stack([o["logits"] for o in outs]), stream=torch.stack([o["stream"] for o in outs]))
    for i in range(L):
        res[f"k{i}"] = torch.stack([o["k"][i] for o in outs])
        res[f"v{i}"] = torch.stack([o["v"][i] for o in outs])
    res["emb"] = torch.stack([o["emb"] for o in outs])
    return res


def rows_of(rec):
    """[(slot, step)] of the verdict's rows."""
    return [(s["slot"], s["step"]) for states in rec for s in states]


def row_classes(rec):
    cls = {}
    for r, (j, t) in enumerate(rows_of(rec)):
        cls.setdefault(f"slot {j}", []).append(r)
        cls.setdefault(f"step {t}", []).append(r)
    return cls


def reference(case, rec=None):
    """(rec, precise outputs, bf16 outputs).  Without `rec` the synthetic record of the case, computed once and shared."""
    if rec is not None:
        return rec, run(case, "precise", rec), run(case, "bf16", rec)
    key = case_id(case)
    if key not in _REF:
        r = synth_record(case)
        _REF[key] = (r, run(case, "precise", r), run(case, "bf16", r))
    return _REF[key]


def judge(case, got, ref3, M, what="engine"):
    """verdict on every output kind.  got: {kind: [rows, C]}.  Returns (ok, {kind: verdict}, message)."""
    rec, prec, ref = ref3
    cls = row_classes(rec)
    res, msgs, ok = {}, [], True
    for name in prec:
        if name == "emb":
            continue
        v = verdict(got[name].float().cpu(), ref[name], prec[name], prec["emb"] if name == "stream" else None, cls, M)
        res[name] = v
        if not v["ok"]:
            ok = False
            msgs.append(B.explain(f"{case_id(case)} {name} ({what})", v, M)
                        + "; rows (slot, step): " + ", ".join(str(rows_of(rec)[r]) for r, _, _ in v["offenders"][:8]))
    return ok, res, "\n".join(msgs)


def worst(res):
    return max(v["ratio_max"] for v in res.values()), max(v["ratio_med"] for v in res.values())


# ------------------------------------------------------------------------------------------------ the exact checks
def touched_rows(before, after, allowed, row_dims):
    """Rows of a cache tensor (any dtype; its first `row_dims` dims flattened are the rows) whose BITS differ between `before`
    and `after`, other than the rows in `allowed`.  Compared where the tensors live (on the device)."""
    rows = math.prod(before.shape[:row_dims])
    as_int = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[before.element_size()]
    b, a = (t.contiguous().view(as_int).reshape(rows, -1) for t in (before, after))
    diff = (b != a).any(dim=1)
    if len(allowed):
        diff[torch.as_tensor(sorted(allowed), dtype=torch.long, device=diff.device)] = False
    return diff.nonzero().flatten().tolist()


def advanced(before, after, what):
    """pos / row / len are each one more than before (int tensors)."""
    assert torch.equal(after.cpu(), before.cpu() + 1), (what, before.tolist(), after.tolist())


def id_flips(fault, golden_dir, steps=None):
    """The id-flip column of DESIGN 6r: the fault planted in the bf16 oracle's greedy decode over chat_real2_margin (network,
    prefill and step count of the token-exact e2e tests; the e4m3-cache faults against the clean decode over an e4m3 cache with
    tests/test_kv8_e2e_gpu.py's lm_head seed).  Returns (first step whose id differs from the clean run's or None, steps).
    A trajectory, unlike everything above: the decode runs in a block whose rows behind the live length hold stale synthetic
    rows, every step writes where the fault says, and the ids are fed back.  Slot and prefix faults have no batch-1 form."""
    import json
    from oracle import synth
    from oracle.g2vlm_oracle import vit_patchify
    q8 = FAULTS[fault] == "kv8"
    if ("flip", q8) not in _REF:
        with open(os.path.join(golden_dir, "chat_real2_margin.json")) as f:
            meta = json.load(f)
        dims = meta["dims"]
        sd = synth.peaked_lm_head(synth.synth_state_dict(dims, seed=meta["seed"]), meta["head_sigma"], 11 if q8 else meta["head_seed"])
        tok = synth.FakeTokenizer(dims["llm"]["vocab"])
        imgs = synth.synth_images(meta["n"], meta["h"], meta["w"], meta["seed"])
        vit = []
        for i in range(meta["n"]):
            gen = torch.Generator(); gen.manual_seed(1234 + i)
            vit.append(vit_patchify(torch.randn((1, 3, meta["vit_grid"][0] * 14, meta["vit_grid"][1] * 14), generator=gen)))
        pre = OracleG2VLM(sd, dims).chat_prefill(tok, tok.new_token_ids, imgs, vit, meta["prompt"])
        _REF[("flip", q8)] = [sd, dims, pre, meta["max_length"], None]
    sd, dims, (cache, kvlen, pos, start), T, clean = _REF[("flip", q8)]
    T = steps or T
    case = dict(dims="real", steps=T)                         # synth_rows reads the widths and the V scale only
    Lc = dims["llm"]

    def roll(mode):
        orc = StepOracle(sd, dims, fault=mode)
        L = orc.num_layers
        rt = roundtrip if q8 else (lambda t: t)
        blk_k = [torch.cat([rt(cache.key_cache[i]), rt(synth_rows(case, 5, T + 2, "k")[0, :, :Lc["kv_heads"]])]) for i in range(L)]
        blk_v = [torch.cat([rt(cache.value_cache[i]), rt(synth_rows(case, 5, T + 2, "v")[0, :, :Lc["kv_heads"]])]) for i in range(L)]
        ids, tk, prev, p, n = [], int(start), 0, int(pos), int(kvlen)
        for _ in range(T):
            st_ = make_state(tk, p, [b[:n] for b in blk_k], [b[:n] for b in blk_v], [b[n:n + 2] for b in blk_k], [b[n:n + 2] for b in blk_v],
                             q8, prev_tok=prev)
            o = step(orc, st_, keep_cache=True)
            for i in range(L):                               # the block after the step: the merged rows, a late row behind them
                blk_k[i][:n + 1] = o["cache"].key_cache[i]; blk_v[i][:n + 1] = o["cache"].value_cache[i]
                if mode == "kv_row_late":
                    blk_k[i][n + 1], blk_v[i][n + 1] = orc.late[i]
            prev, tk, p, n = tk, o["tok"], p + 1, n + 1
            ids.append(o["tok"])
        return ids
    if clean is None:
        clean = _REF[("flip", q8)][4] = roll(None)
    bad = roll(fault)
    return next((i for i, (a, b) in enumerate(zip(clean, bad)) if a != b), None), T
