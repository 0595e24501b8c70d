"""Model blocks of the G2VLM hot path, expressed as sequences of libg2vlm_hip.so kernel calls.

Host side only orchestrates: which rows go to which expert, which buffers alias, which windows
the attention covers.  Every FLOP and every byte moved on the device is in csrc/*.hip.

Row layout of the MoT prefill.  The reference keeps the packed sequence in arrival order and
routes with index gathers/scatters (qwen2vl.py:584-606, 861-865, 894-907: ~10 full-tensor
passes per layer).  Here the geo (patch) rows are kept FIRST and the und (marker / text) rows
LAST for the whole 28-layer stack, so each expert sees one contiguous row range: norms take a
`split` row, GEMMs run as a 2-group launch, nothing is gathered.  Attention is order-agnostic for
the non-causal geo prefill; K/V rows are still written to the cache at their reference positions
(kv_rows), so the cache content is identical to the reference's.
"""
import math
import os

import torch

from . import hip
from .decode import Decode, KVCache, linear_names, weight_key  # noqa: F401  (KVCache: imported from here by callers)


def rope2d_tables(D, seq_len, base=100.0):
    """RoPE2D.get_cos_sin (reference pos_embed.py:120-129) under autocast: the angle is rounded to
    bf16 BEFORE cos/sin (hazard H3).  One-off host table, uploaded by the caller."""
    inv_freq = 1.0 / (base ** (torch.arange(0, D, 2).float() / D))
    t = torch.arange(seq_len, dtype=inv_freq.dtype)
    freqs = torch.einsum("i,j->ij", t, inv_freq).to(torch.bfloat16)
    freqs = torch.cat((freqs, freqs), dim=-1)
    return freqs.cos(), freqs.sin()


def attn_tile_rows(windows, Hq):
    """Query rows per attention item (128: 4-wave workgroups, 256: 8-wave) of the plan Engine.plan builds for `windows`
    (q0, q_len, k0, k_len, causal[, phase]) with Hq query heads."""
    # long KV ranges (MoT global attention, ViT): 8-wave / 256-row workgroups share each K/V tile between twice
    # the queries (0.93 vs 0.82 PF at C3); short per-view windows keep the 4-wave form
    # ... when there are enough query rows to make 256-row items worth it: a 731-row ViT prefill or a long text
    # prompt against a 15 k-row cache runs 3-6 % faster on 128-row tiles (tools/attn_small_q.py)
    long_kv = sum(w[3] for w in windows if w[0] == windows[0][0]) >= 2048 and max(w[1] for w in windows) >= 2048
    # per-view windows (DINO, the Pi3 decoders): 256-row items are 5-8 % faster there too (tools/attn_windows.py: 118 ->
    # 109 us, 150 -> 142 us at 8 x 1369) as long as the last, partly filled tile does not eat the gain and there are
    # enough items to fill the chip twice over
    tall = False
    if not long_kv:
        pad = lambda t: sum((w[1] + t - 1) // t * t for w in windows) / max(1, sum(w[1] for w in windows))  # noqa: E731
        items = sum((w[1] + 255) // 256 for w in windows) * Hq
        tall = items >= 512 and pad(256) <= 1.12 * pad(128)
    return 256 if (long_kv or tall) else 128


def pack_continuations(start_token, pos, continuations):
    """Teacher-forced rows of scoring `continuations` (lists of token ids) after a prefill whose next input is `start_token` at
    mRoPE position `pos`: continuation c = [c0 .. c_{n-1}] becomes the n rows [start, c0 .. c_{n-2}] at positions pos, pos + 1, ..
    - the tokens and positions generate_text feeds while it produces c - with targets c.  The continuations are packed one
    after the other.  Returns (input ids, positions, segment lengths, targets), plain lists of L = sum(n) (lengths: one per
    continuation)."""
    ids, poss, seg_lens, targets = [], [], [], []
    for c in continuations:
        c = [int(t) for t in c]
        if not c:
            raise ValueError("an empty continuation has nothing to score")
        ids += [int(start_token)] + c[:-1]
        poss += list(range(int(pos), int(pos) + len(c)))
        seg_lens.append(len(c))
        targets += c
    return ids, poss, seg_lens, targets


def score_windows(prefix_len, seg_lens):
    """Attention windows (q0, q_len, k0, k_len, causal) of the packed scoring pass: segment j, query rows [off_j, off_j + n_j)
    with its K/V at cache rows prefix_len + off_j .., attends to the prefix [0, prefix_len) (every key, non-causal) and
    causally to its own rows, and to no other segment.  The two windows of a segment share their query rows, so the
    attention plan merges them in its combine pass (as it merges the local and remote blocks of the view-sharded prefill)."""
    wins, off = [], 0
    for n in seg_lens:
        if prefix_len > 0:
            wins.append((off, n, 0, prefix_len, False))
        wins.append((off, n, prefix_len + off, n, True))
        off += n
    return tuple(wins)


def pack_questions(questions):
    """Rows of scoring the choices of several questions about one scene in one pass.  questions[j] = (text_ids, text_pos,
    start_token, start_pos, continuations): the ids and mRoPE positions of question j's own text rows behind the scene (what
    _chat_question prefills), the start token and position generate_text would be given behind them, and the choices as
    lists of token ids.  Rows [0, Lq): every question's text rows, one question after the other; rows [Lq, L): question by
    question, every choice as pack_continuations lays it out behind that question's start token.
    Returns (ids [L], positions [L], layout, targets [L - Lq]); layout[j] = (text rows of question j, (rows of each of its
    choices)).  Only the choice rows have targets."""
    ids, poss, layout, tail_ids, tail_pos, targets = [], [], [], [], [], []
    for text_ids, text_pos, start_token, start_pos, continuations in questions:
        text_ids, text_pos = [int(t) for t in text_ids], [int(p) for p in text_pos]
        if not text_ids or len(text_ids) != len(text_pos):
            raise ValueError("a question needs at least one text row, and one position per row")
        if len(continuations) < 1:
            raise ValueError("a question without a choice has nothing to score")
        ids += text_ids
        poss += text_pos
        c_ids, c_pos, seg_lens, c_tg = pack_continuations(start_token, start_pos, continuations)
        tail_ids += c_ids
        tail_pos += c_pos
        targets += c_tg
        layout.append((len(text_ids), tuple(seg_lens)))
    return ids + tail_ids, poss + tail_pos, tuple(layout), targets


def question_windows(prefix_len, layout):
    """Attention windows (q0, q_len, k0, k_len, causal) of pack_questions' rows over a scene of prefix_len cache rows; row r's
    K/V sit at cache row prefix_len + r.  Question j, rows [a, a + m): the scene (every key) and, causally, itself - what its
    own prefill behind the scene sees.  Choice c of question j, rows [b, b + n): the scene, question j's rows (every key) and,
    causally, itself - what score_windows gives it over a cache that ends with question j.  Nothing sees another question or
    another choice.  Windows that share their query rows are merged by the attention plan's combine pass."""
    P = int(prefix_len)
    wins, a, starts = [], 0, []
    for m, _ in layout:
        if P > 0:
            wins.append((a, m, 0, P, False))
        wins.append((a, m, P + a, m, True))
        starts.append(a)
        a += m
    b = a
    for (m, seg_lens), a_j in zip(layout, starts):
        for n in seg_lens:
            if P > 0:
                wins.append((b, n, 0, P, False))
            wins.append((b, n, P + a_j, m, False))
            wins.append((b, n, P + b, n, True))
            b += n
    return tuple(wins)


class Engine(Decode):
    SCORE_MAX_ROWS = 8192        # rows of one score_rows pass: its logits are rows x vocab bf16 (2.5 GB at the real vocabulary)
    SCORE_MAX_SEGMENTS = 64
    SCORE_PLANS_KEPT = 32        # attention plans of score_rows kept (one per (prefix_len, seg_lens)); the oldest is dropped beyond
    SCORE_MAX_QUESTIONS = 64     # questions of one score_questions pass, each with 1..SCORE_MAX_SEGMENTS choices ...
    SCORE_MAX_CHOICES = 1024     # ... and this many choices in all

    def __init__(self, weights, dims):
        self.w = weights
        self.dims = dims
        self.dev = weights.device
        self._tiles = {}
        self._rope2d = {}
        self._dino_pos = {}
        self._zeros = {}
        self.attn_events = None      # bench.py: list collecting (start, stop) HIP events around every MoT prefill attention launch
        self.gemm_events = None      # bench.py: the same around every gate/up GEMM launch of the MoT prefill (the largest Linear)
        self.patch = dims["dino"].get("patch", 14)   # geometry encoder's patch size: 14 (DINOv2) or 16 (use_dinov3, g2vlm.py:170)
        self._decode_cached = {}     # capacity bucket -> captured batch-1 decode state (decode_begin)
        self._side_streams = {}
        # parity probes (tests/test_full_depth_gpu.py): with `taps` a dict, the fp32 residual stream after the MoT layers listed
        # in `tap_layers` (1-based; split row order), the DINO tokens and the decoder outputs are cloned into it
        self.taps, self.tap_layers = None, ()
        self._decode_gen = 2         # batch-1 decode kernels: 2 = persistent grids (csrc/decode_layer.hip), 1 = csrc/decode.hip
        self._decode_weights = "bf16"   # what the decode step's Linears stream: "bf16", or "fp8" (e4m3 codes + row scales)
        self._decode_kv = "bf16"        # what the decode step keeps its KV cache as: "bf16", or "fp8" (e4m3 codes + row scales)
        self._score_plans = {}          # keys of self._tiles that score_rows made, in order of last use

    @property
    def decode_gen(self):
        return self._decode_gen

    @decode_gen.setter
    def decode_gen(self, gen):
        """A/B switch of the decode kernels.  A captured step belongs to the generation it was captured with: drop it."""
        if gen not in (1, 2):
            raise ValueError("decode_gen: 1 (csrc/decode.hip) or 2 (csrc/decode_layer.hip, default)")
        if gen != 2 and self._decode_weights == "fp8":
            raise ValueError("decode_weights == 'fp8' needs the persistent-grid kernels (decode_gen == 2)")
        if gen != 2 and self._decode_kv == "fp8":
            raise ValueError("decode_kv == 'fp8' needs the persistent-grid kernels (decode_gen == 2)")
        if gen != self._decode_gen:
            self._decode_cached.clear()
        self._decode_gen = gen

    @property
    def decode_weights(self):
        return self._decode_weights

    @decode_weights.setter
    def decode_weights(self, mode):
        """Encoding of the weights every decode step streams: "bf16" (default) or "fp8".

        "fp8": the und expert's qkv / o / gate-up / down Linears and lm_head are read as OCP e4m3 codes with one power-of-two
        scale per output row (g2vlm_amd/quant.py, csrc/decode_fp8.hip): half the weight bytes per token.  It applies to the
        batch-1 step, the batched step with B <= 8 slots, continuous batching and shared-prefix decode; prefill, recon and the
        bf16 decode keep their kernels, weights and bits.  The first switch quantises on the host (a few seconds for the real
        model) and adds `X.w8` / `X.ws` next to every such `X.w` in the weight store; the bf16 tensors stay, prefill needs them.
        Needs decode_gen == 2 (ValueError otherwise).  A batched step with MORE than 8 slots keeps its bf16 skinny-GEMM Linears,
        as it keeps them in "bf16" mode: the setting is silently without effect there.
        A captured step belongs to the encoding it was captured with: changing the mode drops the captured steps."""
        if mode not in ("bf16", "fp8"):
            raise ValueError("decode_weights: 'bf16' (default) or 'fp8'")
        if mode == "fp8":
            if self._decode_gen != 2:
                raise ValueError("decode_weights == 'fp8' needs the persistent-grid kernels (decode_gen == 2)")
            self._quantize_decode_weights()
        if mode != self._decode_weights:
            self._decode_cached.clear()
        self._decode_weights = mode

    @property
    def decode_kv(self):
        return self._decode_kv

    @decode_kv.setter
    def decode_kv(self, mode):
        """Encoding of the KV cache the decode step reads and appends to: "bf16" (default) or "fp8".

        "fp8": every cache row of a kv head is 128 OCP e4m3 codes and one fp32 power-of-two scale (g2vlm_amd/quant.py's
        encoding per row and head, K and V separately; csrc/decode_kv8.hip): 132 bytes against 256.  code * scale is exactly a
        bf16 value, so the engine is the bf16 engine whose cache rows have been replaced by dequant(quant(row)), at copy-in
        and at every append.  It applies to decode_begin (graph and eager: both decode in an engine-owned quantised block, the
        caller's rows are quantised into it and decode_end returns the appended rows dequantised), to decode_open_slots /
        decode_set_slot / decode_begin_batch and continuous batching for any slot count.  Prefill, recon and the caller's
        KVCache stay bf16.  decode_begin_shared keeps bf16 suffix blocks and reads the bf16 prefix in place: the setting is
        silently without effect there (as decode_weights is for more than 8 slots).
        Needs decode_gen == 2 (ValueError otherwise).  Changing the mode drops the captured steps."""
        if mode not in ("bf16", "fp8"):
            raise ValueError("decode_kv: 'bf16' (default) or 'fp8'")
        if mode == "fp8" and self._decode_gen != 2:
            raise ValueError("decode_kv == 'fp8' needs the persistent-grid kernels (decode_gen == 2)")
        if mode != self._decode_kv:
            self._decode_cached.clear()
        self._decode_kv = mode

    def _fp8_names(self):
        return [weight_key(n) for n in linear_names(self.dims["llm"]["layers"])]

    def _quantize_decode_weights(self):
        """X.w8 (uint8 e4m3 codes) / X.ws (fp32 row scales) for every Linear of the decode step, from the bf16 tensors the
        store holds - i.e. after the q|k|v concatenation and the gate/up interleave (a row permutation: the two commute)."""
        from .quant import quantize_rows_e4m3
        t = self.w.t
        for base in linear_names(self.dims["llm"]["layers"]):
            if base + ".w8" in t:
                continue
            q, s = quantize_rows_e4m3(t[weight_key(base)])
            t[base + ".w8"], t[base + ".ws"] = q.to(self.dev), s.to(self.dev)

    # ------------------------------------------------------------------ small caches
    def plan(self, windows, Hq):
        key = (tuple(windows), Hq)
        if key not in self._tiles:
            self._tiles[key] = hip.make_attn_plan(windows, Hq, self.dev, tile_rows=attn_tile_rows(windows, Hq))
        return self._tiles[key]

    def rope2d_tab(self, D, gh, gw):
        key = (D, gh, gw)
        if key not in self._rope2d:
            cos, sin = rope2d_tables(D // 2, max(gh, gw))
            pos = torch.cartesian_prod(torch.arange(gh), torch.arange(gw)).to(torch.int32)
            self._rope2d[key] = (cos.to(self.dev), sin.to(self.dev), pos.to(self.dev))
        return self._rope2d[key]

    def dino_pos(self, H, W):
        """interpolate_pos_encoding (modeling_dinov2_with_registers.py:93-145); host, cached per shape."""
        key = (H, W)
        if key not in self._dino_pos:
            pe = self.w.dino_pos_cpu
            n_pos = pe.shape[1] - 1
            gh, gw = H // 14, W // 14
            if not (gh * gw == n_pos and H == W):
                dim = pe.shape[-1]
                s = int(n_pos ** 0.5)
                patch = pe[:, 1:].reshape(1, s, s, dim).permute(0, 3, 1, 2)
                patch = torch.nn.functional.interpolate(patch.float(), size=(gh, gw), mode="bicubic", align_corners=False,
                                                        antialias=True)
                pe = torch.cat((pe[:, :1], patch.permute(0, 2, 3, 1).reshape(1, -1, dim)), dim=1)
            self._dino_pos[key] = pe[0].contiguous().to(self.dev)
        return self._dino_pos[key]

    # ------------------------------------------------------------------ MoT LLM
    def llm_forward(self, x, split, pos_i32, kv_rows, cache, kv_len, causal, und_rounding, num_layers=None,
                    final_norm_dtype=torch.float32, kv_total=None, kv_exchange=None, local_kv=None, windows=None):
        """Qwen2VLModel.forward_inference (reference qwen2vl.py:1267-1337) on the split row layout.

        x fp32 [L,H] (updated in place): rows [0,split) use the geo expert, rows [split,L) the und
        expert.  K/V rows are written to cache rows kv_rows; attention covers cache rows
        [0, kv_len + L).  Returns the routed final norm of x.

        View-sharded prefill (g2vlm_amd/sharded.py): x holds only this rank's rows, `kv_total` is the GLOBAL number of
        cache rows after this call, `local_kv` = (first row, rows) of this rank's own K/V block in the cache and
        `kv_exchange` the per-layer K/V exchange: .start(layer) launches the all-gather of the ranks' blocks right after the
        cache write, the attention then runs over the LOCAL block while the remote blocks travel (phase 0 of the plan),
        .wait(layer) joins, and the second launch attends to the prefix and the remote blocks and merges.

        `windows`: attention windows (q0, q_len, k0, k_len, causal) replacing the single [0, L) x [0, kv_len + L) one - several
        stages of the reference's stage-by-stage prefill run as ONE pass (G2VLM.forward_cache_update_vit_multi).
        """
        w, hp = self.w, hip
        Lc = self.dims["llm"]
        H, Hq, Hkv, eps = Lc["hidden"], Lc["heads"], Lc["kv_heads"], Lc["eps"]
        L = x.shape[0]
        tot = kv_len + L if kv_total is None else kv_total
        cache.reserve(tot)
        cos, sin = hp.mrope_table(pos_i32, w["inv_freq"])
        if kv_exchange is not None:
            assert not causal and local_kv is not None
            r0, nr = local_kv
            wins = [(0, L, r0, nr, False, 0)]
            if r0 > 0:
                wins.append((0, L, 0, r0, False, 1))
            if r0 + nr < tot:
                wins.append((0, L, r0 + nr, tot - r0 - nr, False, 1))
            plan = self.plan(tuple(wins), Hq)
        elif windows is not None:
            plan = self.plan(tuple(windows), Hq)
        else:
            plan = self.plan(((0, L, 0, tot, bool(causal)),), Hq)
        nq, nqkv = Hq * 128, (Hq + 2 * Hkv) * 128
        h = torch.empty((L, H), dtype=torch.bfloat16, device=self.dev)
        qkv = torch.empty((L, nqkv), dtype=torch.bfloat16, device=self.dev)
        qb = torch.empty((L, nq), dtype=torch.bfloat16, device=self.dev)
        ao = torch.empty((L, nq), dtype=torch.bfloat16, device=self.dev)
        act = torch.empty((L, Lc["ffn"]), dtype=torch.bfloat16, device=self.dev)
        ng, nu = split, L - split

        def groups(A, C, wname, bname=None, res=None, gamma=None, lda=None, ldc=None):
            gs = []
            for tag, r0, m, gam in (("geo", 0, ng, gamma), ("und", split, nu, None)):
                if m == 0:
                    continue
                gs.append(dict(A=A[r0:], W=w[wname.format(tag)], bias=w[bname.format(tag)] if bname else None,
                               C=C[r0:], res=res[r0:] if res is not None else None, gamma=gam, M=m))
            return gs

        for i in range(Lc["layers"] if num_layers is None else num_layers):
            p = f"L{i}."
            hp.rmsnorm(x, w[p + "geo.ln1"], w[p + "und.ln1"], split, eps, out=h)
            hp.gemm_bf16(groups(h, qkv, p + "{}.qkv.w", p + "{}.qkv.b"), nqkv, H, hp.EPI_BF16, out_ld=nqkv)
            hp.qknorm_mrope_cache(qkv, Hq, Hkv, w[p + "geo.qn"], w[p + "und.qn"], w[p + "geo.kn"], w[p + "und.kn"], split, eps,
                                  und_rounding, cos, sin, qb, cache.k[i], cache.v[i], kv_rows)
            if self.attn_events is not None:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            kk, vv_ = cache.k[i][:tot].view(tot, Hkv * 128), cache.v[i][:tot].view(tot, Hkv * 128)
            if kv_exchange is not None:
                kv_exchange.start(i)
                hp.flash_attn(qb, kk, vv_, ao, plan, Hq, Hkv, 128, phase=0)
                kv_exchange.wait(i)
                for ph in range(1, len(plan.phases)):
                    hp.flash_attn(qb, kk, vv_, ao, plan, Hq, Hkv, 128, phase=ph)
            else:
                hp.flash_attn(qb, kk, vv_, ao, plan, Hq, Hkv, 128)
            if self.attn_events is not None:
                ev[1].record()
                self.attn_events.append((ev, L, tot))
            hp.gemm_bf16(groups(ao, x, p + "{}.o.w", None, res=x, gamma=w[p + "ls1"]), H, nq, hp.EPI_RES_F32, out_ld=H, ldres=H,
                         flags=hp.GAMMA_ROUND_BF16)
            hp.rmsnorm(x, w[p + "geo.ln2"], w[p + "und.ln2"], split, eps, out=h)
            if self.gemm_events is not None:
                gev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                gev[0].record()
            hp.gemm_bf16(groups(h, act, p + "{}.gu.w"), 2 * Lc["ffn"], H, hp.EPI_SWIGLU, out_ld=Lc["ffn"])
            if self.gemm_events is not None:
                gev[1].record()
                self.gemm_events.append((gev, L))
            hp.gemm_bf16(groups(act, x, p + "{}.down.w", None, res=x, gamma=w[p + "ls2"]), H, Lc["ffn"], hp.EPI_RES_F32, out_ld=H,
                         ldres=H, lda=Lc["ffn"], flags=hp.GAMMA_ROUND_BF16)
            if self.taps is not None and split > 0 and (i + 1) in self.tap_layers:
                self.taps[f"mot{i + 1}"] = x.clone()
        cache.length = max(cache.length, tot)
        return hp.rmsnorm(x, w["norm.geo"], w["norm.und"], split, eps, out_dtype=final_norm_dtype)

    def embed(self, ids_i32, out):
        return hip.gather_rows(self.w["embed"], ids_i32, out)

    # ------------------------------------------------------------------ scoring: log-probabilities of given continuations
    def score_rows(self, cache, prefix_len, ids, pos, seg_lens, targets, top_k=0):
        """Log-probabilities of C given continuations of one prefilled scene, all in ONE teacher-forced pass.

        cache: the scene's KVCache, cache.length == prefix_len.  ids int32 [L], pos int32 [3, L], targets int32 [L] on the
        device and seg_lens (host ints, sum L) as pack_continuations lays them out.  The L rows are embedded and go through one
        llm_forward on the und expert (their K/V rows land in cache rows [prefix_len, prefix_len + L), beyond the cache's
        length) under score_windows' attention; the bf16 final norm feeds ONE lm_head GEMM over all L rows (the skinny kernel up
        to 64 rows, the tiled ones above) and ONE g2v_logprob_rows_bf16 launch.  Returns (log-probability fp32 [L], rank int32
        [L]) on the device; nothing here waits for the device once the attention plan of this (prefix_len, seg_lens) exists.
        On return cache.length is prefix_len again and rows [0, prefix_len) keep their bits (a cache too small for prefix_len
        + L rows is reallocated and copied, as by any prefill, and stays grown: at most SCORE_MAX_ROWS rows per scene cache).
        This is a prefill: it reads the bf16 weights and the bf16 cache with the prefill kernels whatever decode_weights and
        decode_kv are set to.
        top_k > 0 (at most 32): the logprob launch also writes the rows' logsumexp and ONE g2v_topk_rows_bf16 launch on the same
        logits follows; returns (log-probability, rank, logsumexp fp32 [L], top ids int32 [L, top_k], top logits fp32 [L,
        top_k]) - entry j of a row is the token whose rank is j, its log-probability is top logit - logsumexp."""
        L = int(sum(seg_lens))
        if not 1 <= len(seg_lens) <= self.SCORE_MAX_SEGMENTS or min(seg_lens) < 1:
            raise ValueError(f"score_rows: 1..{self.SCORE_MAX_SEGMENTS} continuations of at least one token each")
        if L > self.SCORE_MAX_ROWS:
            raise ValueError(f"score_rows: {L} rows in one pass, at most {self.SCORE_MAX_ROWS}")
        self._check_top_k(top_k, "score_rows")
        assert cache.length == prefix_len and ids.numel() == L and targets.numel() == L and tuple(pos.shape) == (3, L)
        wins = score_windows(prefix_len, seg_lens)
        self._score_plan(wins)
        return self._score_pass(cache, prefix_len, ids, pos, wins, 0, targets, top_k)

    def _score_plan(self, wins):
        """The attention plan of a scoring pass, built (and uploaded) before the first launch.  An evaluation sweep brings a new
        shape with nearly every item, so only the SCORE_PLANS_KEPT most recently used ones stay (their device tables are freed
        in stream order, behind the launches that read them).  The plan cache is keyed by (windows, heads) alone, so evicting
        also drops the plan of another caller that happens to use the identical windows; that caller rebuilds it on its next
        call - a little host work, never a wrong result."""
        key = (wins, self.dims["llm"]["heads"])
        self._score_plans.pop(key, None)
        self._score_plans[key] = True
        self.plan(wins, key[1])
        while len(self._score_plans) > self.SCORE_PLANS_KEPT:
            self._tiles.pop(next(iter(self._score_plans)), None)
            del self._score_plans[next(iter(self._score_plans))]

    def _score_pass(self, cache, prefix_len, ids, pos, wins, first, targets, top_k):
        """One teacher-forced pass of L rows behind the scene under `wins`; logits, log-probabilities, ranks and (top_k > 0)
        the top-k entries of the rows [first, L) only."""
        Lc = self.dims["llm"]
        L = ids.numel()
        x = torch.empty((L, Lc["hidden"]), dtype=torch.float32, device=self.dev)
        self.embed(ids, x)
        kv_rows = torch.arange(prefix_len, prefix_len + L, dtype=torch.int32, device=self.dev)
        h = self.llm_forward(x, 0, pos, kv_rows, cache, prefix_len, causal=False, und_rounding=1, final_norm_dtype=torch.bfloat16,
                             windows=wins)
        cache.length = prefix_len                            # the scored rows were never part of the scene
        n = L - first
        logits = torch.empty((n, Lc["vocab"]), dtype=torch.bfloat16, device=self.dev)
        hip.linear(h[first:] if first else h, self.w["lm_head"], out=logits)
        lp = torch.empty(n, dtype=torch.float32, device=self.dev)
        rank = torch.empty(n, dtype=torch.int32, device=self.dev)
        if not top_k:
            hip.logprob_rows_bf16(logits, targets, rank=rank, out=lp)
            return lp, rank
        lse = torch.empty(n, dtype=torch.float32, device=self.dev)
        hip.logprob_rows_bf16(logits, targets, lse=lse, rank=rank, out=lp)
        top_ids = torch.empty((n, int(top_k)), dtype=torch.int32, device=self.dev)
        top_vals = torch.empty((n, int(top_k)), dtype=torch.float32, device=self.dev)
        hip.topk_rows_bf16(logits, int(top_k), out_idx=top_ids, out_val=top_vals)
        return lp, rank, lse, top_ids, top_vals

    def score_questions(self, cache, prefix_len, ids, pos, layout, targets, top_k=0):
        """score_rows for the choices of Q questions about one prefilled scene, questions included, in ONE teacher-forced pass.

        cache: the scene's KVCache (system prompt, views, images - no question), cache.length == prefix_len.  ids int32 [L],
        pos int32 [3, L], layout and targets int32 [L - Lq] as pack_questions lays them out: the Lq text rows of all questions
        first, then every choice's rows.  All L rows go through one llm_forward on the und expert under question_windows'
        attention (a question sees the scene and itself, a choice the scene, its question and itself), their K/V in cache rows
        [prefix_len, prefix_len + L) beyond the cache's length; the bf16 final norm of the choice rows alone - the contiguous
        tail - feeds ONE lm_head GEMM, ONE g2v_logprob_rows_bf16 launch and, with top_k > 0, ONE g2v_topk_rows_bf16 launch.
        Returns what score_rows returns, for the L - Lq choice rows.  Nothing waits for the device; on return cache.length is
        prefix_len and the scene's rows keep their bits.  1..SCORE_MAX_QUESTIONS questions of 1..SCORE_MAX_SEGMENTS choices,
        SCORE_MAX_CHOICES choices and SCORE_MAX_ROWS rows in all (ValueError before any launch)."""
        layout = tuple((int(m), tuple(int(n) for n in segs)) for m, segs in layout)
        if not 1 <= len(layout) <= self.SCORE_MAX_QUESTIONS:
            raise ValueError(f"score_questions: 1..{self.SCORE_MAX_QUESTIONS} questions, got {len(layout)}")
        for m, segs in layout:
            if m < 1 or not 1 <= len(segs) <= self.SCORE_MAX_SEGMENTS or min(segs) < 1:
                raise ValueError(f"score_questions: a question of at least one row with 1..{self.SCORE_MAX_SEGMENTS} choices of at "
                                 "least one token each")
        n_choices = sum(len(segs) for _, segs in layout)
        if n_choices > self.SCORE_MAX_CHOICES:
            raise ValueError(f"score_questions: {n_choices} choices in one pass, at most {self.SCORE_MAX_CHOICES}")
        Lq = sum(m for m, _ in layout)
        L = Lq + sum(sum(segs) for _, segs in layout)
        if L > self.SCORE_MAX_ROWS:
            raise ValueError(f"score_questions: {L} rows in one pass, at most {self.SCORE_MAX_ROWS}")
        self._check_top_k(top_k, "score_questions")
        assert cache.length == prefix_len and ids.numel() == L and targets.numel() == L - Lq and tuple(pos.shape) == (3, L)
        wins = question_windows(prefix_len, layout)
        self._score_plan(wins)
        return self._score_pass(cache, prefix_len, ids, pos, wins, Lq, targets, top_k)

    @staticmethod
    def _check_top_k(top_k, what):
        if not 0 <= int(top_k) <= hip.TOPK_MAX:
            raise ValueError(f"{what}: top_k = {top_k}, 0 (none) .. {hip.TOPK_MAX}")

    # ------------------------------------------------------------------ DINOv2 encoder
    def dino_embed(self, images_norm):
        """Dinov2WithRegistersEmbeddings.forward (reference modeling_dinov2_with_registers.py:147-171): im2col GEMM,
        CLS, position table, 4 registers.  fp32 [N*(P+5), C]."""
        w, hp = self.w, hip
        N, _, H, W = images_norm.shape
        P = (H // 14) * (W // 14)
        cols = hp.im2col14(images_norm, w["dino.patch.w"].shape[1])
        emb = hp.linear(cols, w["dino.patch.w"], w["dino.patch.b"])
        return hp.dino_assemble(emb, w["dino.cls"], w["dino.regs"], self.dino_pos(H, W), N, P)

    def dino_layers(self, x, n_windows, window_len, num_layers=None):
        """Dinov2WithRegistersEncoder + final LayerNorm (reference dinov2_model.py:251-275, 351) on fp32 token rows x
        (updated in place).  Attention windows are [i*window_len, (i+1)*window_len) for i < n_windows; rows outside every
        window get a zero attention output (hazard H1).  Returns final-LN tokens bf16 [rows, C]."""
        w, hp = self.w, hip
        Dn = self.dims["dino"]
        C, nh = Dn["hidden"], Dn["heads"]
        T = x.shape[0]
        plan = self.plan(tuple((i * window_len, window_len, i * window_len, window_len, False) for i in range(n_windows)), nh)
        h = torch.empty((T, C), dtype=torch.bfloat16, device=self.dev)
        qkv = torch.empty((T, 3 * C), dtype=torch.bfloat16, device=self.dev)
        ao = torch.zeros((T, C), dtype=torch.bfloat16, device=self.dev)        # rows outside every window stay 0
        mid = torch.empty((T, 4 * C), dtype=torch.bfloat16, device=self.dev)
        for i in range(Dn["layers"] if num_layers is None else num_layers):
            p = f"D{i}."
            hp.layernorm(x, w[p + "norm1.w"], w[p + "norm1.b"], 1e-6, out=h)
            hp.linear(h, w[p + "qkv.w"], w[p + "qkv.b"], out=qkv)
            if n_windows > 0:
                hp.flash_attn(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], ao, plan, nh, nh, C // nh)
            hp.linear(ao, w[p + "dense.w"], w[p + "dense.b"], hp.EPI_RES_F32, out=x, res=x, gamma=w[p + "ls1"])
            hp.layernorm(x, w[p + "norm2.w"], w[p + "norm2.b"], 1e-6, out=h)
            hp.linear(h, w[p + "fc1.w"], w[p + "fc1.b"], hp.EPI_GELU, out=mid)
            hp.linear(mid, w[p + "fc2.w"], w[p + "fc2.b"], hp.EPI_RES_F32, out=x, res=x, gamma=w[p + "ls2"])
        return hp.layernorm(x, w["dino.ln.w"], w["dino.ln.b"], 1e-6, out=h)

    def dino_forward(self, images_norm, window_len, num_layers=None):
        """Dinov2WithRegistersModel.forward (reference dinov2_model.py:301-356).  images_norm fp32 [N,3,H,W] on device.
        Windows are [i*window_len, (i+1)*window_len) of the flat [N*(P+5)] token axis exactly as the reference builds
        them (hazard H1: window_len = P, so the last 5N rows get a zero attention output)."""
        return self.dino_layers(self.dino_embed(images_norm), images_norm.shape[0], window_len, num_layers)

    # ------------------------------------------------------------------ Pi3 decoders
    def decoder(self, name, hidden, N, gh, gw, context=None, depth=None):
        """Pi3TransformerDecoder / Pi3ContextTransformerDecoder (reference transformer_head.py:9-56,
        84-130; blocks block.py:259-405).  hidden fp32 [N*P, C]; context fp32 [P, C] = view 0
        (identical for every view, g2vlm.py:1196, so its K/V are computed once).  Returns bf16."""
        w, hp = self.w, hip
        C = self.dims["llm"]["hidden"]
        nh = self.dims["dec"]["heads"]
        D = C // nh
        P = gh * gw
        M = N * P
        cos, sin, pos = self.rope2d_tab(D, gh, gw)
        x = hidden.clone()
        h = torch.empty((M, C), dtype=torch.bfloat16, device=self.dev)
        qkv = torch.empty((M, 3 * C), dtype=torch.bfloat16, device=self.dev)
        ao = torch.empty((M, C), dtype=torch.bfloat16, device=self.dev)
        mid = torch.empty((M, 4 * C), dtype=torch.bfloat16, device=self.dev)
        self_plan = self.plan(tuple((v * P, P, v * P, P, False) for v in range(N)), nh)
        if context is not None:
            cross_plan = self.plan(tuple((v * P, P, 0, P, False) for v in range(N)), nh)
            yn = torch.empty((P, C), dtype=torch.bfloat16, device=self.dev)
            ckv = torch.empty((P, 2 * C), dtype=torch.bfloat16, device=self.dev)
            cq = torch.empty((M, C), dtype=torch.bfloat16, device=self.dev)
        for i in range(self.dims["dec"]["depth"] if depth is None else depth):
            p = f"{name}.{i}."
            hp.layernorm(x, w[p + "norm1.w"], w[p + "norm1.b"], 1e-6, out=h)
            hp.linear(h, w[p + "attn.qkv.w"], w[p + "attn.qkv.b"], out=qkv)
            hp.rope2d(qkv, 0, 2 * nh, D, cos, sin, pos, P)
            hp.flash_attn(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], ao, self_plan, nh, nh, D)
            hp.linear(ao, w[p + "attn.proj.w"], w[p + "attn.proj.b"], hp.EPI_RES_F32, out=x, res=x)
            if context is not None:
                hp.layernorm(context, w[p + "norm_y.w"], w[p + "norm_y.b"], 1e-6, out=yn)
                hp.linear(yn, w[p + "ckv.w"], w[p + "ckv.b"], out=ckv)
                hp.rope2d(ckv, 0, nh, D, cos, sin, pos, P)
                hp.layernorm(x, w[p + "norm2.w"], w[p + "norm2.b"], 1e-6, out=h)
                hp.linear(h, w[p + "cq.w"], w[p + "cq.b"], out=cq)
                hp.rope2d(cq, 0, nh, D, cos, sin, pos, P)
                hp.flash_attn(cq, ckv[:, :C], ckv[:, C:], ao, cross_plan, nh, nh, D)
                hp.linear(ao, w[p + "cproj.w"], w[p + "cproj.b"], hp.EPI_RES_F32, out=x, res=x)
                n_mlp = "norm3"
            else:
                n_mlp = "norm2"
            hp.layernorm(x, w[p + n_mlp + ".w"], w[p + n_mlp + ".b"], 1e-6, out=h)
            hp.linear(h, w[p + "mlp.fc1.w"], w[p + "mlp.fc1.b"], hp.EPI_GELU, out=mid)
            hp.linear(mid, w[p + "mlp.fc2.w"], w[p + "mlp.fc2.b"], hp.EPI_RES_F32, out=x, res=x)
        return hp.linear(hp.cast_bf16(x), w[name + ".out.w"], w[name + ".out.b"])

    def decoders_and_heads(self, hidden, context, N, gh, gw, H, W):
        """The three Pi3 decoders and the fp32 heads of G2VLM.reconstruct (reference g2vlm.py:1186-1226: point, camera, global
        decoder, then the heads).  Returns (point_hidden, camera_hidden, global_hidden, points, local_points, poses,
        global_points).  The global decoder and its head share nothing with the other two until the results are returned, so
        they run on a side stream; the caller's stream runs camera decoder -> camera head -> point decoder -> point head (the
        point head needs the poses).  Two sequences side by side fill each other's low-power stretches (layer norms, RoPE, the
        fp32 heads, single-round Linears' epilogues); the order of independent kernels changes nothing in their results.
        G2V_HEADS_OVERLAP: 0 = everything in sequence, 1 = only the camera / point heads on the side stream (A/B).
        Buffers cross the two streams without record_stream: every use of the side stream starts with side.wait_stream(caller's)
        and ends with the caller's stream waiting for it, so a block freed after the join is only ever reused behind that join
        in either stream's order - and a deferred free would make the caching allocator hipMalloc in steady state
        (tools/step_outliers.py: 13 device mallocs in 40 steps with record_stream, a device-wide stall each)."""
        P = gh * gw
        mode = "0" if torch.cuda.is_current_stream_capturing() else os.environ.get("G2V_HEADS_OVERLAP", "2")
        if mode == "0":
            point_hidden = self.decoder("point_decoder", hidden, N, gh, gw)
            camera_hidden = self.decoder("camera_decoder", hidden, N, gh, gw)
            global_hidden = self.decoder("global_points_decoder", hidden, N, gh, gw, context=context)
            points, local, poses, glob = self.heads(point_hidden, camera_hidden, global_hidden, N, H, W)
            return point_hidden, camera_hidden, global_hidden, points, local, poses, glob
        cur = torch.cuda.current_stream()
        side = self.side_stream(cur)
        if mode == "1":
            camera_hidden = self.decoder("camera_decoder", hidden, N, gh, gw)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                poses = self.camera_poses(camera_hidden, N, P)
            point_hidden = self.decoder("point_decoder", hidden, N, gh, gw)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                points, local = self.point_maps_local(point_hidden, poses, N, H, W)
            global_hidden = self.decoder("global_points_decoder", hidden, N, gh, gw, context=context)
            cur.wait_stream(side)
            glob = self.point_maps_global(global_hidden, N, H, W)
            return point_hidden, camera_hidden, global_hidden, points, local, poses, glob
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            global_hidden = self.decoder("global_points_decoder", hidden, N, gh, gw, context=context)
            glob = self.point_maps_global(global_hidden, N, H, W)
        camera_hidden = self.decoder("camera_decoder", hidden, N, gh, gw)
        poses = self.camera_poses(camera_hidden, N, P)
        point_hidden = self.decoder("point_decoder", hidden, N, gh, gw)
        points, local = self.point_maps_local(point_hidden, poses, N, H, W)
        cur.wait_stream(side)
        return point_hidden, camera_hidden, global_hidden, points, local, poses, glob

    def side_stream(self, cur):
        """One side stream per caller's stream (kept: stream creation is not free), for work that is independent of what
        the caller's stream is doing (G2VLM.prefill_text_and_dino)."""
        key = cur.cuda_stream
        if key not in self._side_streams:
            self._side_streams[key] = torch.cuda.Stream(device=self.dev)
        return self._side_streams[key]

    def conf_head(self, conf_hidden, N, H, W):
        """Confidence map of a train_conf_pi3 checkpoint (reference g2vlm.py:1208-1210): fp32 Linear 1024 -> patch^2 +
        pixel_shuffle(patch) -> [N, H, W, 1]."""
        cf = hip.gemm_f32(hip.cast_f32(conf_hidden), self.w["conf_head.w"], self.w["conf_head.b"])
        return hip.pixel_shuffle(cf, N, H, W, 1, self.patch)

    def camera_poses(self, camera_hidden, N, P):
        """Pi3CameraHead (reference camera_head.py:32-93; fp32, autocast off, g2vlm.py:1213-1215): 2 x [3 Linear + ReLU + skip]
        on the view's P tokens, mean over P, 2 x (Linear + ReLU), fc_t / fc_rot, row-normalise, SVD, det fix.
        camera_hidden bf16 [N*P, 512] -> fp32 [N, 4, 4]."""
        w, hp = self.w, hip
        feat = hp.cast_f32(camera_hidden)
        for i in range(2):
            t = hp.gemm_f32(feat, w[f"cam.res{i}.1.w"], w[f"cam.res{i}.1.b"], relu=True)
            t = hp.gemm_f32(t, w[f"cam.res{i}.2.w"], w[f"cam.res{i}.2.b"], relu=True)
            feat = hp.gemm_f32(t, w[f"cam.res{i}.3.w"], w[f"cam.res{i}.3.b"], relu=True, res=feat)
        return hp.camera_tail(feat, N, P, w["cam.mlp0.w"], w["cam.mlp0.b"], w["cam.mlp1.w"], w["cam.mlp1.b"],
                              w["cam.fc_t.w"], w["cam.fc_t.b"], w["cam.fc_rot.w"], w["cam.fc_rot.b"])

    def point_maps(self, point_hidden, global_hidden, poses, N, H, W):
        """Pi3LinearPts3d x 2 + the post-math (reference transformer_head.py:58-81, g2vlm.py:1200-1205, 1219-1226): fp32 Linear
        1024 -> 3 patch^2, pixel_shuffle, z = exp(z), (x z, y z, z), world points = pose . [local, 1].  Per patch: the hidden
        rows may be any (H / patch) x (W / patch) grid of patches per view.  Returns (points, local_points, global_points)."""
        points, local = self.point_maps_local(point_hidden, poses, N, H, W)
        return points, local, self.point_maps_global(global_hidden, N, H, W)

    def point_maps_local(self, point_hidden, poses, N, H, W):
        """The point head's half of point_maps: (world points, local points)."""
        w, hp = self.w, hip
        pf = hp.gemm_f32(hp.cast_f32(point_hidden), w["point_head.w"], w["point_head.b"])
        local, points = hp.pts_epilogue(pf, N, H, W, 1, poses, patch=self.patch)
        return points, local

    def point_maps_global(self, global_hidden, N, H, W):
        """The global point head's half of point_maps."""
        w, hp = self.w, hip
        gf = hp.gemm_f32(hp.cast_f32(global_hidden), w["global_point_head.w"], w["global_point_head.b"])
        glob, _ = hp.pts_epilogue(gf, N, H, W, 0, patch=self.patch)
        return glob

    def heads(self, point_hidden, camera_hidden, global_hidden, N, H, W):
        """fp32 islands of G2VLM.reconstruct (reference g2vlm.py:1200-1226)."""
        poses = self.camera_poses(camera_hidden, N, (H // self.patch) * (W // self.patch))
        points, local, glob = self.point_maps(point_hidden, global_hidden, poses, N, H, W)
        return points, local, poses, glob

    # ------------------------------------------------------------------ Qwen2-VL ViT
    def vit_forward(self, pixel_values, grid_thw, cos, sin, num_layers=None, n_images=1):
        """Qwen2VisionTransformerPretrainedModel.forward (reference modeling_qwen2_vl.py:1048-1072).
        pixel_values fp32 [T, Kpad] on device (K = 1176 zero-padded on the host to the patch GEMM's
        K); cos/sin fp32 [T, head_dim] on device.  Returns bf16 [T/4, out].
        n_images > 1: that many images of the same grid stacked along T (cos / sin tiled by the caller) - the reference
        runs them one call each (g2vlm.py:1362-1370); the tokens do not interact (one attention window per frame), so one
        pass over the stack gives each image its own result."""
        w, hp = self.w, hip
        V = self.dims["vit"]
        C, nh = V["embed"], V["heads"]
        D = C // nh
        T = pixel_values.shape[0]
        t, gh, gw = grid_thw
        t = t * n_images
        assert pixel_values.shape[1] == w["vit.patch.w"].shape[1] and T == t * gh * gw
        x = hp.linear(pixel_values if pixel_values.dtype == torch.bfloat16 else hp.cast_bf16(pixel_values), w["vit.patch.w"], None)
        plan = self.plan(tuple((i * gh * gw, gh * gw, i * gh * gw, gh * gw, False) for i in range(t)), nh)
        h = torch.empty((T, C), dtype=torch.bfloat16, device=self.dev)
        qkv = torch.empty((T, 3 * C), dtype=torch.bfloat16, device=self.dev)
        ao = torch.empty((T, C), dtype=torch.bfloat16, device=self.dev)
        mid = torch.empty((T, int(C * V["mlp_ratio"])), dtype=torch.bfloat16, device=self.dev)
        for i in range(V["depth"] if num_layers is None else num_layers):
            p = f"V{i}."
            hp.layernorm(x, w[p + "norm1.w"], w[p + "norm1.b"], 1e-6, out=h)
            hp.linear(h, w[p + "attn.qkv.w"], w[p + "attn.qkv.b"], out=qkv)
            hp.rope_vision(qkv, 2 * nh, D, cos, sin)
            hp.flash_attn(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], ao, plan, nh, nh, D)
            hp.linear(ao, w[p + "attn.proj.w"], w[p + "attn.proj.b"], hp.EPI_RES_BF16, out=x, res=x)
            hp.layernorm(x, w[p + "norm2.w"], w[p + "norm2.b"], 1e-6, out=h)
            hp.linear(h, w[p + "mlp.fc1.w"], w[p + "mlp.fc1.b"], hp.EPI_QUICKGELU, out=mid)
            hp.linear(mid, w[p + "mlp.fc2.w"], w[p + "mlp.fc2.b"], hp.EPI_RES_BF16, out=x, res=x)
        hp.layernorm(x, w["vit.ln_q.w"], w["vit.ln_q.b"], 1e-6, out=h)
        m = hp.linear(h.view(T // 4, 4 * C), w["vit.m0.w"], w["vit.m0.b"], hp.EPI_GELU)
        return hp.linear(m, w["vit.m2.w"], w["vit.m2.b"])
