"""The decode step (reference generate_text loop body, g2vlm.py:1088-1125): one token through the und-expert layers, the
final norm, lm_head and the sampler, for one scene or for B scene slots.

The step program is written once (`Decode._step`): embed, mRoPE table, per layer qkv -> attention -> o -> gate/up -> down,
lm_head, argmax or sample, advance.  What differs between the modes is chosen when the state is built and kept in it:

  st["lin"]   one Linear FAMILY, lin(x, name, norm=None, bias=None, out=None, res=None, act=False):
                gen-1 batch 1 (csrc/decode.hip), gemv_pg (csrc/decode_layer.hip), gemv_pg_batch (csrc/decode_batch.hip), the
                last two on e4m3 weights (csrc/decode_fp8.hip), or separate RMSNorm + skinny GEMM for more than 8 slots
  st["attn"]  one attention FORM, attn(layer): decode_attn_pg, decode_attn_pg_kv8 (csrc/decode_kv8.hip: the same over an e4m3
                cache), decode_attn_fused, qknorm_mrope_cache + decode_attn_batch, or decode_attn_shared (shared-prefix decode)

Selection.  Persistent-grid GEMVs iff decode_gen == 2 and B <= 8, on e4m3 weights iff decode_weights == "fp8" as well.
Attention: shared if a prefix is set, else the persistent-grid form if decode_gen == 2, else the fused form at batch 1 or
while its grid fits the chip, else the split form.  The cache of a state without a prefix is e4m3 iff decode_kv == "fp8"
(which needs decode_gen == 2): st["k"] / st["v"] are then code tensors, st["ks"] / st["vs"] their scales, and the attention is
decode_attn_pg_kv8 for any slot count.  A state (and its captured step) keeps what it was built with.
The step is allocation-free and host-state-free: position, cache row and KV length live in the state on the device and are
advanced by the last kernel, so the whole step can be captured in a hipGraph (`Decode._capture`).
"""
import torch

from . import hip


class KVCache:
    """Pre-allocated contiguous replacement of NaiveCache (qwen2vl.py:237-251): same logical content
    (K post-RoPE, bf16, [len, Hkv, 128] per layer) without the per-call realloc + 4 scatters."""

    def __init__(self, num_layers, n_kv_heads=2, device="cuda", capacity=0):
        self.num_layers_, self.hkv, self.device = num_layers, n_kv_heads, device
        self.k = [None] * num_layers
        self.v = [None] * num_layers
        self.capacity = 0
        self.length = 0
        if capacity:
            self.reserve(capacity)

    def reserve(self, n):
        if n <= self.capacity:
            return
        cap = max(n, int(self.capacity * 1.5))
        for i in range(self.num_layers_):
            nk = torch.empty((cap, self.hkv, 128), dtype=torch.bfloat16, device=self.device)
            nv = torch.empty_like(nk)
            if self.k[i] is not None and self.length:
                nk[:self.length].copy_(self.k[i][:self.length]); nv[:self.length].copy_(self.v[i][:self.length])
            self.k[i], self.v[i] = nk, nv
        self.capacity = cap

    # NaiveCache-compatible views
    @property
    def num_layers(self):
        return self.num_layers_

    @property
    def seq_lens(self):
        return self.length

    @property
    def key_cache(self):
        return {i: (self.k[i][:self.length] if self.length else None) for i in range(self.num_layers_)}

    @property
    def value_cache(self):
        return {i: (self.v[i][:self.length] if self.length else None) for i in range(self.num_layers_)}


class KV8Cache:
    """Engine-owned e4m3 KV blocks of a decode state (Engine.decode_kv == "fp8"): per layer, codes k[i] / v[i] uint8
    [B, cap, Hkv, 128] and power-of-two scales ks[i] / vs[i] fp32 [B, cap, Hkv] (g2vlm_amd/quant.py's encoding per row and kv
    head).  The layers are views of one allocation each, so a row of every layer is reached in one indexing operation.
    Every row starts as zero codes with scale 1."""

    def __init__(self, num_layers, n_slots, capacity, n_kv_heads, device):
        shape = (num_layers, n_slots, capacity, n_kv_heads)
        self.kc, self.vc = (torch.zeros(shape + (128,), dtype=torch.uint8, device=device) for _ in range(2))
        self.ksc, self.vsc = (torch.ones(shape, dtype=torch.float32, device=device) for _ in range(2))
        self.k, self.v, self.ks, self.vs = (list(t.unbind(0)) for t in (self.kc, self.vc, self.ksc, self.vsc))
        self.capacity, self.length = capacity, 0

    def put(self, j, cache, n):
        """Rows [0, n) of the bf16 KVCache `cache`, quantised, into slot j."""
        for i in range(len(self.k)):
            hip.kv_quant_e4m3(cache.k[i][:n], self.k[i][j, :n], self.ks[i][j, :n])
            hip.kv_quant_e4m3(cache.v[i][:n], self.v[i][j, :n], self.vs[i][j, :n])

    def get(self, j, lo, hi, cache):
        """Rows [lo, hi) of slot j, dequantised (exact), into the same rows of the bf16 KVCache `cache`."""
        for i in range(len(self.k)):
            hip.kv_dequant_e4m3(self.k[i][j, lo:hi], self.ks[i][j, lo:hi], out=cache.k[i][lo:hi])
            hip.kv_dequant_e4m3(self.v[i][j, lo:hi], self.vs[i][j, lo:hi], out=cache.v[i][lo:hi])

    def clear_row0(self, j):
        self.kc[:, j, 0] = 0; self.vc[:, j, 0] = 0
        self.ksc[:, j, 0] = 1; self.vsc[:, j, 0] = 1


def linear_names(layers):
    """The Linears the decode step streams, as the step names them."""
    return [f"L{i}.und.{n}" for i in range(layers) for n in ("qkv", "o", "gu", "down")] + ["lm_head"]


def weight_key(name):
    """Store key of Linear `name`'s bf16 matrix; its e4m3 codes / row scales are name + ".w8" / ".ws" (lm_head has no ".w")."""
    return name if name == "lm_head" else name + ".w"


# ---- Linear families.  The closures hold tensors, never the state: a dropped state frees its KV blocks at once.
def _lin_gemv1(w, eps):
    def lin(x, name, norm=None, bias=None, out=None, res=None, act=False):
        if act:
            hip.gemv_rmsnorm_swiglu_bf16(x, norm, eps, w[weight_key(name)], out)
        elif norm is not None:
            hip.gemv_rmsnorm_bf16(x, norm, eps, w[weight_key(name)], bias, out)
        else:
            hip.gemv_bf16(x, w[weight_key(name)], bias, out, res=res)
    return lin


def _lin_pg(w, eps, batched, fp8):
    fn = getattr(hip, "gemv_pg" + ("_batch" if batched else "") + ("_fp8" if fp8 else ""))

    def lin(x, name, norm=None, bias=None, out=None, res=None, act=False):
        mats = (w[name + ".w8"], w[name + ".ws"]) if fp8 else (w[weight_key(name)],)
        if norm is not None:
            fn(x, *mats, norm_w=norm, eps=eps, bias=bias, out=out, res=res, act=act)
        else:
            fn(x, *mats, bias=bias, out=out, res=res, act=act)
    return lin


def _lin_skinny(w, eps, h, gws):
    def lin(x, name, norm=None, bias=None, out=None, res=None, act=False):
        if norm is not None:
            hip.rmsnorm(x, norm, norm, 0, eps, out=h)
            x = h
        epi = hip.EPI_SWIGLU if act else (hip.EPI_BF16 if res is None else hip.EPI_RES_F32)
        hip.linear(x, w[weight_key(name)], bias, epi, out=out if res is None else res, res=res, ws=gws)
    return lin


class Decode:
    """The decode half of Engine (engine.py): needs self.w, self.dims, self.dev, self.decode_gen, self._decode_weights,
    self._decode_kv and self._decode_cached."""

    # ------------------------------------------------------------------ the step
    def _step(self, st):
        w, Lc = self.w, self.dims["llm"]
        lin, attn = st["lin"], st["attn"]
        x, qkv, ao = st["lin_io"]                          # what the Linears read and write: flat at batch 1, [B, .] for slots
        hip.gather_rows(w["embed"], st["tok"], st["x"])
        hip.mrope_table_into(st["pos"], w["inv_freq"], st["cos"], st["sin"])
        for i in range(Lc["layers"]):
            p = f"L{i}.und."
            lin(x, p + "qkv", norm=w[p + "ln1"], bias=w[p + "qkv.b"], out=qkv)
            attn(i)
            lin(ao, p + "o", res=x)
            lin(x, p + "gu", norm=w[p + "ln2"], out=st["act"], act=True)
            lin(st["act"], p + "down", res=x)
        lin(x, "lm_head", norm=w["norm.und"], out=st["logits"])
        if st.get("rng") is not None:                      # do_sample (reference g2vlm.py:1119-1122)
            hip.sample_rows_bf16(st["logits"], st["tok"], st["amax"], st["rng"])
        elif st["flat"]:
            hip.argmax_bf16(st["logits"], st["tok"], st["amax"])
        else:
            hip.argmax_rows_bf16(st["logits"], st["tok"], st["amax"])
        (hip.decode_advance if st["flat"] else hip.decode_advance_batch)(st["pos"], st["row"], st["len"])

    def _attention(self, st, prefix):
        """The attention form of `st`: attn(layer) over st["k"] / st["v"] (blocks of scene_rows rows, split by attn_cap; with
        st["ks"] / st["vs"] when the state's cache is e4m3)."""
        w, Lc = self.w, self.dims["llm"]
        Hq, Hkv, eps, scale = Lc["heads"], Lc["kv_heads"], Lc["eps"], 128 ** -0.5
        d, B, rows, cap = self.dev, st["B"], st["scene_rows"], st["attn_cap"]
        k, v, qkv, ao, cos, sin, ln = st["k"], st["v"], st["qkv"], st["ao"], st["cos"], st["sin"], st["len"]
        f32 = lambda nbytes: torch.empty(nbytes // 4, dtype=torch.float32, device=d)  # noqa: E731
        norms = lambda i: (w[f"L{i}.und.qn"], w[f"L{i}.und.kn"])  # noqa: E731
        if prefix is not None:                               # every slot's cache is this prefix + its own suffix block
            plen = prefix.length
            ws = f32(hip.decode_attn_shared_workspace(Hq, Hkv, B, plen, rows))
            return lambda i: hip.decode_attn_shared(qkv, *norms(i), eps, 1, cos, sin, prefix.k[i], prefix.v[i], plen, k[i], v[i], ln,
                                                    rows, rows, Hq, Hkv, scale, ao, ws)
        if st["kv"] == "fp8":
            ks, vs = st["ks"], st["vs"]
            ws = f32(hip.decode_attn_pg_workspace(Hq, Hkv, B))
            return lambda i: hip.decode_attn_pg_kv8(qkv, *norms(i), eps, 1, cos, sin, k[i], v[i], ks[i], vs[i], ao, ln, rows, cap, Hq, Hkv,
                                                    scale, ws)
        if st["gen"] == 2:
            ws = f32(hip.decode_attn_pg_workspace(Hq, Hkv, B))
            return lambda i: hip.decode_attn_pg(qkv, *norms(i), eps, 1, cos, sin, k[i], v[i], ao, ln, rows, cap, Hq, Hkv, scale, ws)
        ws = f32(B * hip.decode_attn_workspace(rows, Hq))
        # the fused norm + RoPE + append form of the attention kernel holds 206 VGPRs (2 workgroups per CU): one launch less per
        # layer while the grid fits the chip at once (15.0 vs 12.9 + 4.6 us at B = 1), slower once it does not (34.6 vs 26.9 +
        # 4.7 us at B = 8, 688 workgroups)
        if st["flat"] or B * ((rows // 64 + 3) // 4) * Hkv <= 512:
            return lambda i: hip.decode_attn_fused(qkv, *norms(i), eps, 1, cos, sin, k[i], v[i], ao, ln, rows, rows, Hq, Hkv, scale, ws)
        q, row = torch.empty((B, Hq * 128), dtype=torch.bfloat16, device=d), st["row"]

        def split(i):
            qn, kn = norms(i)
            hip.qknorm_mrope_cache(qkv, Hq, Hkv, qn, qn, kn, kn, 0, eps, 1, cos, sin, q, k[i], v[i], row)
            hip.decode_attn_batch(q, k[i], v[i], ao, ln, rows, rows, Hq, Hkv, scale, ws)
        return split

    def _decode_state(self, B, k, v, scene_rows, attn_cap, sample=None, flat=False, prefix=None, scales=None):
        """Device-side state of a decode over the KV blocks k / v (one tensor per layer, scene_rows rows per scene, which must
        not move any more).  flat: the batch-1 step (1-D activations and logits, batch-1 kernels); else B slots.
        scales = (ks, vs): k / v hold e4m3 codes and these are their scales (KV8Cache)."""
        Lc = self.dims["llm"]
        H, Hq, Hkv, Fd, eps = Lc["hidden"], Lc["heads"], Lc["kv_heads"], Lc["ffn"], Lc["eps"]
        d, bf = self.dev, torch.bfloat16
        i32 = lambda vals: torch.tensor(vals, dtype=torch.int32, device=d)  # noqa: E731
        buf = lambda n, dt=bf: torch.empty((B, n), dtype=dt, device=d)  # noqa: E731
        vec = (lambda t: t.view(-1)) if flat else (lambda t: t)
        x, qkv, ao = buf(H, torch.float32), buf((Hq + 2 * Hkv) * 128), buf(Hq * 128)
        st = dict(B=B, cap=scene_rows, scene_rows=scene_rows, attn_cap=attn_cap, steps=0, graph=None, flat=flat, prefix=prefix,
                  gen=self.decode_gen, k=k, v=v,              # a state keeps the generation and the encodings it was built with
                  kv="bf16" if scales is None else "fp8", ks=None if scales is None else scales[0], vs=None if scales is None else scales[1],
                  pos=i32([[0] * B] * 3), row=i32([j * scene_rows for j in range(B)]), len=i32([1] * B), tok=i32([0] * B),
                  x=x, qkv=qkv, ao=ao, lin_io=(vec(x), vec(qkv), vec(ao)), act=vec(buf(Fd)), logits=vec(buf(Lc["vocab"])),
                  cos=buf(128, torch.float32), sin=buf(128, torch.float32), amax=torch.zeros(129 * B, dtype=torch.int32, device=d))
        if sample is not None:                               # (seed, temperature): draw instead of argmax, every slot its own stream
            st["rng"] = hip.make_rng(sample[0], sample[1], d)
        if st["gen"] == 2 and B <= 8:
            st["lin"] = _lin_pg(self.w, eps, not flat, self._decode_weights == "fp8")
        elif flat:
            st["lin"] = _lin_gemv1(self.w, eps)
        else:
            st["lin"] = _lin_skinny(self.w, eps, buf(H), torch.zeros(hip.GEMM_WS_WORDS, dtype=torch.int32, device=d))
        st["attn"] = self._attention(st, prefix)
        return st

    def _capture(self, st):
        """Capture the step of `st` into st["graph"] (after one warm-up step whose state changes are undone)."""
        init = {n: st[n].clone() for n in ("pos", "row", "len", "tok") + (("rng",) if st.get("rng") is not None else ())}
        s = torch.cuda.Stream(device=self.dev)               # warm up once on a side stream: lazy module loads must not
        s.wait_stream(torch.cuda.current_stream())           # happen during capture
        with torch.cuda.stream(s):
            self._step(st)
        torch.cuda.current_stream().wait_stream(s)
        for n, t in init.items():
            st[n].copy_(t)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step(st)
        st["graph"] = g

    # ------------------------------------------------------------------ batch-1 decode
    def decode_begin(self, cache, start_token, pos, max_new_tokens, use_graph=True, sample=None):
        """Point the device-side decode state at the first step after `cache` (a prefilled KVCache).

        use_graph: the step is replayed from a hipGraph.  Capturing it (a warm-up step, ~200 launches recorded, the graph
        instantiated) costs ~10 ms, 5 % of a 128-token answer, so the captured step is kept: it runs over an engine-owned
        KV block sized in 4096-row buckets, the caller's prefill rows are copied into it (630 MB at 11 k rows: 0.3 ms) and
        `decode_end` copies the appended rows back, which keeps NaiveCache's append semantics (qwen2vl.py:626-634) for the
        caller's cache.  Eager mode decodes in the caller's cache directly.

        decode_kv == "fp8": graph and eager alike decode in an engine-owned e4m3 block (KV8Cache) - the caller's rows are
        quantised into it (one kernel per layer and tensor in place of the copy), `decode_end` returns the appended rows
        dequantised; eager mode only skips the capture.

        sample = (seed, temperature): the next token is drawn from softmax(logits / temperature) (the reference's
        do_sample branch, g2vlm.py:1119-1122) instead of argmax; the sampler state lives on the device like the rest."""
        d = self.dev
        kv_len = cache.length
        need = kv_len + max_new_tokens + 1
        cap = (need + 4095) // 4096 * 4096                    # the attention splits its keys by this bucket: graph and eager alike
        kv8 = self._decode_kv == "fp8"
        if not use_graph and not kv8:
            cache.reserve(cap)
            st = self._decode_state(1, cache.k, cache.v, cache.capacity, cap, sample, flat=True)
            st.update(cache=cache, user_cache=None)
        else:
            # an e4m3 state is kept for eager mode too, hence use_graph (always True with a bf16 cache); the weight mode stays last
            key = (cap, sample is not None, bool(use_graph), self._decode_gen, self._decode_kv, self._decode_weights)
            st = self._decode_cached.get(key)
            if st is None:
                self._decode_cached.clear()                   # one bucket resident (0.35-0.6 GB each)
                if kv8:
                    own = KV8Cache(len(cache.k), 1, cap, self.dims["llm"]["kv_heads"], d)
                    st = self._decode_state(1, own.k, own.v, cap, cap, sample, flat=True, scales=(own.ks, own.vs))
                else:
                    own = KVCache(len(cache.k), self.dims["llm"]["kv_heads"], d, capacity=cap)
                    st = self._decode_state(1, own.k, own.v, own.capacity, cap, sample, flat=True)
                st["cache"] = own
                if use_graph:
                    self._capture(st)
                self._decode_cached[key] = st
            own = st["cache"]
            if kv8:
                own.put(0, cache, kv_len)
            else:
                for i in range(len(cache.k)):
                    own.k[i][:kv_len].copy_(cache.k[i][:kv_len]); own.v[i][:kv_len].copy_(cache.v[i][:kv_len])
            own.length = kv_len
            st["user_cache"] = cache
        st["pos"].fill_(pos); st["row"].fill_(kv_len); st["len"].fill_(kv_len + 1); st["tok"].fill_(int(start_token))
        if sample is not None:
            st["rng"].copy_(hip.make_rng(sample[0], sample[1], d))      # step 0 of this call's stream (the capture warm-up drew once)
        st["base_len"], st["steps"] = kv_len, 0
        return st

    def decode_step(self, st):
        """Run one token.  Returns the device tensor holding the NEXT token id (int32 [1], overwritten every step)."""
        self.decode_step_batch(st)
        st["cache"].length = st["base_len"] + st["steps"]
        return st["tok"]

    def decode_end(self, st):
        """Give the caller's cache the rows the decode appended (graph mode, and either mode with an e4m3 cache, decodes in an
        engine-owned block; from an e4m3 block the rows come back dequantised: what the decode attended to)."""
        user = st.get("user_cache")
        if user is None:
            return
        lo, hi = st["base_len"], st["base_len"] + st["steps"]
        user.reserve(hi)
        own = st["cache"]
        if st["kv"] == "fp8":
            own.get(0, lo, hi, user)
        else:
            for i in range(len(user.k)):
                user.k[i][lo:hi].copy_(own.k[i][lo:hi]); user.v[i][lo:hi].copy_(own.v[i][lo:hi])
        user.length = hi
        st["user_cache"] = None

    # ------------------------------------------------------------------ batched decode
    # One token for each of B scenes (same weights, one KV cache each): the reference loop body with its batch = 1 limit
    # lifted.  Weights are streamed once per step for all scenes; the packed cache [B * cap] is addressed by row.
    def _open_slots(self, n_slots, cap_rows, sample, prefix=None):
        Lc = self.dims["llm"]
        B = int(n_slots)
        if not (1 <= B <= 64):
            raise ValueError("batched decode: 1..64 scene slots")
        cap = (int(cap_rows) + 63) // 64 * 64
        if self._decode_kv == "fp8" and prefix is None:      # a shared-prefix state keeps bf16 blocks (decode_begin_shared)
            own = KV8Cache(Lc["layers"], B, cap, Lc["kv_heads"], self.dev)
            st = self._decode_state(B, own.k, own.v, cap, cap, sample, scales=(own.ks, own.vs))
            st["cache8"] = own
            return st
        kv = lambda: [torch.zeros((B, cap, Lc["kv_heads"], 128), dtype=torch.bfloat16, device=self.dev) for _ in range(Lc["layers"])]  # noqa: E731
        return self._decode_state(B, kv(), kv(), cap, cap, sample, prefix=prefix)

    def decode_open_slots(self, n_slots, cap_rows, use_graph=True, sample=None):
        """Device-side state of a batched decode with `n_slots` scene slots of `cap_rows` cache rows each, all idle
        (an idle slot attends to one zero key; its row of every GEMM is independent of the others and its ids are
        ignored).  Scenes enter and leave through decode_set_slot while the captured step keeps replaying: the graph
        only holds pointers into this state."""
        st = self._open_slots(n_slots, cap_rows, sample)
        if use_graph:
            self._capture(st)
        return st

    def decode_set_slot(self, st, j, cache, start_token, position, max_new_tokens):
        """Put a prefilled scene into slot j: copy its cache rows into the slot's block and point the slot's device-side
        state at its first decode step.  Runs between replays of the captured step (same stream)."""
        n, cap = cache.length, st["cap"]
        if n + max_new_tokens + 1 > cap:
            raise ValueError(f"scene needs {n + max_new_tokens + 1} cache rows, the slots hold {cap}")
        if st["kv"] == "fp8":                                # quantised on the way in
            st["cache8"].put(j, cache, n)
        else:
            for i in range(len(st["k"])):
                st["k"][i][j, :n].copy_(cache.k[i][:n]); st["v"][i][j, :n].copy_(cache.v[i][:n])
        st["pos"][:, j] = int(position)
        st["row"][j] = j * cap + n
        st["len"][j] = n + 1
        st["tok"][j] = int(start_token)

    def decode_idle_slot(self, st, j):
        """Park slot j (its scene left): the captured step keeps advancing every slot, so an idle one is rewound to its
        first row before it can run past its block.  In an e4m3 cache that row becomes zero codes with scale 1."""
        if st["kv"] == "fp8":
            st["cache8"].clear_row0(j)
        st["pos"][:, j] = 0
        st["row"][j] = j * st["cap"]
        st["len"][j] = 1
        st["tok"][j] = 0

    def decode_begin_batch(self, caches, start_tokens, positions, max_new_tokens, use_graph=True, sample=None):
        """Pack B prefilled caches into one [B, cap, Hkv, 128] block per layer and set up the device-side decode state.
        caches: list of KVCache (one per scene, after their prefills); start_tokens / positions: one int per scene."""
        B = len(caches)
        if not (1 <= B <= 64) or len(start_tokens) != B or len(positions) != B:
            raise ValueError("decode_begin_batch: 1..64 scenes, one start token and one position each")
        st = self.decode_open_slots(B, max(c.length for c in caches) + max_new_tokens + 1, use_graph, sample)
        for j, c in enumerate(caches):
            self.decode_set_slot(st, j, c, start_tokens[j], positions[j], max_new_tokens)
        return st

    # ------------------------------------------------------------------ shared-prefix decode (several questions, one scene)
    def decode_begin_shared(self, prefix_cache, suffixes, start_tokens, positions, max_new_tokens, use_graph=True, sample=None):
        """Batched decode of B questions about one scene.  prefix_cache: the KVCache of the shared rows (system prompt,
        views), read in place and never written; suffixes[j]: a KVCache holding question j's own prefilled rows (the rows
        that follow the prefix in its single-question cache); start_tokens / positions: one int per question.
        The state is decode_open_slots' with [B, cap_s, Hkv, 128] suffix blocks (cap_s: the longest question plus
        max_new_tokens + 1) in place of whole-scene blocks; the attention (g2v_decode_attn_shared) reads the prefix once
        per step for all questions.  Nothing allocated here depends on the prefix length.  The captured graph holds
        pointers into prefix_cache: it must not be reallocated while this state decodes.
        The prefix is the caller's bf16 cache, so these states keep bf16 suffix blocks whatever decode_kv says: the setting
        is without effect here (an e4m3 prefix would be a second copy of the scene's rows)."""
        B = len(suffixes)
        if not (1 <= B <= 64) or len(start_tokens) != B or len(positions) != B:
            raise ValueError("decode_begin_shared: 1..64 questions, one start token and one position each")
        if prefix_cache.length < 1:
            raise ValueError("decode_begin_shared: empty prefix")
        st = self._open_slots(B, max(c.length for c in suffixes) + max_new_tokens + 1, sample, prefix=prefix_cache)
        for j, c in enumerate(suffixes):
            self.decode_set_slot(st, j, c, start_tokens[j], positions[j], max_new_tokens)
        if use_graph:
            self._capture(st)
        return st

    def decode_step_batch(self, st):
        """One token per scene.  Returns the device tensor of NEXT token ids (int32 [B], overwritten every step)."""
        if st["graph"] is not None:
            st["graph"].replay()
        else:
            self._step(st)
        st["steps"] += 1
        return st["tok"]
