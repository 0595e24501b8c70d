"""GPU: every decode step of g2vlm_amd/decode.py, slot by slot, against the precise oracle (tests/decode_step_check.py).

One test over decode_step_check.CASES.  A case sets decode_gen / decode_weights / decode_kv, fills synthetic caches (K rows of unit
rms per head, V rows at the scale of a normed projection, the rows behind the live length pre-filled with finite stale rows),
opens the state through the public entry points (decode_begin, decode_open_slots + decode_set_slot + decode_idle_slot,
decode_begin_shared, decode_end) and loops: read the engine's own tok / pos / row / len and the live cache rows of every slot, run
decode_step / decode_step_batch, read st["logits"], st["x"] and the new cache rows, run the exact checks.  Then the precise and the
bf16 oracle evaluate every recorded state on the host and block_check.verdict is applied at M_DECODE = 1.321 per output kind
(logits, the stream's update x - embed[tok], each layer's new K / V row), rows = (slot, step).  M_DECODE is measured on the oracle
alone (tests/test_decode_step_check_cpu.py).  Only what a state already holds is read; no entry point has a tap.

Exact checks, after every step and for every slot: tok is the argmax of the engine's OWN logit row under the kernel's tie rule;
pos, row and len are each one more than before (and at a scene's first step what the entry point was given: a capture warm-up
fully undone, nothing carried over in a cached state); every element of every cache tensor (e4m3 scales, the shared prefix, the
neighbours' blocks, the caller's cache) other than the one new row per layer and slot keeps its bits, compared on the device;
appended e4m3 scales are powers of two; an idle slot writes its row 0 only; decode_end hands the caller exactly the appended rows.

Measured on MI355X, largest over the cases of a family (max e / max b, median e / median b), all within M_DECODE = 1.321:
  batch 1 1.128 / 1.083 (18 cases), bucket edges 1.084 / 1.039 (6), cached state reused 1.056 / 1.050 (2), slots 1.010 / 1.014 (11),
  split attention and its twin 1.000 / 1.000 (3), slot churn 1.000 / 1.000 (2), shared prefix 1.112 / 1.063 (7).
49 cases in 4.3 s (6.6 s with the fixtures), the slowest 0.47 s (b1_kv65_real_g1E_w16k16: it builds the real-width engine).  The
module prints the ratios of every case and, at its end, the largest per family, the total and the slowest case.  No engine bug was
found; wrong calls made to the engine by hand (layer 1 reading layer 0's q / k gammas, the rope table built at pos + 1, the attention
given len + 1) are seen as the planted faults predict: 4.7 - 9.6, 12 - 24, and "k0 changed in rows [66] (allowed [65])".
"""
import json
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_check as B  # noqa: E402
import decode_step_check as C  # noqa: E402

DEV = "cuda"
RATIOS, TIMES = {}, {}


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
    for cid, (fam, mx, md) in RATIOS.items():
        w = worst.setdefault(fam, [0.0, 0.0, 0])
        w[0], w[1], w[2] = max(w[0], mx), max(w[1], md), w[2] + 1
    print("\n[decode steps] largest (max e / max b, median e / median b, cases) per family: "
          + json.dumps({k: [round(v[0], 3), round(v[1], 3), v[2]] for k, v in worst.items()}))
    if TIMES:
        slow = max(TIMES, key=TIMES.get)
        print(f"[decode steps] {len(TIMES)} cases in {sum(TIMES.values()):.1f} s, the slowest {slow} {TIMES[slow]:.2f} s")


def set_modes(eng, case):
    eng.decode_weights, eng.decode_kv = "bf16", "bf16"
    eng.decode_gen = case["gen"]
    eng.decode_weights, eng.decode_kv = case["weights"], case["kv"]


def closure_of(fn):
    return dict(zip(fn.__code__.co_freevars, (c.cell_contents for c in fn.__closure__ or ())))


def user_cache(eng, K, V, n):
    """A caller's KVCache holding rows [0, n) of K / V [L, ., Hkv, 128] (capacity exactly n, at least 1)."""
    from g2vlm_amd.decode import KVCache
    Lc = eng.dims["llm"]
    c = KVCache(Lc["layers"], Lc["kv_heads"], DEV, capacity=max(n, 1))
    for i in range(Lc["layers"]):
        c.k[i].zero_(); c.v[i].zero_()
        c.k[i][:n].copy_(K[i, :n]); c.v[i][:n].copy_(V[i, :n])
    c.length = n
    return c


class Blocks:
    """The cache tensors of a state, addressed by (slot, row): bf16 blocks or e4m3 codes + scales."""

    def __init__(self, st):
        self.st, self.q8 = st, st["kv"] == "fp8"
        self.flat = st["k"][0].dim() == 3                     # batch-1 bf16: [rows, Hkv, 128]
        self.rows = st["k"][0].shape[0] if self.flat else st["k"][0].shape[1]
        self.L = len(st["k"])

    def _sel(self, t, j, lo, hi):
        return t[lo:hi] if self.flat else t[j, lo:hi]

    def read(self, j, lo, hi):
        """(K, V) per layer, rows [lo, hi) of slot j as bf16 on the host (e4m3: codes x scales, exact)."""
        from g2vlm_amd.quant import dequantize_rows
        out = []
        for codes, scales in ((self.st["k"], self.st["ks"]), (self.st["v"], self.st["vs"])):
            per = []
            for i in range(self.L):
                t = self._sel(codes[i], j, lo, hi).cpu()
                if self.q8:
                    s = self._sel(scales[i], j, lo, hi).cpu()
                    t = dequantize_rows(t.reshape(-1, 128), s.reshape(-1)).view(t.shape)
                per.append(t)
            out.append(per)
        return out

    def fill(self, j, lo, K, V):
        """Rows [lo, lo + m) of slot j := K / V [L, m, Hkv, 128] (clipped to the block), quantised for an e4m3 block."""
        from g2vlm_amd import hip
        m = min(K.shape[1], self.rows - lo)
        if m <= 0:
            return
        for i in range(self.L):
            for src, codes, scales in ((K, self.st["k"], self.st["ks"]), (V, self.st["v"], self.st["vs"])):
                rows = src[i, :m].to(DEV).contiguous()
                if self.q8:
                    hip.kv_quant_e4m3(rows, self._sel(codes[i], j, lo, lo + m), self._sel(scales[i], j, lo, lo + m))
                else:
                    self._sel(codes[i], j, lo, lo + m).copy_(rows)

    def tensors(self):
        """{name: (tensor, row dims)} of everything a step may write into or must leave alone."""
        out = {}
        for i in range(self.L):
            for n in ("k", "v") + (("ks", "vs") if self.q8 else ()):
                out[f"{n}{i}"] = (self.st[n][i], 1 if self.flat else 2)
        return out


def snapshot(named):
    return {n: t.clone() for n, (t, _) in named.items()}


def assert_untouched(named, before, allowed, what):
    for n, (t, rd) in named.items():
        bad = C.touched_rows(before[n], t, allowed.get(n, allowed.get("*", [])), rd)
        assert not bad, f"{what}: {n} changed in rows {bad[:8]} (allowed {sorted(allowed.get(n, allowed.get('*', [])))[:8]})"


def run_case(case, eng):
    Lc = eng.dims["llm"]
    L, Hkv, V, H = Lc["layers"], Lc["kv_heads"], Lc["vocab"], Lc["hidden"]
    fam, S, nB, graph = case["family"], case["steps"], case["B"], case["graph"]
    q8 = C.kv8(case)
    set_modes(eng, case)
    scs = C.scenes(case)
    plen = case.get("plen", 0)
    rec, got = [], dict(logits=[], stream=[], **{f"{n}{i}": [] for i in range(L) for n in ("k", "v")})
    extra = {}                                               # tensors outside the state's blocks that no step may touch
    prev_tok = {}

    def begin_b1(sc):
        j, n, tok, pos, first, seed = sc
        K, V_ = C.scene_rows(case, seed, n)
        uc = user_cache(eng, K, V_, n)
        st = eng.decode_begin(uc, tok, pos, S, use_graph=graph)
        assert (st["graph"] is not None) == graph and st["kv"] == ("fp8" if q8 else "bf16") and st["flat"]
        return st, uc, K, V_

    def lin_kind(st):
        return st["lin"].__qualname__.split(".")[0], closure_of(st["lin"]).get("fp8")

    # ---- open the state
    if fam in ("b1", "edge", "reuse"):
        st, uc, K0, V0 = begin_b1(scs[0])
        blocks = Blocks(st)
        assert blocks.rows >= C.cap_of(case) and st["attn_cap"] == C.cap_of(case)
        blocks.fill(0, scs[0][1], K0[:, scs[0][1]:], V0[:, scs[0][1]:])
        want = "_lin_pg" if case["gen"] == 2 else "_lin_gemv1"
        assert lin_kind(st) == (want, C.weights_q(case) if case["gen"] == 2 else None), lin_kind(st)
        if st.get("user_cache") is not None:
            extra.update({f"user.{n}{i}": (t[i], 1) for i in range(L) for n, t in (("k", uc.k), ("v", uc.v))})
        entered = {0: scs[0]}
    elif fam == "shared":
        pk, pv = C.prefix_rows(case)
        prefix = user_cache(eng, pk, pv, plen + 2)           # two stale rows behind the prefix
        prefix.length = plen
        ucs = [user_cache(eng, *C.scene_rows(case, seed, n), n) for _, n, _, _, _, seed in scs]
        st = eng.decode_begin_shared(prefix, ucs, [s[2] for s in scs], [s[3] for s in scs], S, use_graph=graph)
        assert st["kv"] == "bf16" and st["ks"] is None and st["prefix"] is prefix and (st["graph"] is not None) == graph
        assert st["cap"] == C.cap_of(case)
        blocks = Blocks(st)
        for j, n, _, _, _, seed in scs:
            K, V_ = C.scene_rows(case, seed, n)
            blocks.fill(j, n, K[:, n:], V_[:, n:])
        extra.update({f"prefix.{n}{i}": (t[i], 1) for i in range(L) for n, t in (("k", prefix.k), ("v", prefix.v))})
        entered = {s[0]: s for s in scs}
    else:
        st = eng.decode_open_slots(nB, case["cap_rows"], use_graph=graph)
        assert st["cap"] == C.cap_of(case) and st["kv"] == ("fp8" if q8 else "bf16") and (st["graph"] is not None) == graph
        blocks = Blocks(st)
        entered = {}
        for sc in scs:
            j, n, tok, pos, first, seed = sc
            if first == 0:
                K, V_ = C.scene_rows(case, seed, n)
                eng.decode_set_slot(st, j, user_cache(eng, K, V_, n), tok, pos, S)
                blocks.fill(j, n, K[:, n:], V_[:, n:])
                entered[j] = sc
        if fam == "split":                                   # the switch between the fused and the split attention form
            assert (st["attn"].__name__ == "split") == (case["cap_rows"] == 14400), st["attn"].__name__
    if fam not in ("b1", "edge", "reuse"):
        kind, fp8 = lin_kind(st)
        if nB > 8 or case["gen"] == 1:                       # more than 8 slots keep the bf16 skinny Linears whatever decode_weights says
            assert kind == "_lin_skinny", kind
        else:
            assert (kind, fp8) == ("_lin_pg", C.weights_q(case)), (kind, fp8)
    named = dict(blocks.tensors(), **extra)

    T = S * (2 if fam == "reuse" else 1)
    idle = set()
    for t in range(T):
        # ---- what enters or leaves between steps
        if fam == "reuse" and t == S:
            check_decode_end(eng, st, uc, K0, V0, scs[0][1], S, blocks)
            first_st = st
            st, uc, K0, V0 = begin_b1(scs[1])
            assert st is first_st, "the second answer did not reuse the cached captured state"
            extra = {f"user.{n}{i}": (tt[i], 1) for i in range(L) for n, tt in (("k", uc.k), ("v", uc.v))}
            named = dict(blocks.tensors(), **extra)
            entered = {0: scs[1]}                            # the rows behind its 37 are the first answer's: stale by themselves
        if fam == "churn" and t in (2, 3, 4):
            before = snapshot(named)
            mine = {n: list(range(blocks.rows, 2 * blocks.rows)) for n in blocks.tensors()}
            if t == 4:
                j, n, tok, pos, first, seed = scs[-1]
                K, V_ = C.scene_rows(case, seed, n)
                eng.decode_set_slot(st, j, user_cache(eng, K, V_, n), tok, pos, T - t)
                blocks.fill(j, n, K[:, n:], V_[:, n:])
                entered[j] = scs[-1]
                idle.discard(1)
            else:
                eng.decode_idle_slot(st, 1)                  # the step advances an idle slot too: rewound before each of its steps
                idle.add(1)
            assert_untouched(named, before, mine, f"step {t}: changing slot 1")
        live = C.live_slots(case, t)
        assert sorted(set(range(nB)) - idle) == live

        # ---- 1. read the state
        tok0, pos0, row0, len0 = (st[n].clone() for n in ("tok", "pos", "row", "len"))
        tk, ps, rw, ln = tok0.cpu().tolist(), pos0.cpu(), row0.cpu().tolist(), len0.cpu().tolist()
        assert bool((ps == ps[0:1]).all()), ps
        ps = ps[0].tolist()
        states = []
        for j in range(nB):
            assert rw[j] == j * blocks.rows + ln[j] - 1, (t, j, rw[j], ln[j])
            if j in idle:
                assert (tk[j], ps[j], ln[j]) == (0, 0, 1), (t, j)
                continue
            _, n, tok, pos, first, _ = entered[j]
            a = t - first
            assert ln[j] == n + a + 1 and ps[j] == pos + a, (t, j, ln[j], ps[j])
            if a == 0:
                assert tk[j] == tok, (t, j, tk[j], tok)
            Kj, Vj = blocks.read(j, 0, ln[j] - 1)
            bk, bv = blocks.read(j, ln[j] - 1, min(ln[j] + 1, blocks.rows))
            if plen:
                Kj = [torch.cat([prefix.k[i][:plen].cpu(), Kj[i]]) for i in range(L)]
                Vj = [torch.cat([prefix.v[i][:plen].cpu(), Vj[i]]) for i in range(L)]
            states.append(C.make_state(tk[j], ps[j], Kj, Vj, bk, bv, q8, plen, prev_tok.get(j, 0), j, t))
            prev_tok[j] = tk[j]
        rec.append(C.link_neighbours(states))
        before = snapshot(named)

        # ---- 2. the step
        out = eng.decode_step(st) if st["flat"] else eng.decode_step_batch(st)
        torch.cuda.synchronize()
        assert out is st["tok"]

        # ---- 3. its outputs, 4. the exact checks
        logits = st["logits"].view(nB, V).float().cpu()
        x = st["x"].view(nB, H).float().cpu()
        tok1 = st["tok"].cpu().tolist()
        assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(x).all())
        C.advanced(pos0, st["pos"], "pos"); C.advanced(row0, st["row"], "row"); C.advanced(len0, st["len"], "len")
        new_rows = [rw[j] for j in range(nB)]
        assert_untouched(named, before, {n: new_rows for n in blocks.tensors()}, f"step {t}")
        for j in live:
            assert tok1[j] == C.argmax_host(logits[j]), (t, j, tok1[j])
            nk, nv = blocks.read(j, ln[j] - 1, ln[j])
            got["logits"].append(logits[j]); got["stream"].append(x[j])
            for i in range(L):
                got[f"k{i}"].append(nk[i].flatten().float()); got[f"v{i}"].append(nv[i].flatten().float())
            if q8:
                for i in range(L):
                    for sname in ("ks", "vs"):
                        s = blocks._sel(st[sname][i], j, ln[j] - 1, ln[j])
                        assert bool(C.is_power_of_two(s).all()), (t, j, sname, s.cpu().tolist())
    if fam in ("b1", "edge", "reuse"):
        check_decode_end(eng, st, uc, K0, V0, entered[0][1], S, blocks)
    return rec, {k: torch.stack(v) for k, v in got.items()}


def check_decode_end(eng, st, uc, K0, V0, n, S, blocks):
    """decode_end: the caller's rows [lo, hi) are the engine-owned block's (dequantised for e4m3) bit for bit, the rows below lo
    keep theirs, length == hi.  Eager mode with a bf16 cache decodes in the caller's cache: those ARE the rows."""
    owned = st.get("user_cache") is not None
    own_k, own_v = blocks.read(0, n, n + S)
    eng.decode_end(st)
    torch.cuda.synchronize()
    assert uc.length == n + S and st.get("user_cache") is None and (owned or st["cache"] is uc)
    for i in range(blocks.L):
        for user, own, orig in ((uc.k[i], own_k[i], K0[i]), (uc.v[i], own_v[i], V0[i])):
            assert torch.equal(user[n:n + S].cpu().view(torch.int16), own.view(torch.int16)), ("appended rows", i)
            assert torch.equal(user[:n].cpu().view(torch.int16), orig[:n].view(torch.int16)), ("rows below lo", i)


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_decode_steps_against_the_precise_oracle(case, tiny, engines):
    t0 = time.perf_counter()
    eng = engines(case["dims"])
    with torch.no_grad():
        rec, got = run_case(case, eng)
    assert [len(s) for s in rec] == [len(C.live_slots(case, t)) for t in range(len(rec))]
    ok, res, msg = C.judge(case, got, C.reference(case, rec), C.M_DECODE)
    cid = C.case_id(case)
    RATIOS[cid] = (case["family"],) + C.worst(res)
    TIMES[cid] = time.perf_counter() - t0
    print(f"\n[decode steps] {cid} ({TIMES[cid]:.2f} s): " + ", ".join(f"{k} {v['ratio_max']:.2f} / {v['ratio_med']:.2f}" for k, v in res.items()), end="")
    assert ok, msg
