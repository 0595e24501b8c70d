"""GPU: every row of the scoring passes against the precise oracle (tests/score_check.py).

One test over score_check.CASES.  A case fills a scene's KVCache with synthetic rows of the cache's own scale (rows [0, P): the
scene; every row from P to the capacity: finite stale rows, so a key too many or a read of a row not yet written changes the
result) and scores through the public entry points: G2VLM.score_continuations / score_questions on TINY (they call
Engine.score_rows / score_questions), pack_continuations / pack_questions + Engine.score_rows / score_questions at the real
widths (one layer, vocabulary 2048).  engine.llm_forward and hip.logprob_rows_bf16 are wrapped by pass-through recorders, so the
engine's OWN final-norm rows and logit rows are seen; no launch and no line of the engine changes.  The new K / V rows are read
from cache rows [P, P + L) after the pass.  The precise and the bf16 oracle then evaluate the same scene and tokens on the host -
one sequential causal pass per (question, choice), none of the engine's window or packing code - and block_check.verdict is
applied at M_SCORE = 1.346 per output kind (final_norm, logits, each layer's K and V rows), rows = the packed rows.  M_SCORE is
measured on the oracle alone (tests/test_score_check_cpu.py).

Exact checks, under no margin: logprobs and logsumexp against fp64 on the engine's own logit rows (tests/test_logprob_gpu.py's
bound); ranks exact, top ids and top values bit-exact against tests/test_topk_gpu.py's stable key sort of those rows;
top_logprobs == top values - lse in fp32; every dict of the wrappers is the right slice of the engine's tensors, total the fp64
sum of its logprobs; the targets the logprob launch was given are the choices' ids; cache.length == P on return; rows [0, P) keep
their bits, and the rows from P + L on where nothing was reallocated; every row [P, P + L) of every layer was written (where the
pass has to reallocate the cache - capacity exactly P - the stale fill behind P is gone with the old buffers, so these two checks
have nothing to look at: there the scene rows [0, P) are held to their bits and the written rows to the K / V verdicts); lm_head
takes the skinny form up to 64 rows and a tiled form from 65 (hip.gemm_route).  A question's rows and a choice's results keep
their bits when the other questions' ids change, when the question is scored alone and when the questions are permuted; 34
distinct layouts back to back (two more than the engine keeps plans for) and the first again give the bits each gives on its own.

Measured on an MI355X, largest over the cases of a family (max e / max b, median e / median b), all within M_SCORE = 1.346:
  score_rows TINY 1.087 / 1.136 (9 cases), real widths 1.002 / 1.016 (1); score_questions TINY 1.093 / 1.084 (7), real widths
  1.024 / 1.000 (1); every layer-0 K / V row 1.00.  19 cases in 1.6 s, the slowest 0.44 s (it builds the real-width engine); the
  24 tests of the module 4.4 s.  Every exact check holds on every case, P = 0 included; no engine bug was found.  Wrong windows
  given to the engine by hand are seen (7.8 and 9.1).  The module prints the ratios of every case and, at its end, the largest per
  family.  DESIGN 6s."""
import json
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_check as B  # noqa: E402
import score_check as C  # noqa: E402

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
    print("\n[score rows] largest (max e / max b, median e / median b, cases) per family: "
          + json.dumps({k: [round(v[0], 3), round(v[1], 3), v[2]] for k, v in worst.items()}))
    if TIMES:
        slow = max(TIMES, key=TIMES.get)
        print(f"[score rows] {len(TIMES)} cases in {sum(TIMES.values()):.1f} s, the slowest {slow} {TIMES[slow]:.2f} s")


def i32(v):
    return torch.as_tensor(v, dtype=torch.int32).to(DEV)


class Recorder:
    """Pass-through wrappers of engine.llm_forward, hip.logprob_rows_bf16 and the two Engine entry points: what they were given
    and what they returned, cloned behind the call; and of hip.gemm_bf16: what hip.gemm_route says of the same arguments."""

    def __init__(self, monkeypatch, eng):
        from g2vlm_amd import hip
        self.h, self.logits, self.targets, self.res, self.windows, self.routes = [], [], [], [], [], []
        fwd, lp, gemm = eng.llm_forward, hip.logprob_rows_bf16, hip.gemm_bf16

        def gemm_bf16(*a, **kw):
            self.routes.append(hip.gemm_route(*a, **kw))
            return gemm(*a, **kw)

        def llm_forward(*a, **kw):
            h = fwd(*a, **kw)
            self.h.append(h.clone())
            self.windows.append(kw.get("windows"))
            return h

        def logprob_rows_bf16(logits, targets, **kw):
            out = lp(logits, targets, **kw)
            self.logits.append(logits.clone())
            self.targets.append(targets.clone())
            return out
        monkeypatch.setattr(eng, "llm_forward", llm_forward)
        monkeypatch.setattr(hip, "logprob_rows_bf16", logprob_rows_bf16)
        monkeypatch.setattr(hip, "gemm_bf16", gemm_bf16)
        for name in ("score_rows", "score_questions"):
            def entry(*a, _f=getattr(eng, name), **kw):
                res = _f(*a, **kw)
                self.res.append(res)
                return res
            monkeypatch.setattr(eng, name, entry)


def scene_cache(eng, case, K=None, V=None):
    """The scene's KVCache: rows [0, P) the scene, every further row up to the capacity a finite stale row."""
    from g2vlm_amd.decode import KVCache
    Lc = eng.dims["llm"]
    if K is None:
        K, V = C.scene_rows(case)
    cap = C.capacity(case)
    c = KVCache(Lc["layers"], Lc["kv_heads"], DEV, capacity=cap)
    for i in range(Lc["layers"]):
        c.k[i].copy_(K[i, :cap]); c.v[i].copy_(V[i, :cap])
    c.length = case["P"]
    return c


def call(case, eng, model, cache, questions, top_k):
    """The pass through the public entry points.  Returns (dicts per question or None, flat segment lengths)."""
    from g2vlm_amd.engine import pack_continuations, pack_questions
    P = case["P"]
    segs = [n for _, s in case["layout"] for n in s]
    if case["kind"] == "rows":
        _, _, start, spos, conts = questions[0]
        if model is not None:
            gi = dict(packed_start_tokens=torch.tensor([start]), packed_query_position_ids=torch.full((3, 1), spos), key_values_lens=torch.tensor([P]))
            return [model.score_continuations(cache, gi, conts, top_k=top_k)], segs
        ids, pos, seg_lens, targets = pack_continuations(start, spos, conts)
        assert list(seg_lens) == segs
        eng.score_rows(cache, P, i32(ids), i32(pos).expand(3, -1).contiguous(), seg_lens, i32(targets), top_k=top_k)
        return None, segs
    if model is not None:
        qs = []
        for text, tpos, start, spos, conts in questions:
            ti = dict(packed_text_ids=torch.tensor(text), packed_text_position_ids=torch.tensor(tpos).expand(3, -1), key_values_lens=torch.tensor([P]))
            gi = dict(packed_start_tokens=torch.tensor([start]), packed_query_position_ids=torch.full((3, 1), spos),
                      key_values_lens=torch.tensor([P + len(text)]))
            qs.append((ti, gi, conts))
        return model.score_questions(cache, qs, top_k=top_k), segs
    ids, pos, layout, targets = pack_questions(questions)
    assert tuple(layout) == case["layout"]
    eng.score_questions(cache, P, i32(ids), i32(pos).expand(3, -1).contiguous(), layout, i32(targets), top_k=top_k)
    return None, segs


def run_pass(case, eng, model, monkeypatch, questions=None, scene=None):
    """One recorded pass of a case with every exact check.  Returns {final_norm, logits, k{i}, v{i}} on the host and the
    engine's result tuple (host)."""
    from g2vlm_amd import hip
    questions = questions if questions is not None else C.tokens(case)
    K, V = scene if scene is not None else C.scene_rows(case)
    Lc = eng.dims["llm"]
    Ly, P, top_k = Lc["layers"], case["P"], case["top_k"]
    Lq, L, starts, chs = C.sizes(case)
    cache = scene_cache(eng, case, K, V)
    cap0 = cache.capacity
    before = [(cache.k[i].clone(), cache.v[i].clone()) for i in range(Ly)]
    rec = Recorder(monkeypatch, eng)
    dicts, segs = call(case, eng, model, cache, questions, top_k)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(rec.h) == len(rec.logits) == len(rec.res) == 1, "one llm_forward, one logprob launch, one Engine entry"
    h, logits, res = rec.h[0], rec.logits[0], [t.cpu() for t in rec.res[0]]
    assert h.shape == (L, Lc["hidden"]) and h.dtype == torch.bfloat16 and logits.shape == (L - Lq, Lc["vocab"])
    assert len(res) == (5 if top_k else 2) and bool(torch.isfinite(h.float()).all()) and bool(torch.isfinite(logits.float()).all())
    # the targets the launch was given; logprobs, lse, ranks, top-k against the engine's own logit rows
    targets = [int(t) for j, c, b, n in chs for t in questions[j][4][c]]
    assert rec.targets[0].cpu().tolist() == targets
    lp, rank = res[:2]
    lse, top_ids, top_vals = res[2:] if top_k else (None, None, None)
    assert lp.dtype == torch.float32 and rank.dtype == torch.int32 and lp.shape == rank.shape == (L - Lq,)
    top_lp = torch.cat([d["top_logprobs"] for q in dicts for d in q]) if (dicts is not None and top_k) else None
    bad = C.exact_scores(logits.cpu(), targets, lp, rank, lse, top_ids, top_vals, top_lp)
    assert not bad, bad
    if top_k:
        assert top_ids.shape == top_vals.shape == (L - Lq, top_k) and top_ids.dtype == torch.int32 and top_vals.dtype == torch.float32
    # the wrappers' dicts: the right slices, bit for bit
    if dicts is not None:
        assert [len(q) for q in dicts] == [len(s) for _, s in case["layout"]]
        bad = C.check_dicts([d for q in dicts for d in q], res, segs)
        assert not bad, bad
    # lm_head's route: the last GEMM of the pass, behind the four of every layer
    n = L - Lq
    assert len(rec.routes) == 4 * Ly + 1
    assert (rec.routes[-1][0] == "skinny") == (n <= 64), (n, rec.routes[-1])
    # the cache
    assert cache.length == P
    grown = cache.capacity != cap0
    assert grown == (cap0 < P + L) and cache.capacity >= P + L
    new = list(range(P, P + L))
    for i in range(Ly):
        for name, t, b4 in (("k", cache.k[i], before[i][0]), ("v", cache.v[i], before[i][1])):
            if grown:
                assert P == 0 or not C.touched_rows(b4[:P], t[:P], [], 1), f"{name}{i}: a scene row changed"
            else:
                badr = C.touched_rows(b4, t, new, 1)
                assert not badr, f"{name}{i} changed in rows {badr[:8]} (allowed [{P}, {P + L}))"
                same = (t[P:P + L].view(torch.int16) == b4[P:P + L].view(torch.int16)).flatten(1).all(dim=1).nonzero().flatten().tolist()
                assert not same, f"{name}{i}: rows {[P + r for r in same][:8]} still hold their stale fill"
    got = dict(final_norm=h.float().cpu(), logits=logits.float().cpu())
    for i in range(Ly):
        got[f"k{i}"] = cache.k[i][P:P + L].flatten(1).float().cpu()
        got[f"v{i}"] = cache.v[i][P:P + L].flatten(1).float().cpu()
    got["windows"], got["routes"] = rec.windows[0], rec.routes
    return got, res


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_scoring_passes_against_the_precise_oracle(case, tiny, engines, monkeypatch):
    t0 = time.perf_counter()
    eng = engines(case["dims"])
    with torch.no_grad():
        got, res = run_pass(case, eng, tiny if case["dims"] == "tiny" else None, monkeypatch)
    cid = C.case_id(case)
    wins, routes = got.pop("windows"), got.pop("routes")
    per_rows = {}
    for w in wins:
        per_rows[(w[0], w[1])] = per_rows.get((w[0], w[1]), 0) + 1
    want = {0: {1}, 1: {2}}[min(case["P"], 1)] if case["kind"] == "rows" else {1: {2, 3}, 0: {1, 2}}[min(case["P"], 1)]
    assert set(per_rows.values()) == want, per_rows          # one, two or three windows share their query rows
    if case["exact_only"]:
        TIMES[cid] = time.perf_counter() - t0
        print(f"\n[score rows] {cid} ({TIMES[cid]:.2f} s): exact checks only", end="")
        return
    ok, vres, msg = C.judge(case, got, C.reference(case), C.M_SCORE)
    RATIOS[cid] = (f"{case['kind']}_{case['dims']}",) + C.worst(vres)
    TIMES[cid] = time.perf_counter() - t0
    print(f"\n[score rows] {cid} ({TIMES[cid]:.2f} s; GEMMs {sorted({r[0] for r in routes[:-1]})}, lm_head {routes[-1][0]}): " + ", ".join(f"{k} {v['ratio_max']:.2f} / {v['ratio_med']:.2f}" for k, v in vres.items()), end="")
    assert ok, msg


def test_a_case_without_a_scene_is_what_the_entry_point_says(tiny):
    """P = 0: score_windows has the branch (no prefix window).  The parametrised case above holds the result; here the entry point's
    own contract: cache.length == 0 on return and nothing but rows [0, L) written."""
    case = next(c for c in C.CASES if c["P"] == 0)
    eng = tiny.engine
    cache = scene_cache(eng, dict(case, cap="larger"))
    before = [(cache.k[i].clone(), cache.v[i].clone()) for i in range(len(cache.k))]
    from g2vlm_amd.engine import pack_continuations
    _, _, start, spos, conts = C.tokens(case)[0]
    ids, pos, seg_lens, targets = pack_continuations(start, spos, conts)
    with torch.no_grad():
        lp, rank = eng.score_rows(cache, 0, i32(ids), i32(pos).expand(3, -1).contiguous(), seg_lens, i32(targets))
    torch.cuda.synchronize()
    assert cache.length == 0 and bool(torch.isfinite(lp).all())
    for i, (k4, v4) in enumerate(before):
        assert not C.touched_rows(k4, cache.k[i], range(len(ids)), 1), f"k{i}"
        assert not C.touched_rows(v4, cache.v[i], range(len(ids)), 1), f"v{i}"


def test_wrong_windows_made_by_hand_are_seen(tiny, monkeypatch):
    """The engine given wrong windows by hand - in bounds, finite, every exact check still holds - is flagged as the planted
    faults predict: a choice's window onto its question one key short (offenders: choice rows only), and the scene window one
    key long, reading cache row P (packed row 0's K / V, written by the same pass).
    Measured on an MI355X: largest ratios 7.8 and 9.1 against M_SCORE = 1.346."""
    from g2vlm_amd import engine as E
    eng = tiny.engine
    qw, sw = E.question_windows, E.score_windows

    def question_one_short(prefix_len, layout):
        Lq = sum(m for m, _ in layout)
        return tuple((q0, n, k0, k - 1, c) if (q0 >= Lq and not c and k0 >= prefix_len and k >= 2) else (q0, n, k0, k, c)
                     for q0, n, k0, k, c in qw(prefix_len, layout))

    def prefix_one_long(prefix_len, seg_lens):
        return tuple((q0, n, k0, k + 1, c) if (k0 == 0 and not c) else (q0, n, k0, k, c) for q0, n, k0, k, c in sw(prefix_len, seg_lens))
    for name, fn, bad, cid in (("question_windows", qw, question_one_short, "questions_P63_2q1+2_65q3_tiny_k0_fit"),
                               ("score_windows", sw, prefix_one_long, "rows_P63_0q2+63_tiny_k0_fit")):
        case = next(c for c in C.CASES if C.case_id(c) == cid)
        assert bad(case["P"], case["layout"] if name == "question_windows" else case["layout"][0][1]) != \
            fn(case["P"], case["layout"] if name == "question_windows" else case["layout"][0][1])
        monkeypatch.setattr(E, name, bad)
        with torch.no_grad():
            got, _ = run_pass(case, eng, tiny, monkeypatch)      # undoes the patch behind the pass
        assert getattr(E, name) is fn
        ok, res, msg = C.judge(case, got, C.reference(case), C.M_SCORE, "wrong " + name)
        print(f"\n[score rows] {name} wrong by hand on {cid}: largest ratio {max(C.worst(res)):.1f}", end="")
        assert not ok
        if name == "question_windows":
            named = C.offenders(case, res)
            assert named and named <= C.fault_rows("question_window_one_short", case), sorted(named)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def key_splits(eng, wins, case, j):
    """How the attention plan of a pass cuts the key tiles of question j's windows into pieces: sorted (window, head, first key
    tile, end key tile), the window named by what it is (query rows relative to the question / its choices; scene, question or
    self keys) and not by where it sits in the packing."""
    plan = eng._tiles[(tuple(wins), eng.dims["llm"]["heads"])]
    Lq, L, starts, chs = C.sizes(case)
    P, a, m = case["P"], starts[j], case["layout"][j][0]
    tail = [r for jj, c, b, n in chs if jj == j for r in range(b, b + n)]
    tiles = plan.tiles.cpu().view(-1, 8).tolist()
    out = []
    for segs, _, _ in plan.phases:
        for d, h, kt0, kt1 in segs.cpu().view(-1, 8)[:, :4].tolist():
            q0, _, k0 = tiles[d][:3]
            if a <= q0 < a + m or q0 in tail:
                rows = ("q", q0 - a) if q0 < Lq else ("c", tail.index(q0))
                keys = "scene" if k0 == 0 and P else "question" if (k0 == P + a and q0 >= Lq) else "self"
                if kt1 > kt0:
                    out.append((rows, keys, h, kt0, kt1))
    return sorted(out)


@pytest.mark.parametrize("P", [60, 65])
def test_a_questions_bits_depend_on_nothing_but_the_question(P, tiny, monkeypatch):
    """Question 1 of three (rows and choices of differing lengths): its final-norm rows, its K / V rows, its choices' logit
    rows, log-probabilities, logsumexp, ranks and top-5 keep their bits when (a) the other questions' ids and choices change,
    (b) it is scored alone, (c) the order of the questions is permuted.

    What the claim rests on.  A row's bits are a function of its inputs, of the form every GEMM takes (every pass here has at most
    64 rows: the skinny form with the same K split, asserted with hip.gemm_route on every GEMM of every pass) and of how the
    attention plan cuts the key tiles of the row's windows into pieces: the plan balances the (item, 64-key tile) units of the
    WHOLE pass over its workgroups (hip._schedule_items), a window of two or more key tiles may be cut between them, and the
    partial results of the pieces are merged by (max, sum) - another legitimate order of the same fp32 sums (M_TABLE's `w`).
    At P = 60 every window of these layouts is one key tile, which cannot be cut: the bits must hold in all three situations.
    At P = 65 the scene window is two key tiles: the bits must hold wherever the plan cuts question 1's windows as in the
    reference pass (read back from the plan's segment table), which (a) does by construction.  Where the cut differs, k0 and v0
    must still keep their bits (layer-0 K / V do not pass through attention), nothing but the outputs behind the first
    attention may move, and the whole pass is held to the oracle of ITS layout and tokens at M_SCORE: a dependence on the
    packing position that is more than another order of the same sums is reported there.
    Measured on an MI355X: P = 60 all three bit-identical; P = 65 (a) and (c) cut alike and bit-identical, (b) cut differently:
    k0 / v0 keep their bits, final_norm, k1, v1, the logits and what is computed from them do not; that pass against the oracle of
    its own layout: 1.114 / 1.057 (M_SCORE = 1.346)."""
    eng = tiny.engine
    base = dict(kind="questions", dims="tiny", P=P, layout=((3, (2, 1)), (5, (3, 2, 1)), (2, (1, 2))), top_k=5, cap="larger", exact_only=False)
    scene = C.scene_rows(base)
    qs = C.tokens(base)
    V = eng.dims["llm"]["vocab"]

    def mine(case, questions, j):
        """Everything of question j in a recorded pass, by name; the GEMM routes of the pass; the key splits of its windows."""
        got, res = run_pass(case, eng, tiny, monkeypatch, questions, scene)
        Lq, L, starts, chs = C.sizes(case)
        m = case["layout"][j][0]
        rows = list(range(starts[j], starts[j] + m))
        tail = [r for jj, c, b, n in chs if jj == j for r in range(b, b + n)]
        out = {}
        for name in ("final_norm", "k0", "v0", "k1", "v1"):
            out[name] = got[name][rows + tail]
        t = torch.tensor([r - Lq for r in tail])
        out["logits"] = got["logits"][t]
        for name, x in zip(("logprobs", "ranks", "lse", "top_ids", "top_vals"), res):
            out[name] = x[t]
        return out, [(r[0],) + tuple(r[2:]) for r in got["routes"]], key_splits(eng, got["windows"], case, j), got

    with torch.no_grad():
        ref, r0, s0, _ = mine(base, qs, 1)
        other = [q if j == 1 else ([(t + 1 + 3 * i) % V for i, t in enumerate(q[0])], q[1], q[2], q[3], [[(t + 11) % (V - 64) for t in c] for c in q[4]])
                 for j, q in enumerate(qs)]
        alone = dict(base, layout=(base["layout"][1],))
        perm = dict(base, layout=(base["layout"][2], base["layout"][1], base["layout"][0]))
        assert all(r[0] == "skinny" for r in r0), r0
        held = []
        for what, case, questions, j in (("other ids", base, other, 1), ("alone", alone, [qs[1]], 0), ("permuted", perm, [qs[2], qs[1], qs[0]], 1)):
            got, r1, s1, full = mine(case, questions, j)
            assert r1 == r0, (what, r1, r0)
            diff = [k for k in ref if not same_bits(ref[k], got[k])]
            print(f"\n[score rows] P = {P}, {what}: key tiles cut as in the reference pass: {s1 == s0}; changed bits: {diff or 'none'}", end="")
            if s1 == s0:
                held.append(what)
                assert not diff, f"{what}: {diff} of question 1 changed their bits"
            else:
                assert P > 64, f"{what}: a window of one key tile was cut: {sorted(set(s1) ^ set(s0))[:6]}"
                assert not set(diff) & {"k0", "v0"}, f"{what}: {diff}: layer-0 K / V rows do not depend on attention"
                ref2 = tuple(C.score(C.oracle("tiny", mode), case, questions, scene) for mode in ("precise", "bf16"))
                ok, vres, msg = C.judge(case, full, ref2, C.M_SCORE, what)
                print(f"; against the oracle of this layout: largest ratios {C.worst(vres)[0]:.3f} / {C.worst(vres)[1]:.3f}", end="")
                assert ok, msg
        assert "other ids" in held and (P > 64 or len(held) == 3), held
        assert not same_bits(mine(base, other, 0)[0]["logprobs"], mine(base, qs, 0)[0]["logprobs"])       # the other questions' scores did move


def test_more_layouts_than_plans_are_kept_back_to_back(tiny):
    """SCORE_PLANS_KEPT + 2 distinct small layouts back to back with no wait between them, then the first again: every result has
    the bits that layout gives on its own (the evicted plans' device tables are freed behind the launches that read them)."""
    from g2vlm_amd.engine import pack_continuations
    eng = tiny.engine
    N = eng.SCORE_PLANS_KEPT + 2
    P = 5
    case = dict(kind="rows", dims="tiny", P=P, layout=((0, (N + 3,)),), top_k=5, cap="larger", exact_only=False)
    _, _, start, spos, _ = C.tokens(case)[0]
    V = eng.dims["llm"]["vocab"]
    args = []
    for s in range(N):
        conts = [[(7 + 3 * s + 5 * i) % (V - 64) for i in range(1 + s % 3)], [(11 + s + 2 * i) % (V - 64) for i in range(1 + s // 3)]]
        ids, pos, seg_lens, targets = pack_continuations(start, spos, conts)
        args.append((i32(ids), i32(pos).expand(3, -1).contiguous(), tuple(seg_lens), i32(targets)))
    assert len({a[2] for a in args}) == N
    cache = scene_cache(eng, case)
    with torch.no_grad():
        solo = []
        for a in args:
            torch.cuda.synchronize()
            solo.append([t.cpu() for t in eng.score_rows(cache, P, *a, top_k=5)])
        torch.cuda.synchronize()
        assert len(eng._score_plans) == eng.SCORE_PLANS_KEPT
        order = list(range(N)) + [0]
        runs = [eng.score_rows(cache, P, *args[s], top_k=5) for s in order]      # no wait in between
        torch.cuda.synchronize()
    assert len(eng._score_plans) == eng.SCORE_PLANS_KEPT and cache.length == P
    for s, res in zip(order, runs):
        for name, a, b in zip(("logprobs", "ranks", "lse", "top_ids", "top_vals"), solo[s], res):
            assert same_bits(a, b.cpu()), f"layout {s} ({args[s][2]}): {name} differs from the layout run on its own"
