"""CPU: the step oracle, the margin, the re-orderings, the planted faults and the exact checks of tests/decode_step_check.py.
No GPU, nothing of the engine.

  * `step` on the precise and the bf16 oracle restates the loop body of OracleG2VLM.generate_text and nothing else: over the same
    cache it gives generate_text's ids, and the bf16 one its logits to the bit;
  * M_TABLE / M_DECODE reproduce: the bf16 oracle's step under the eight legitimate re-orderings of its fp32 sums on every case
    of the GPU module (decode_step_check.CASES); the bf16 oracle and every re-ordering pass every case at M_DECODE;
  * every fault of FAULTS is planted on every case it applies to: the ones outside MISSES are flagged on every such case, and
    where the fault sits in some slots only, the verdict names them; the ones in MISSES pass, ratios printed;
  * the exact checks catch a planted "wrote one extra row" and "touched the neighbour's block" on a host mock of the cache.

Measured (printed by the tests below; DESIGN 6r holds the same tables):
  re-ordering   max e / max b   median e / median b        (largest over the 49 cases x their outputs)
  k2            1.044           1.057
  k4            1.051           1.022
  k8            1.026           1.026
  t32           1.001           1.011
  t64           1.010           1.000
  t128          1.010           1.000
  s2            1.045           1.007
  s4            1.045           1.011          -> M_DECODE = 1.25 x 1.057 = 1.321

  fault                      cases  largest ratio per case   flagged
  len_one_short              43     7.8 .. 193               all
  len_one_long               43     5.9 .. 130               all
  kv_row_early               45     53 .. 629                all
  kv_row_late                49     53 .. 639                all
  pos_advanced_early         49     8.7 .. 91                all
  wrong_layer_qk_gamma       43     4.9 .. 35                all
  wrong_layer_ln             43     9.5 .. 43                all
  qkv_bias_dropped           47     1.4 .. 9.4               all
  final_norm_gamma_of_ln2    49     11 .. 40                 all
  slot_reads_neighbour       16     81 .. 256                all
  prefix_last_key_dropped    7      11 .. 136                all
  suffix_first_key_dropped   7      7.2 .. 108               all
  kv8_scale_stale            13     7.8e3 .. 2.9e4           all
  kv8_attends_unquantised    13     1.00 .. 1.05             none (MISSES)
  stale_token                49     105 .. 677               all
  und_rounding_flipped       49     1.00 .. 1.21             none (MISSES)

Cost.  A case has 5 - 45 rows, each one token through 1 - 2 layers (2 - 4 ms on the host, the same on 2, 4 or 8 threads: the matrices
are too small to share out), 797 rows in all; 2 + 8 + 16 oracles go over them.  The file takes 62 s, against 12 s for
tests/test_block_check_cpu.py and 22 s for tests/test_dinov3_block_check_cpu.py; every verdict is computed once and kept (`ratios`).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import decode_step_check as C  # noqa: E402
from oracle.g2vlm_oracle import NaiveCache, OracleG2VLM  # noqa: E402


def setup_module():
    torch.set_num_threads(min(8, os.cpu_count() or 1))


_RATIOS = {}


def ratios(case, mode):
    """(ok, {kind: verdict}, message) of the oracle `mode` (a re-ordering or a fault) on a case at the committed M_DECODE; kept."""
    key = (C.case_id(case), mode)
    if key not in _RATIOS:
        ref3 = C.reference(case)
        _RATIOS[key] = C.judge(case, C.run(case, mode, ref3[0]), ref3, C.M_DECODE, mode)
    return _RATIOS[key]


@pytest.mark.parametrize("which", ["tiny", "real"])
def test_step_restates_the_loop_body_of_generate_text(which):
    case = next(c for c in C.CASES if c["family"] == "b1" and c["dims"] == which and c["kv_len"] == 65 and not C.kv8(c) and not C.weights_q(c))
    _, n, tok, pos, _, seed = C.scenes(case)[0]
    K, V = C.scene_rows(case, seed, n)
    sd, dims = C.state_dict(which, False)
    steps = 6
    for mode in ("bf16", "precise"):
        plain = OracleG2VLM(sd, dims, precise=mode == "precise")
        cache = NaiveCache(plain.num_layers)
        for i in range(plain.num_layers):
            cache.key_cache[i], cache.value_cache[i] = K[i, :n].to(plain.cd), V[i, :n].to(plain.cd)
        ids, logits = plain.generate_text(cache, n, pos, tok, steps, return_logits=True)
        orc = C.oracle(which, False, mode)
        k, v, t = K[:, :n].to(orc.cd), V[:, :n].to(orc.cd), tok
        for s in range(steps):
            assert t == ids[s], (mode, s)
            o = C.step(orc, C.make_state(t, pos + s, list(k), list(v), list(K[:, n:n + 2]), list(V[:, n:n + 2])))
            assert torch.equal(o["logits"], logits[s]), (mode, s, float((o["logits"] - logits[s]).abs().max()))
            assert C.argmax_host(o["logits"]) == o["tok"]
            shape = (k.shape[0], 1) + tuple(k.shape[2:])
            k, v, t = torch.cat([k, o["k"].view(shape).to(orc.cd)], 1), torch.cat([v, o["v"].view(shape).to(orc.cd)], 1), o["tok"]
        for i in range(plain.num_layers):                    # ... and leaves the cache generate_text leaves
            assert torch.equal(k[i], cache.key_cache[i]) and torch.equal(v[i], cache.value_cache[i]), (mode, i)


def test_the_cases_reach_what_they_are_for():
    ids = [C.case_id(c) for c in C.CASES]
    assert len(set(ids)) == len(ids)
    assert {c["family"] for c in C.CASES} == set(C.FAMILIES)
    for c in C.CASES:
        assert 4 <= c["steps"] <= 6
        Hkv = C.dims_of(c)["llm"]["kv_heads"]
        if c["family"] == "split":                           # decode.py's switch between the fused and the split attention
            rows = C.cap_of(c)
            assert (c["B"] * ((rows // 64 + 3) // 4) * Hkv > 512) == (c["cap_rows"] == 14400) and c["gen"] == 1
        if c["family"] in ("slots", "churn"):
            assert c["cap_rows"] % 64 and any(n + c["steps"] + 1 == C.cap_of(c) for _, n, _, _, first, _ in C.scenes(c) if first == 0)
        if c["family"] == "edge":
            assert (c["kv_len"] + c["steps"] - 1, C.cap_of(c)) in ((4094, 4096), (4098, 8192))
    for f in C.MUST_FLAG:
        assert f not in C.MISSES and any(C.fault_applies(f, c) for c in C.CASES), f


def test_the_margin_reproduces():
    table = {}
    for vn in C.VARIANTS:
        mx = md = 0.0
        for case in C.CASES:
            _, res, _ = ratios(case, vn)
            w = C.worst(res)
            mx, md = max(mx, w[0]), max(md, w[1])
        table[vn] = (mx, md)
        print(f"\n[margin] {vn}: max e / max b {mx:.3f}, median e / median b {md:.3f}", end="")
    largest = max(max(t) for t in table.values())
    print(f"\n[margin] M_DECODE = {C.SLACK} x {largest:.3f} = {C.SLACK * largest:.3f} (committed: {C.M_DECODE})")
    for vn, (mx, md) in table.items():
        # the table is a record of fp32 sums: another BLAS or thread count moves its third digit
        assert abs(mx - C.M_TABLE[vn][0]) < 0.02 and abs(md - C.M_TABLE[vn][1]) < 0.02, (vn, mx, md, C.M_TABLE[vn])
    assert C.M_DECODE == round(C.SLACK * max(max(t) for t in C.M_TABLE.values()), 3)
    assert abs(C.SLACK * largest - C.M_DECODE) < 0.02 * C.SLACK


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_the_bf16_oracle_and_every_reordering_pass(case):
    ref3 = C.reference(case)
    rec, prec, ref = ref3
    assert len(C.rows_of(rec)) == sum(len(C.live_slots(case, t)) for t in range(len(rec)))
    for s in (s for states in rec for s in states):          # every state is what the engine would hold: bf16 rows, e4m3-exact if kv8
        assert s["K"][0].dtype == torch.bfloat16 and s["K"][0].shape[0] >= 1
        if s["kv8"]:
            assert torch.equal(C.roundtrip(s["K"][0]), s["K"][0]) and torch.equal(C.roundtrip(s["V"][-1]), s["V"][-1])
    ok, _, msg = C.judge(case, ref, ref3, C.M_DECODE, "bf16 oracle")
    assert ok, msg
    for vn in C.VARIANTS:
        ok, _, msg = ratios(case, vn)
        assert ok, msg


def test_every_planted_fault_on_every_case_it_applies_to():
    missed = {}
    for fault in C.FAULTS:
        cases = [c for c in C.CASES if C.fault_applies(fault, c)]
        assert cases, fault
        flags, worst = [], []
        for case in cases:
            ok, res, msg = ratios(case, fault)
            flags.append(not ok)
            worst.append(max(C.worst(res)))
            if fault == "slot_reads_neighbour":              # wrong in slots >= 1 only: the verdict names them, never slot 0
                rows = C.rows_of(C.reference(case)[0])
                named = {rows[r][0] for v in res.values() for r, _, _ in v["offenders"]}
                assert named and 0 not in named, (C.case_id(case), named)
        flagged = all(flags)
        if not flagged:
            missed[fault] = max(worst)
        print(f"\n[fault] {fault}: {len(cases)} cases, verdict fails on {sum(flags)}; largest ratio per case {min(worst):.2f} .. {max(worst):.2f} "
              f"(M_DECODE = {C.M_DECODE}) -> {'FLAGGED' if flagged else 'MISSED'}", end="")
        if fault in C.MISSES:
            assert not any(flags), (fault, flags)            # a miss passes everywhere: it is below the margin, not near it
    print()
    assert not set(C.MUST_FLAG) & set(missed), missed
    assert set(missed) == set(C.MISSES) and len(missed) <= 2, missed
    for f, r in missed.items():
        assert abs(r - C.MISSES[f]) < 0.1 and r < C.M_DECODE, (f, r)


def test_a_fault_in_one_step_is_named_with_its_slot_and_step():
    case = next(c for c in C.CASES if C.case_id(c) == "slots_B2_cap100_tiny_g2G_w16k16")
    ref3 = C.reference(case)
    rec, prec, ref = ref3
    got = {k: v.clone() for k, v in ref.items()}
    r = C.rows_of(rec).index((1, 3))
    got["stream"][r] += 0.05 * (prec["stream"][r] - prec["emb"][r])
    ok, res, msg = C.judge(case, got, ref3, C.M_DECODE, "one row 5 % off")
    assert not ok and [x for x, _, _ in res["stream"]["offenders"]] == [r]
    assert "slot 1+step 3" in msg and "(1, 3)" in msg
    assert all(v["ok"] for k, v in res.items() if k != "stream")


def test_the_exact_checks_on_a_host_mock_of_the_cache():
    B_, cap, Hkv = 3, 128, 2
    g = torch.Generator().manual_seed(3)
    k = torch.randn((B_, cap, Hkv, 128), generator=g).to(torch.bfloat16)
    ks = torch.ones((B_, cap, Hkv))
    lens = torch.tensor([5, 127, 64], dtype=torch.int32)
    new = [j * cap + int(lens[j]) - 1 for j in range(B_)]
    after, after_s = k.clone(), ks.clone()
    for j in range(B_):
        after[j, lens[j] - 1] = 1.0; after_s[j, lens[j] - 1] = 0.5
    assert C.touched_rows(k, after, new, 2) == [] and C.touched_rows(ks, after_s, new, 2) == []
    extra = after.clone(); extra[0, 5] = 2.0                 # wrote one extra row
    assert C.touched_rows(k, extra, new, 2) == [5]
    nb = after.clone(); nb[2, 0, 1, 7] = -nb[2, 0, 1, 7]     # slot 1, on its last row, touched the neighbour's row 0
    assert C.touched_rows(k, nb, new, 2) == [2 * cap]
    sc = after_s.clone(); sc[1, 3, 0] = 2.0                  # a scale of a past row
    assert C.touched_rows(ks, sc, new, 2) == [cap + 3]
    z = torch.zeros((4, 8)); nz = z.clone(); nz[1, 0] = -0.0   # bits, not values
    assert C.touched_rows(z, nz, [], 1) == [1]
    C.advanced(lens, lens + 1, "len")
    with pytest.raises(AssertionError):
        C.advanced(lens, lens + torch.tensor([1, 2, 1], dtype=torch.int32), "len")
    assert bool(C.is_power_of_two(torch.tensor([0.5, 1.0, 2.0 ** -9])).all()) and not bool(C.is_power_of_two(torch.tensor([0.75, 0.0, 3.0])).any())
    row = torch.tensor([1.0, 3.0, -0.0, 3.0, 0.0])
    assert C.argmax_host(row) == 1 and C.argmax_host(torch.tensor([-0.0, 0.0, -1.0])) == 0
