"""CPU: the margin, the re-orderings and the planted glue faults of tests/block_check.py.  No GPU, nothing of the engine.

  * block_check.M_TABLE / M reproduce: the bf16 oracle's blocks under the six legitimate re-orderings of their fp32 sums, on
    every case of the GPU module (block_check.CASES), max e / max b and median e / median b per variant; M = 1.25 x the largest;
  * the bf16 oracle itself and every re-ordering pass `verdict` at that M on every case;
  * every planted fault (block_check.FAULTS) is run on every case it applies to.  Two columns: (a) verdict's ratios - the
    fault is FLAGGED if verdict fails on every such case; (b) the global rel-L2 of the faulty run against the clean one on the
    stage-end tensors tests/test_e2e_gpu.py bounds, at recon_tiny518_2v's token count (block_check.BIG: 2 views of 21 x 37
    patches, T = 1564), against that module's BOUND - whether the existing suite would have let it through.

Measured (printed by the tests below; DESIGN 6o holds the same tables):
  re-ordering   max e / max b   median e / median b        (largest over the 62 cases x their outputs)
  k2            1.109           1.075
  k4            1.063           1.038
  k8            1.063           1.019
  t32           1.064           1.114
  t64           1.116           1.114
  t128          1.116           1.114          -> M = 1.25 x 1.116 = 1.395

  fault                   cases  (a) largest ratio per case   flagged   (b) global rel-L2 / bound at T = 1564         hidden
  split_off_by_one        13     368 .. 466                   all       last hidden 1.77, K 1.55, V 1.52              no
  window_drops_last_key   40     8.5 .. 108                   all       DINO tokens 0.46, decoder 0.63                yes
  h1_fixed                12     81 .. 182                    all       DINO tokens 3.00                              no
  rope_pos_last_patch     16     16 .. 29                     all       decoder 0.58                                  yes
  kv_row_early            17     344 .. 461                   all       last hidden 0.13, K 4.25, V 4.65              no
  wrong_layer_gamma       18     10.6 .. 20                   all       last hidden 3.44, DINO tokens 4.23            no
  und_bias_dropped        17     6.6 .. 7.3                   all       0.11, 0.28, 0.24                              yes
  context_own_view        4      80 .. 116                    all       decoder 9.08                                  no
  und_rounding_flipped    17     1.00 .. 1.18                 none      0.08, 0.17, 0.14                              yes
Three row-local faults pass the global bounds (and the one-ulp rounding flag, which passes everything): HIDDEN below.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import block_check as B  # noqa: E402
from test_e2e_gpu import BOUND as E2E_BOUND  # noqa: E402
from test_full_depth_gpu import BOUND as FULL_BOUND  # noqa: E402

# planted faults `verdict` does not flag at the measured M, with the largest ratio (max e / max b) over their cases
MISSES = {"und_rounding_flipped": 1.18}
# ... and the ones the global bounds of tests/test_e2e_gpu.py let through at T = 1564 (measured below, then asserted)
HIDDEN = {"window_drops_last_key", "rope_pos_last_patch", "und_bias_dropped", "und_rounding_flipped"}


def setup_module():
    torch.set_num_threads(min(8, os.cpu_count() or 1))


def ratios(case, mode):
    """{output: verdict} of the oracle `mode` (a re-ordering or a fault) on a case, judged at the committed M."""
    inp, _, _ = B.reference(case)
    return B.judge(case, B.run(case, B.oracle(case["dims"], mode), inp), B.M, mode)


def test_the_margin_reproduces():
    table = {}
    for vn in B.VARIANTS:
        mx = md = 0.0
        for case in B.CASES:
            _, res, _ = ratios(case, vn)
            mx = max([mx] + [v["ratio_max"] for v in res.values()])
            md = max([md] + [v["ratio_med"] for v in res.values()])
        table[vn] = (mx, md)
        print(f"\n[margin] {vn}: max e / max b {mx:.3f}, median e / median b {md:.3f}", end="")
    largest = max(max(t) for t in table.values())
    print(f"\n[margin] M = {B.SLACK} x {largest:.3f} = {B.SLACK * largest:.3f} (committed: {B.M})")
    for vn, (mx, md) in table.items():
        # the table is a record of fp32 sums: another BLAS or thread count moves its third digit
        assert abs(mx - B.M_TABLE[vn][0]) < 0.02 and abs(md - B.M_TABLE[vn][1]) < 0.02, (vn, mx, md, B.M_TABLE[vn])
    assert B.M == round(B.SLACK * max(max(t) for t in B.M_TABLE.values()), 3)
    assert abs(B.SLACK * largest - B.M) < 0.02 * B.SLACK


@pytest.mark.parametrize("case", B.CASES, ids=B.case_id)
def test_the_bf16_oracle_and_every_reordering_pass(case):
    inp, prec, ref = B.reference(case)
    ok, _, msg = B.judge(case, ref, B.M, "bf16 oracle")
    assert ok, msg
    for vn in B.VARIANTS:
        ok, _, msg = ratios(case, vn)
        assert ok, msg


def test_verdict_names_the_row_and_its_class():
    case = next(c for c in B.CASES if B.case_id(c) == "mot_geo_tiny_2v_2x3_d1")
    inp, prec, ref = B.reference(case)
    got = {k: v.clone() for k, v in ref.items()}
    first_marker = int(inp["gi"]["packed_text_indexes"][0])
    got["stream"][first_marker] += 0.05 * (prec["stream"][first_marker] - inp["x"][first_marker]).to(got["stream"].dtype)
    ok, res, msg = B.judge(case, got, B.M, "one row 5 % off")
    assert not ok and [r for r, _, _ in res["stream"]["offenders"]] == [first_marker]
    assert "special+split" in msg and f"row {first_marker}" in msg
    # a row that must be zero is compared absolutely, and only zero passes
    z = torch.zeros(4, 8)
    z[1:] = torch.randn(3, 8)
    bad = z.clone(); bad[0, 0] = 1e-6
    assert B.verdict(z * (1 + 1e-3), z * (1 + 1e-3), z, None, {}, B.M)["absolute"] == [0]
    v = B.verdict(bad, z * (1 + 1e-3), z, None, {"h1": [0]}, B.M)
    assert not v["ok"] and v["offenders"][0][:2] == (0, "h1 (absolute)")


def global_rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def hidden_from_the_global_bounds(fault):
    """(hidden?, {tensor: rel-L2 / bound}) of a fault at T = 1564 under the stage-end bounds of the existing suite."""
    figs = {}
    for kind in B.FAULTS[fault]:
        case = B.BIG.get(kind)
        if case is None or not B.fault_applies(fault, case):
            continue
        inp = B.inputs(case, B.oracle("tiny", "precise")) if kind not in _BIG_INP else _BIG_INP[kind]
        _BIG_INP[kind] = inp
        if kind not in _BIG_CLEAN:
            _BIG_CLEAN[kind] = B.run(case, B.oracle("tiny", "bf16"), inp)
        clean, bad = _BIG_CLEAN[kind], B.run(case, B.oracle("tiny", fault), inp)
        if kind.startswith("mot"):
            last = case["depth"] - 1
            figs[kind + ".last_hidden"] = global_rel(bad["final_norm"], clean["final_norm"]) / E2E_BOUND["last_hidden"]
            figs[kind + ".kv_last_k"] = global_rel(bad[f"k{last}"], clean[f"k{last}"]) / E2E_BOUND["geo_kv_last_k"]
            figs[kind + ".kv_last_v"] = global_rel(bad[f"v{last}"], clean[f"v{last}"]) / E2E_BOUND["geo_kv_last_v"]
        elif kind == "dino":
            N, P = case["N"], case["gh"] * case["gw"]
            pick = lambda t: t.view(N, P + 5, -1)[:, 5:]     # noqa: E731  (dino_tokens: the patch rows)
            figs["dino.dino_tokens"] = global_rel(pick(bad["final_ln"]), pick(clean["final_ln"])) / E2E_BOUND["dino_tokens"]
        else:
            figs["dec.global_hidden"] = global_rel(bad["out"], clean["out"]) / FULL_BOUND["global_hidden"]
    # the bounds are about twice what a clean engine measures, so a fault stays under them while it adds less than
    # sqrt(1 - 1 / 4) = 0.87 of a bound to the clean half
    return all(f < 0.87 for f in figs.values()), figs


_BIG_INP, _BIG_CLEAN = {}, {}


def test_every_planted_fault_on_every_case_it_applies_to():
    missed, hidden = {}, set()
    for fault in B.FAULTS:
        cases = [c for c in B.CASES if B.fault_applies(fault, c)]
        assert cases, fault
        flags, worst = [], []
        for case in cases:
            ok, res, _ = ratios(case, fault)
            flags.append(not ok)
            worst.append(max(max(v["ratio_max"] / 1.0, v["ratio_med"]) for v in res.values()))
        hid, figs = hidden_from_the_global_bounds(fault)
        if hid:
            hidden.add(fault)
        flagged = all(flags)
        if not flagged:
            missed[fault] = max(worst)
        print(f"\n[fault] {fault}: {len(cases)} cases, verdict fails on {sum(flags)}; largest ratio per case {min(worst):.2f} .. {max(worst):.2f} "
              f"(M = {B.M}) -> {'FLAGGED' if flagged else 'MISSED'}; global rel-L2 / bound at T = 1564: "
              + ", ".join(f"{k} {v:.2f}" for k, v in figs.items()) + f" -> {'HIDDEN from' if hid else 'seen by'} the global bounds", end="")
    print()
    assert not set(B.ROW_LOCAL) & set(missed), missed
    assert set(missed) == set(MISSES) and len(missed) <= 2, missed
    for f, r in missed.items():
        assert abs(r - MISSES[f]) < 0.1 and r < B.M, (f, r)
    assert hidden == HIDDEN and len(hidden) >= 3, hidden
