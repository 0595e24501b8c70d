"""CPU: the margin, the re-orderings and the planted glue faults of tests/dinov3_block_check.py.  No GPU, nothing of the engine.

  * M_TABLE / M reproduce: the round_qk bf16 oracle under the six re-orderings of its fp32 sums on every case of the GPU
    module (dinov3_block_check.CASES), max e / max b and median e / median b per variant; M = SLACK x the largest;
  * the round_qk oracle and every re-ordering pass `verdict` at that M on every case; what round_qk alone costs against the
    plain oracle's b_r is measured and asserted (ROUND_QK_COST);
  * every planted fault is run on every case it applies to: (a) verdict's ratios - it must fail on every such case, with the
    offending rows in the class the fault is about; (b) on 2-view cases of the golden fixtures' grids (BIG: 3 x 4, T = 34, and the
    largest, 14 x 14, T = 402) the two quantities tests/test_dinov3_gpu.py bounds: the global rel-L2 of the faulty patch tokens
    against the clean bf16 run as a fraction of 2e-2, and their global error against the precise run as a fraction of 1.5 x the
    clean run's - whether that test would have let the fault through (both fractions <= 1).

Measured (printed by the tests below; DESIGN 6q holds the full tables):
  re-ordering   max e / max b   median e / median b        (largest over the 210 cases x their outputs)
  k2            1.110           1.082
  k4            1.110           1.021
  k8            1.135           1.057
  t32           1.046           1.008
  t64           1.046           1.024
  t128          1.046           1.024          -> M = 1.25 x 1.135 = 1.419
  round_qk against the plain oracle's b_r: 1.263 / 1.164
All twelve faults are flagged on every case they apply to (smallest ratio 5.0, k_takes_v_bias); none of them passes the two
global bounds of tests/test_dinov3_gpu.py at T = 34 or T = 402 (the closest: window_drops_last_key at T = 402, 1.04 of the
first bound and 2.55 of the second), so HIDDEN is empty: what this module adds is the row and its class, and the outputs,
window forms and configs that no golden fixture has.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dinov3_block_check as B  # noqa: E402
from oracle import dinov3_oracle as O3  # noqa: E402

# planted faults that no bf16 output can show, with the derivation of why.  None: where a fault changes nothing a case computes
# (a transposed SQUARE grid; the angles of a view whose patch rows no window reaches) the faulty run is the clean run, and
# dinov3_block_check.fault_applies leaves that case out for that reason, not for a missed verdict
MISSES = {}
# the faults that the two global bounds of tests/test_dinov3_gpu.py let through on each case of BIG (measured below, then asserted)
HIDDEN = {"r4_2v_3x4_h1_d2": set(), "r4_2v_14x14_h1_d2": set()}


def setup_module():
    # rows of 128 .. 1024 numbers, 7 .. 138 of them: beyond a few threads the oracle only waits for its own pool (the module takes
    # twice as long on 16 threads as on 4; the tables come out the same to the last digit printed)
    torch.set_num_threads(min(4, os.cpu_count() or 1))


_RATIOS = {}


def ratios(case, mode):
    """(ok, {output: verdict}, message) of the Ops `mode` (a re-ordering or a fault) on a case, judged at the committed M;
    computed once."""
    key = (B.case_id(case), mode)
    if key not in _RATIOS:
        _RATIOS[key] = B.judge(case, B.run(case, B.ops(mode), B.reference(case)[0]), B.M, mode)
    return _RATIOS[key]


def test_the_drivers_restate_the_oracle():
    """dinov3_block_check.run feeds the oracle's layers itself (so a fault can sit in what they are fed): without a fault it gives
    the bits of oracle.dinov3_oracle.taps, which tests/test_oracle_golden.py pins to the reference."""
    for case in B.CASES:
        if case["kind"] == "layers" and B.has(case, "embed"):
            sd, cfg = B.state_dict(case["cfg"]), B.config(case["cfg"])
            inp, _, _, plain = B.reference(case)
            t = O3.taps(sd, cfg, inp["images"], B.windows(case), case["depth"])
            assert torch.equal(t["embed"], plain["embed"]) and torch.equal(t["patch_tokens"].flatten(0, 1), plain["forward"])


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


@pytest.mark.parametrize("cfg", list(B.CONFIGS))
def test_the_bf16_oracle_and_every_reordering_pass(cfg):
    for case in (c for c in B.CASES if c["cfg"] == cfg):
        inp, prec, rq, plain = B.reference(case)
        ok, _, msg = B.judge(case, rq, B.M, "round_qk bf16 oracle")
        assert ok, msg
        for vn in B.VARIANTS:
            ok, _, msg = ratios(case, vn)
            assert ok, msg


def test_what_round_qk_costs():
    """The round_qk oracle judged against the PLAIN bf16 oracle's b_r: what the engine's one deviation from the reference costs,
    as the two ratios (recorded, and the reason b_r is taken from the round_qk oracle)."""
    mx = md = 0.0
    for case in B.CASES:
        _, res, _ = B.judge(case, B.reference(case)[2], B.M, "round_qk", yardstick="plain")
        mx = max([mx] + [v["ratio_max"] for v in res.values()])
        md = max([md] + [v["ratio_med"] for v in res.values()])
    print(f"\n[round_qk] against the plain oracle's b_r: max e / max b {mx:.3f}, median e / median b {md:.3f}")
    assert abs(mx - B.ROUND_QK_COST[0]) < 0.02 and abs(md - B.ROUND_QK_COST[1]) < 0.02, (mx, md)


def rows_of(res, *outputs):
    return {name: {r: c for r, c, _ in res[name]["offenders"]} for name in outputs if name in res}


def offenders_as_expected(fault, case, res):
    """The rows `verdict` names, against what the fault is about.  Returns a complaint or None."""
    g = B.geom(case)
    named = rows_of(res, *B.OUTPUTS)
    everywhere = {r: c for rows in named.values() for r, c in rows.items()}
    if fault in ("window_drops_last_key", "k_takes_v_bias"):
        # a row outside every window has no keys and a zero attention output either way, and never mixes with another row
        bad = [(n, r) for n in ("stream", "final_ln") for r, c in named[n].items() if "uncovered" in c]
        return f"uncovered rows named: {bad}" if bad else None
    if fault == "uncovered_rows_stale":
        bad = [(n, r, c) for n, rows in named.items() for r, c in rows.items() if "uncovered" not in c]
        return f"rows other than the uncovered ones named: {bad}" if bad or not everywhere else None
    if fault == "h1_fixed":
        return None if any("uncovered" in c for c in named["stream"].values()) else "no uncovered row named in the stream"
    if fault in ("prefix_rows_rotated", "rope_prefix_off_by_R"):
        want = ("cls", "registers") if fault == "prefix_rows_rotated" else ("registers",)
        return None if any(c.split("+")[0] in want for c in named["stream"].values()) else f"no {want} row named in the stream"
    if fault == "rope_not_per_view" and case["window"] == "clean":
        bad = [(n, r) for n in ("stream", "final_ln") for r in named[n] if r < g["S"]]
        return f"rows of view 0 named under per-view windows: {bad}" if bad else None
    if fault == "registers_after_patches" and "embed" in res:
        regs = set(B.row_classes(case, "embed")["registers"])
        return None if regs <= set(named["embed"]) else "not every register row of the embedding named"
    if fault == "output_slice_off_by_one":
        return None if res["stream"]["ok"] and res["final_ln"]["ok"] and not res["forward"]["ok"] else "not the forward output alone"
    return None


def global_rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_every_planted_fault_on_every_case_it_applies_to():
    missed, hidden = {}, {B.case_id(c): set() for c in B.BIG}
    for fault in B.FAULTS:
        cases = [c for c in B.CASES if B.fault_applies(fault, c)]
        assert cases and B.fault_applies(fault, B.BIG[0]), fault
        flags, worst = [], []
        for case in cases:
            ok, res, _ = ratios(case, fault)
            flags.append(not ok)
            worst.append(max(max(v["ratio_max"], v["ratio_med"]) for v in res.values()))
            if not ok:
                complaint = offenders_as_expected(fault, case, res)
                assert complaint is None, (fault, B.case_id(case), complaint)
        col_b = []
        for big in B.BIG:
            if not B.fault_applies(fault, big):
                col_b.append(f"{B.case_id(big)}: does not apply")
                continue
            inp, prec, _, clean = B.reference(big)
            bad = B.run(big, B.ops(fault), inp)["forward"]
            e_clean = global_rel(clean["forward"], prec["forward"])
            f1, f2 = global_rel(bad, clean["forward"]) / 2e-2, global_rel(bad, prec["forward"]) / (1.5 * e_clean)
            if f1 <= 1 and f2 <= 1:
                hidden[B.case_id(big)].add(fault)
            col_b.append(f"{B.case_id(big)}: rel-L2 vs the clean bf16 run / 2e-2 = {f1:.2f}, error vs precise / (1.5 x clean) = {f2:.2f} -> "
                         f"{'HIDDEN from' if f1 <= 1 and f2 <= 1 else 'seen by'} today's bound")
        flagged = all(flags)
        if not flagged:
            missed[fault] = max(w for w, f in zip(worst, flags) if not f)
        print(f"\n[fault] {fault}: {len(cases)} cases, verdict fails on {sum(flags)}; largest ratio per case {min(worst):.2f} .. {max(worst):.2f} "
              f"(M = {B.M}) -> {'FLAGGED' if flagged else 'MISSED'}; " + "; ".join(col_b), end="")
    print()
    assert not set(B.ROW_LOCAL) & set(missed), missed
    assert set(missed) == set(MISSES), missed
    assert hidden == HIDDEN, hidden


def test_verdict_names_a_moved_register_row():
    case = next(c for c in B.CASES if B.case_id(c) == "r4_2v_2x3_clean_d1")
    inp, prec, rq, _ = B.reference(case)
    got = {k: v.clone() for k, v in rq.items()}
    got["embed"][12, 0] = torch.nextafter(got["embed"][12, 0], torch.tensor(float("inf")))      # view 1's first register, one ulp
    ok, res, msg = B.judge(case, got, B.M, "one register one ulp off")
    assert not ok and [r for r, _, _ in res["embed"]["offenders"]] == [12] and "registers (not the parameter's bits)" in msg
