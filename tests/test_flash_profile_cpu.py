"""CPU: the score profiles, the derived bounds and the planted errors of tests/flash_profile_check.py (prefill attention).

flash_fwd_kernel, flash_fwd64_kernel and flash_combine_kernel (csrc/attn.hip) are emulated in torch (flash_profile_check.emulate).
Shown here, without a GPU:
  * every family, under both emulated forms, in one segment and cut into 3 and 7 segments, keeps the emulation inside the hard
    bound (flat: the exact-weights bound) on every element, the noisy families inside the sharp bound too, and every peak-200 row
    bit-equal to its key's V row; at D = 128 (both forms) and, generic form, at D = 16 and 80;
  * the fp64 reference agrees with the oracle's varlen_attention(precise=True) on a small case of every family;
  * the peaks visit every slot of a full tile, every slot of the partial tile, key 0, key k_len - 1 and a causal row's last key;
  * each planted error is over a bound in the family built for it (FAMILY_OF), and which of them the Gaussian control lets
    through under the row bounds BOUND[D] of tests/test_attention_gpu.py (GAUSS_MISSES: observed, then asserted);
  * make_attn_plan refuses a causal window with k_len < q_len.

Planted errors at D = 128, 4:2 heads (|err| / hard and |err| / sharp in the family; the Gaussian control under BOUND[128]):
  planted error                                             family (form, segments)        / hard   / sharp   Gaussian control (e_max, e_row in units of the bound)
  skip_rescale      no rescale in one 32-row block          rise 20 (generic, 1)           100      128       flagged: 67 x, 123 x
  l_only            l rescaled, O not                       rise 3 (generic, 1)            653      1060      flagged: 179 x, 338 x
  swap_weights      two weights swapped in a 16-key group   peak 30, variant 1 (generic)   1.4e5    5.0e4     flagged: 60 x, 145 x
  v_neighbour       V row from the next key slot            flat (generic, 1)              31       -         flagged: 58 x, 121 x
  drop_last_key     key k_len - 1 masked                    ramp (generic, 1)              229      130       flagged: 19 x, 36 x
  past_diagonal     one key past the diagonal admitted      ramp causal 200 x 256          1370     1030      flagged: 50 x, 112 x
  stale_p           one d-block of 16 keys: previous P      wide 120 (generic, 1)          608      465       flagged: 125 x, 125 x
  ref_never_raised  fwd64 reference never raised            rise 70 (fwd64, 1)             inf      inf       MISSED: 0.48 x, 0.64 x
  raw_m             one slot's m in raw units               offset 250 (generic, 3)        80       324       flagged: 660 x, 1310 x
  drop_slot         last slot of the merge dropped          rise 20 (generic, 3)           9.5e4    4.9e4     flagged: 114 x, 180 x
Every planted error is caught by a structured family.  The Gaussian control (77 x 420 and causal 300 x 357, q and k of unit variance)
under BOUND[128] catches nine of the ten as well: the errors are planted on every head of a whole 32-row block or tile, and a row
that averages a few hundred V rows moves by many times 3e-2 of its RMS when one weight in 64 goes astray.  It cannot see the
reference that is never raised - right in exact arithmetic, wrong only where 2^(s c - m_ref) overflows - nor does it reach the
code the families run: alpha and merge weights that underflow, segments whose references differ by hundreds of units, a single key
or tile with all the weight, equal weights, offsets of +-250, and the rows that must equal a V row bit for bit.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flash_profile_check as F  # noqa: E402

RATIOS = F.Ratios()
CPU_HEADS = {128: (4, 2), 16: (2, 2), 80: (2, 2)}
_BUILT = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    RATIOS.report("emulation")


def built(D, i):
    """(q, k, v, info, sums) of case i of head dim D: built once, shared, never changed."""
    if (D, i) not in _BUILT:
        cs = F.cases(D)[i]
        Hq, Hkv = CPU_HEADS[D]
        q, k, v, info = F.build(cs, Hq, Hkv, D, seed=1000 * D + i)
        _BUILT[(D, i)] = (q, k, v, info, F.reference(q, k, v, cs["causal"], D))
    return _BUILT[(D, i)]


def run_case(D, i, form, cuts, fault=None, ratios=RATIOS, name=None):
    cs = F.cases(D)[i]
    q, k, v, info, sums = built(D, i)
    got = F.emulate(q, k, v, cs["causal"], form, cuts, fault)
    over = F.check(ratios, name or f"{cs['family']} D={D} {form}", cs["family"], got, sums)
    if fault is None and info["exact"] is not None:
        sees, jr = info["exact"]
        rep = q.shape[1] // k.shape[1]
        assert torch.equal(got[sees], v[jr[sees]].repeat_interleave(rep, dim=1)), F.case_id(cs)
    return over, got, sums


@pytest.mark.parametrize("cuts", [1, 3, 7])
@pytest.mark.parametrize("D,form", [(128, "generic"), (128, "fwd64"), (16, "generic"), (80, "generic")])
def test_the_emulation_stays_inside_the_bounds(D, form, cuts):
    if D != 128 and cuts == 7:
        cuts = 2
    bad = []
    for i, cs in enumerate(F.cases(D)):
        over, _, _ = run_case(D, i, form, cuts)
        if over:
            bad.append((F.case_id(cs), over))
    assert not bad, bad


@pytest.mark.parametrize("family", F.FAMILIES)
def test_the_reference_matches_the_oracle(family):
    from oracle import g2vlm_oracle as O
    D, Hq, Hkv = 64, 4, 2
    if family == "peak":
        cs = [c for c in F.cases(D) if c["family"] == "peak" and c["Lq"] == 77][0]
    else:
        param = {"ramp": 1.0, "flat": 0.0, "rise": 20.0, "fall": 70.0, "offset": 250.0, "wide": 120.0, "gauss": 0.0}[family]
        cs = dict(family=family, param=param, alt=family == "rise", variant=0, Lq=70, Lk=100, causal=family in ("ramp", "fall", "flat"))
    q, k, v, _ = F.build(cs, Hq, Hkv, D, seed=3)
    want = F.reference(q, k, v, cs["causal"], D)[0]
    ora = O.varlen_attention(q.double(), k.double(), v.double(), [0, cs["Lq"]], [0, cs["Lk"]], cs["causal"], precise=True)
    assert bool(torch.isfinite(want).all())
    assert float((want - ora).abs().max()) < 1e-12


@pytest.mark.parametrize("D", F.SWEEP_DS)
def test_the_peaks_visit_every_key_slot(D):
    full, part, first, last, diag = F.peak_coverage(D)
    assert full == set(range(64)) and part == set(range(320, 357)) and first and last and diag
    fams = {c["family"] for c in F.cases(D)}
    assert fams == set(F.FAMILIES)
    for c in F.cases(D):
        assert c["Lq"] in (77, 200, 300) and (c["Lk"] <= 256 if c["family"] == "ramp" else c["Lk"] in (357, 420) or c["family"] == "flat")


# ------------------------------------------------------------------------------------------------ planted errors
def case_index(D, family, param, **kw):
    for i, c in enumerate(F.cases(D)):
        if c["family"] == family and c["param"] == param and all(c[k_] == v_ for k_, v_ in kw.items()):
            return i
    raise KeyError((family, param, kw))


# fault -> (family, parameter, case filter, form, segments): the family built to expose it
FAMILY_OF = {
    "skip_rescale": ("rise", 20.0, dict(alt=False), "generic", 1),          # the first tiles keep a weight 2^20 .. 2^120 too large
    "l_only": ("rise", 3.0, dict(alt=False), "generic", 1),                # every tile's rescale is missing from O
    "swap_weights": ("peak", 30.0, dict(variant=1), "generic", 1),         # keys 145 and 150 are both peaks: their rows get the other's V row
    "v_neighbour": ("flat", 0.0, dict(causal=False), "generic", 1),        # equal weights: the mean moves by (v_149 - v_148) / n
    "drop_last_key": ("ramp", 1.0, dict(causal=False), "generic", 1),      # every row selects key k_len - 1
    "past_diagonal": ("ramp", 1.0, dict(causal=True, Lq=200, Lk=256), "generic", 1),   # the admitted key would carry twice the weight
    "stale_p": ("wide", 120.0, dict(causal=False), "generic", 1),          # the previous tile's weights are unrelated
    "ref_never_raised": ("rise", 70.0, dict(alt=False), "fwd64", 1),       # 2^(s c - m_ref) overflows from the third tile on
    "raw_m": ("offset", 250.0, dict(causal=False), "generic", 3),          # m / c = +-1960: that slot takes all or none
    "drop_slot": ("rise", 20.0, dict(alt=False), "generic", 3),            # the last slot holds all the weight
}
# planted errors the Gaussian control does NOT flag under BOUND[D] (observed by the test below, then asserted)
GAUSS_MISSES = {"ref_never_raised"}


def gauss_flagged(D, got, want):
    if not bool(torch.isfinite(got.float()).all()):
        return True, float("inf"), float("inf")
    e_max, e_row = F.row_errors(got, want, D)
    bm, br = F.BOUND[D]
    return bool(((e_max > bm) | (e_row > br)).any()), float(e_max.max()) / bm, float(e_row.max()) / br


def test_planted_errors():
    """Each planted error is over a bound in its family; the Gaussian control flags exactly those not in GAUSS_MISSES."""
    D = 128
    missed, uncaught = set(), set()
    for fault in F.FAULTS:
        family, param, kw, form, cuts = FAMILY_OF[fault]
        i = case_index(D, family, param, **kw)
        clean, r = F.Ratios(), F.Ratios()
        assert run_case(D, i, form, cuts, ratios=clean, name="c")[0] == 0
        over, _, _ = run_case(D, i, form, cuts, fault=fault, ratios=r, name="f")
        flagged, wm, wr = False, 0.0, 0.0
        for gi in (j for j, c in enumerate(F.cases(D)) if c["family"] == "gauss"):
            _, got, sums = run_case(D, gi, form, cuts, fault=fault, ratios=F.Ratios(), name="g")
            _, g0, _ = run_case(D, gi, form, cuts, ratios=F.Ratios(), name="g")
            assert not gauss_flagged(D, g0, sums[0])[0]
            fl, m_, r_ = gauss_flagged(D, got, sums[0])
            flagged, wm, wr = flagged or fl, max(wm, m_), max(wr, r_)
        print(f"\n[planted] {fault}: {family} {param:g} ({form}, {cuts} segment(s)) |err| / hard {r.worst['f']['hard']:.3g}, / sharp "
              f"{r.worst['f']['sharp']:.3g}, {over} elements over; Gaussian control under BOUND[{D}]: "
              f"{'flags it' if flagged else 'MISSES it'} (e_max {wm:.2f} x, e_row {wr:.2f} x the bound)")
        if over == 0:
            uncaught.add(fault)
        if not flagged:
            missed.add(fault)
    assert not uncaught, uncaught
    assert missed == GAUSS_MISSES, missed


# ------------------------------------------------------------------------------------------------ the plan's refusal
def test_make_attn_plan_refuses_a_causal_window_with_keyless_rows():
    """Bottom-right causal with k_len < q_len leaves the first q_len - k_len rows without a key: their query tiles would be
    skipped (output never written) or end as 0 x (1 / 0).  No caller passes such a window; the plan refuses it."""
    from g2vlm_amd import hip
    with pytest.raises(ValueError, match="k_len"):
        hip.make_attn_plan([(0, 300, 0, 200, True)], 4, "cpu")
    with pytest.raises(ValueError, match="k_len"):
        hip.make_attn_plan([(0, 64, 0, 64, False), (64, 2, 64, 1, True)], 4, "cpu", tile_rows=256)
    plan = hip.make_attn_plan([(0, 200, 0, 200, True), (200, 300, 0, 100, False)], 4, "cpu")        # equal lengths and non-causal stay
    assert plan.n_tiles == 5
