"""GPU: the bf16 GEMVs and attentions of the decode step on every launch plan, against fp64.

csrc/decode_layer.hip (g2v_gemv_pg, g2v_decode_attn_pg), csrc/decode_batch.hip (g2v_gemv_pg_batch) and csrc/decode.hip (the
first generation: g2v_gemv_bf16, g2v_gemv_rmsnorm_bf16, g2v_gemv_rmsnorm_swiglu_bf16, g2v_gemv_swiglu_bf16, g2v_swiglu_bf16,
g2v_decode_attn, _dyn, _batch, _fused).  Operands, the launch table and the checks are tests/decode_check.py's;
tests/test_decode_check_cpu.py shows that the table reaches every batch depth, block size, scenes-per-pass count and long-K
pass count, and that the checks flag planted errors where they are planted.

GEMVs: every row of decode_check.TABLE, element by element with gemm_check.check_gemm on the activation read back through the
entry point under test (zero flags; TAU = 2^-16, 2 ulps for SwiGLU), outputs pre-filled with NaN sentinels, residuals random
fp32, two sentinel rows behind every target, the route of every launch asserted.  The batch-1 entries run 8 different
activation vectors, one launch each.

Attention: g2v_decode_attn_pg in its production form (max_len < scene_rows, lengths on the device, every cache row at and past
the new one NaN before the step) against qknorm_mrope_cache for the appended rows (bit for bit) and against fp64 softmax
attention (rel < 4e-3, worst element < 2^-6 of the row's rms: the bounds of tests/test_kv8_gpu.py on the same kernel body); the
first-generation attentions at the same lengths, G = 6 and 2, with the bound of tests/test_kernels_gpu.py and bit for bit
against each other.

Measured on an MI355X (the module prints the figures after its last test): zero flags in all 192 rows of the table; implied
accumulation error at most 1.1e-8 T (TAU 1.5e-5) in every entry (gemv_pg 8.6e-9, gemv_pg_batch 1.1e-8, first generation 9.3e-9);
SwiGLU at most 0.50 ulp in gemv_pg, gemv_pg_batch, gemv_rmsnorm_swiglu_bf16 and swiglu_bf16; the read-back norms at most 0.024
of their bound (first generation 0.024, gemv_pg_batch 0.020, gemv_pg 0: every value inside its rounding interval) with at most
0.39 % multi-valued elements (MULTI_CAP 2 %); 18 - 58 % of the GEMV outputs have more than one admissible value.
g2v_decode_attn_pg: rel at most 2.2e-3, worst element 1.2e-2 of the rms.  First generation: rel at most 1.1e-4 against the
bf16-rounded fp64 attention, worst element 1.1e-2 of the rms; no launch of any kernel here was flagged, so csrc/ is unchanged.

Structured score profiles (tests/attn_profile_check.py: families, plan mirror, the hard and the sharp bound with their
derivation; tests/test_attn_profile_cpu.py: the bounds proven on an emulation of the core, the planted errors).  The cached
rows are built from the q of the step, so that a head's scores follow a sawtooth per wave, rise or fall over the cache, hold one
peak key, spread over +-120 log2 units, sit at +-250 or are all equal; g2v_decode_attn_pg at B = 32 / max_len 2176 (three
batches per wave), B = 1 / 4160 (128 partials of one batch) and G = 8 at B = 3 / 17000, g2v_decode_attn_batch at B = 8 / 4160.
Zero elements over either bound, the peak-200 cases bit-equal to the peak key's V row.  Measured maxima of |err| / hard bound
and |err| / sharp bound on an MI355X, the CPU emulation's beside them:
                 g2v_decode_attn_pg    emulation        g2v_decode_attn_batch (hard1 / sharp1)   its emulation
  saw            0.75 / 0.38           0.81 / 0.42      0.97 / 0.97                               0.98 / 0.98
  saw_even       0.75 / 0.38           0.81 / 0.45      -
  rise           0.75 / 0.40           0.81 / 0.39      -
  fall           0.75 / 0.41           0.81 / 0.38      -
  peak           0.51 / 0.28           0.47 / 0.25      0.000 / 0.000                             0.001 / 0.001
  wide           0.67 / 0.38           0.68 / 0.32      0.94 / 0.93                               0.96 / 0.95
  offset         0.53 / 0.41           0.57 / 0.38      -
  flat           0.75 / -              0.81 / -         -
(0.75 / 0.81: the two-key slots, the same rows in every family.  The first generation keeps its weights in fp32: its bounds are
the output's bf16 rounding plus an fp32 term, and a half-ulp rounding reaches them.)  No kernel was flagged: csrc/ is unchanged.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_profile_check as P  # noqa: E402
import decode_check as D  # noqa: E402
import gemm_check as G  # noqa: E402
import rowop_check as R  # noqa: E402

pytestmark = pytest.mark.gpu
LENS = [1, 2, 32, 33, 65, 357, 4103]                         # cache lengths INCLUDING the new token, mixed over the slots
SLOTS = [(1, i) for i in range(7)] + [(3, 0), (3, 3), (3, 6), (8, 0)]
MEASURED = {}
WORST = {}
PROFILE = P.Ratios()


def worst(name, **kw):
    w = WORST.setdefault(name, {})
    for k, v in kw.items():
        w[k] = max(w.get(k, 0.0), v)


@pytest.fixture(scope="module", autouse=True)
def measured():
    yield
    for k, v in sorted(MEASURED.items()):
        print(f"[bf16 decode] {k}: n {v['n']} multi {v['multi'] / max(v['n'], 1):.2%} implied error {v['max_d']:.2e} T "
              f"swiglu {v['max_ulps']:.2f} ulp")
    for k, v in sorted(WORST.items()):
        print(f"[bf16 decode] {k}: " + " ".join(f"{a} {b:.3e}" for a, b in sorted(v.items())))
    PROFILE.report("bf16 decode profiles")
    D._EYE.clear()


@pytest.fixture(scope="module")
def hip():
    from g2vlm_amd import hip as h
    h.lib()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return h


def bits(t):
    return R.bits(t)


# ------------------------------------------------------------------------------------------------ GEMVs
def operand(hip, c, entry):
    """The activation the kernel multiplies, itself checked: a fused norm against the fp64 RMSNorm, the fused SwiGLU input bit
    for bit against swiglu_bf16, which is checked against the fp64 function."""
    A = c.activation(hip, entry)
    torch.cuda.synchronize()
    if c.norm:
        r = D.check_norm(A, c.x, c.nw)
        worst("norm " + entry, ratio=r.max_ratio, multi_share=r.multi_share)
        assert r.count == 0, r.report(what=f"norm read back through {entry}")
        assert r.multi_share <= R.MULTI_CAP, r.multi_share
    if c.form == "sw":
        sw = D.nan_bf16(c.B, c.K)
        for b in range(c.B):
            hip.swiglu_bf16(c.x[b], sw[b])
        torch.cuda.synchronize()
        assert torch.equal(bits(A), bits(sw))
        chk = D.check_swiglu(sw, c.x)
        worst("swiglu_bf16", ulps=chk.max_ulps)
        assert chk.count == 0, chk.report(what="swiglu_bf16")
    return A


@pytest.mark.parametrize("row", D.TABLE, ids=D.case_id)
def test_every_launch_plan_against_fp64(hip, row):
    entry, form, B, N, K = row
    if entry != "g1":
        assert hip.gemv_pg_route(*D.route_args(row)) == D.ROUTES[row], row
    c = D.Case(form, B, N, K, seed=D.case_seed(row), quant=False)
    A = operand(hip, c, entry)
    got = c.run(hip, entry)
    chk = c.check(hip, got, entry, A=A)
    D.record(f"{entry} {form}", chk, store=MEASURED)
    assert chk.count == 0, chk.report(what=D.case_id(row))
    assert c.guard_clean(), "a row behind the B outputs was stored"


REAL4 = D.PRODUCTION[:4]


@pytest.mark.parametrize("entry", ["pg", "pgb", "g1"])
def test_repeated_launches_are_bit_identical(hip, entry):
    for form, N, K in REAL4 + [("bias", 6401, 256), ("gu", 8224, 256)]:
        c = D.Case(form, 8 if entry != "pgb" else 5, N, K, seed=400, quant=False)
        first = c.run(hip, entry).clone()
        for _ in range(2):
            assert torch.equal(bits(c.run(hip, entry)), bits(first)), (entry, form)


@pytest.mark.parametrize("B", [2, 3, 5, 8])
def test_a_row_of_the_batched_kernel_does_not_depend_on_its_neighbours(hip, B):
    """NB = 2, 4, 8 and 8: scene 0's outputs keep their bits when the other scenes' activations change, theirs do not."""
    for form, N, K in REAL4 + [("bias", 8193, 256), ("gu", 16416, 256), ("o", 2000, 12288)]:
        c = D.Case(form, B, N, K, seed=500 + B, quant=False)
        a = c.run(hip, "pgb").clone()
        c.x = c.x.clone()
        c.x[1:] = D.dev(D.rnd(B - 1, c.x.shape[1], seed=777)).to(c.x.dtype)
        b = c.run(hip, "pgb")
        assert torch.equal(bits(a[0]), bits(b[0])), form
        for z in range(1, B):
            assert not torch.equal(bits(a[z]), bits(b[z])), (form, z)


@pytest.mark.parametrize("entry,B,N", [("pg", 8, 6401), ("pgb", 2, 12289), ("pgb", 3, 8193), ("pgb", 8, 4097)])
def test_one_weight_element_of_the_last_ragged_batch_moves_exactly_its_output(hip, entry, B, N):
    """Depth 5 (5 + 4), NB = 2 depth 5 (5 + 2), NB = 4 depth 3 (3 + 2), NB = 8 depth 2 (2 + 1): the last row of wave 0's last
    batch gets one weight negated; that output changes in every activation row, every other bit of the output stays."""
    K = 256
    form, threads, rb, kch = hip.gemv_pg_route(B if entry == "pgb" else 0, N, K, False, False, False)
    uq, ur = divmod(N, 256 * threads // 64)
    assert ur >= 1 and (uq + 1) > rb and (uq + 1) % rb                   # wave 0 has uq + 1 rows: two or more trips, the last ragged
    n = uq                                                                 # its last row
    c = D.Case("bias", B, N, K, seed=700 + B, quant=False)
    a = c.run(hip, entry).clone()
    k = int((c.x.float().abs().min(0).values * c.wd[n].float().abs()).argmax())
    c.wd[n, k] = -c.wd[n, k]
    b = c.run(hip, entry)
    changed = bits(a) != bits(b)
    assert changed[:, n].all() and int(changed.sum()) == B, (changed.nonzero().tolist()[:10], n)
    chk = c.check(hip, b, entry)
    assert chk.count == 0, chk.report(what="after the flip")


# ------------------------------------------------------------------------------------------------ attention
def slot_lengths(B, shift):
    return [LENS[(z + shift) % len(LENS)] for z in range(B)]


def make_step(hip, lens, Hq, Hkv, seed, max_len=None, pad=192, edit=None):
    """One decode step over B = len(lens) slots in the engine's form: caches [B, scene_rows, Hkv, 128] with scene_rows = max_len
    + pad, Gaussian bf16 rows [0, n - 1) per slot, NaN in the new row n - 1 and in every row behind it.  edit: applied to the raw
    qkv rows (on the host, in place) before anything is derived from them."""
    B = len(lens)
    if max_len is None:
        max_len = (max(lens) + 40 + 63) // 64 * 64
    assert max(lens) <= max_len
    rows = max_len + pad
    g = torch.Generator(); g.manual_seed(seed)
    qkv = torch.randn((B, (Hq + 2 * Hkv) * 128), generator=g).bfloat16()
    if edit is not None:
        edit(qkv)
    qkv = qkv.cuda()
    qw = (1 + 0.1 * torch.randn(128, generator=g)).cuda()
    kw = (1 + 0.1 * torch.randn(128, generator=g)).cuda()
    pos = torch.tensor([[n - 1 for n in lens]] * 3, dtype=torch.int32, device="cuda")
    inv_freq = (1.0 / (1e6 ** (torch.arange(0, 128, 2).float() / 128))).cuda()
    cos, sin = hip.mrope_table(pos, inv_freq)
    kc = torch.full((B, rows, Hkv, 128), float("nan"), dtype=torch.bfloat16)
    vc = torch.full((B, rows, Hkv, 128), float("nan"), dtype=torch.bfloat16)
    for z, n in enumerate(lens):
        if n > 1:
            kc[z, :n - 1] = torch.randn((n - 1, Hkv, 128), generator=g).bfloat16()
            vc[z, :n - 1] = torch.randn((n - 1, Hkv, 128), generator=g).bfloat16()
    s = dict(qkv=qkv, qw=qw, kw=kw, cos=cos, sin=sin, kc=kc.cuda(), vc=vc.cuda(), lens=lens, max_len=max_len, rows=rows,
             ld=torch.tensor(lens, dtype=torch.int32, device="cuda"))
    # what the separate kernel appends and the q it leaves: the reference for the appended rows and the attention's operands
    s["k_ref"], s["v_ref"] = s["kc"].clone(), s["vc"].clone()
    s["qn"] = torch.empty((B, Hq * 128), dtype=torch.bfloat16, device="cuda")
    at = torch.tensor([z * rows + n - 1 for z, n in enumerate(lens)], dtype=torch.int32, device="cuda")
    hip.qknorm_mrope_cache(qkv, Hq, Hkv, qw, qw, kw, kw, 0, 1e-6, 1, cos, sin, s["qn"], s["k_ref"], s["v_ref"], at)
    torch.cuda.synchronize()
    return s


def run_pg(hip, s, Hq, Hkv, out=None, ws=None):
    B = len(s["lens"])
    if out is None:
        out = D.nan_bf16(B, Hq * 128)
    if ws is None:
        ws = torch.empty(hip.decode_attn_pg_workspace(Hq, Hkv, B) // 4, dtype=torch.float32, device="cuda")
    hip.decode_attn_pg(s["qkv"], s["qw"], s["kw"], 1e-6, 1, s["cos"], s["sin"], s["kc"], s["vc"], out, s["ld"], s["rows"], s["max_len"],
                       Hq, Hkv, 128 ** -0.5, ws)
    return out


def check_against_fp64(name, s, out, Hq, Hkv):
    """out [B, Hq 128] against fp64 attention of the normalised q over the reference cache rows [0, n)."""
    qn, k, v, out = s["qn"].cpu(), s["k_ref"].cpu(), s["v_ref"].cpu(), out.cpu()
    assert torch.isfinite(out.float()).all()
    for z, n in enumerate(s["lens"]):
        want = D.attention64(qn[z].view(Hq, 128), k[z, :n], v[z, :n], Hkv)
        r, e = D.row_metrics(out[z].view(Hq, 128), want)
        worst(name, rel=r, elem=e)
        print(f"[{name}] B {len(s['lens'])} Hq {Hq} slot {z} len {n}: rel {r:.3e} worst element {e:.3e} of rms")
        assert r < D.REL_BOUND, (z, n, r)
        assert e < D.ELEM_BOUND, (z, n, e)


def check_step(hip, lens, Hq, Hkv, seed, max_len=None):
    s = make_step(hip, lens, Hq, Hkv, seed, max_len)
    Hv = Hq + Hkv
    for z, n in enumerate(lens):                                 # the step starts from NaN at and behind the new row
        assert torch.isnan(s["kc"][z, n - 1:].float()).all() and torch.isnan(s["vc"][z, n - 1:].float()).all()
    out = run_pg(hip, s, Hq, Hkv)
    torch.cuda.synchronize()
    # every cache bit: the appended K row is qknorm_mrope_cache's, V is the step's row, rows below unchanged, rows behind
    # (to the bucket's end and the scene_rows - max_len rows past it) still NaN
    assert torch.equal(bits(s["kc"]), bits(s["k_ref"])) and torch.equal(bits(s["vc"]), bits(s["v_ref"]))
    for z, n in enumerate(lens):
        assert torch.equal(bits(s["vc"][z, n - 1]).flatten(), bits(s["qkv"][z, Hv * 128:])), z
        assert torch.isfinite(s["kc"][z, :n].float()).all() and torch.isnan(s["kc"][z, n:].float()).all(), z
        assert torch.isnan(s["vc"][z, n:].float()).all(), z
    check_against_fp64("attn_pg", s, out, Hq, Hkv)
    return s, out


@pytest.mark.parametrize("Hq", [12, 4])                     # G = 6 (the model's), G = 2
@pytest.mark.parametrize("B,shift", SLOTS)
def test_attn_pg_in_the_engine_s_form_appends_and_matches_fp64(hip, Hq, B, shift):
    """Every length at B = 1, 3, 8 (nbh = 128, 85, 32), max_len = the 64-row bucket above the longest slot, scene_rows = max_len + 192."""
    check_step(hip, slot_lengths(B, shift), Hq, 2, seed=100 * B + 10 * shift + Hq)


GROUPS = [(2, 2, 0), (3, 1, 3), (8, 2, 6), (8, 1, 1)]         # (Hq, Hkv, shift): G = 1, 3, 4, 8 - one, one, two and three passes of
#                                                              four rows over the G + 1 rows to normalise, and GMAX


@pytest.mark.parametrize("Hq,Hkv,shift", GROUPS)
def test_attn_pg_at_the_edges_of_the_group_size(hip, Hq, Hkv, shift):
    """G = 1, 3, 4, 8 at B = 3 (G = 6 and 2 above): the same assertions and bounds, which are on the error against fp64 and do not
    depend on G."""
    check_step(hip, slot_lengths(3, shift), Hq, Hkv, seed=300 + 10 * shift + Hq + Hkv)


@pytest.mark.parametrize("Hq", [12, 4])
def test_attn_pg_with_a_full_slot_and_with_idle_waves(hip, Hq):
    """Lk == max_len (the new row is the bucket's last); max_len = 130 at B = 1: S = 2 keys per block, SW = 1 per wave, so waves
    2 and 3 of every block own nothing and blocks 65 - 127 have no key at all."""
    check_step(hip, [4160, 2, 357], Hq, 2, seed=31 + Hq, max_len=4160)
    check_step(hip, [357, 357], Hq, 2, seed=32 + Hq, max_len=357)
    for n in (1, 2, 129, 130):
        check_step(hip, [n], Hq, 2, seed=33 + n + Hq, max_len=130)


@pytest.mark.parametrize("Hq", [12, 4])
def test_attn_pg_with_eight_long_blocks_per_head_streams_five_batches(hip, Hq):
    """B = 32 at max_len = 4224: nbh = 8, 528 keys per block, 132 per wave: four full 32-key batches, a 4-key one, the rescale path."""
    lens = [4224, 4103, 1, 2, 33, 4224, 357, 65] + [LENS[z % 7] for z in range(24)]
    check_step(hip, lens, Hq, 2, seed=41 + Hq, max_len=4224)


def test_attn_pg_replays_from_a_graph_bit_identically(hip):
    """Three steps (attention, then the lengths advanced on the device) captured once and replayed equal the same three steps
    run eagerly, bit for bit: outputs and caches.  One stream, no parallel branches."""
    Hq, Hkv, lens = 12, 2, slot_lengths(6, 2)
    B = len(lens)
    base = make_step(hip, lens, Hq, Hkv, seed=99)
    runs = []
    for graph in (False, True):
        s = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in base.items()}
        out = torch.empty((B, Hq * 128), dtype=torch.bfloat16, device="cuda")
        ws = torch.empty(hip.decode_attn_pg_workspace(Hq, Hkv, B) // 4, dtype=torch.float32, device="cuda")
        outs = []

        def step():
            run_pg(hip, s, Hq, Hkv, out, ws)
            s["ld"].add_(1)
        if graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()                                        # warm-up outside the capture, then undone
            torch.cuda.current_stream().wait_stream(side)
            for n in ("ld", "kc", "vc"):
                s[n].copy_(base[n])
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            for _ in range(3):
                g.replay()
                outs.append(out.clone())
        else:
            for _ in range(3):
                step()
                outs.append(out.clone())
        torch.cuda.synchronize()
        runs.append((outs, [s[n].clone() for n in ("kc", "vc")], s["ld"].clone()))
    (oe, ce, le), (og, cg, lg) = runs
    assert all(torch.equal(a, b) for a, b in zip(oe, og)) and all(torch.isfinite(a.float()).all() for a in oe)
    assert torch.equal(le, lg) and le.tolist() == [n + 3 for n in lens]
    for a, b in zip(ce, cg):
        assert torch.equal(bits(a), bits(b))
    for z, n in enumerate(lens):                             # the three new rows of every slot are written, NaN behind
        for c in ce:
            assert torch.isfinite(c[z, :n + 2].float()).all() and torch.isnan(c[z, n + 2:].float()).all(), z


def assert_bf16_close(got, ref, rl=4e-3, ulps=2.0):
    """tests/test_kernels_gpu.py's comparison, as the first-generation attention tests apply it (ulps = 1.01)."""
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape
    assert torch.isfinite(got).all()
    r = float((got - ref).double().norm() / (ref.double().norm() + 1e-30))
    assert r < rl, f"rel-L2 {r}"
    tol = ulps * 2.0 ** -8 * ref.abs().clamp_min(ref.abs().max() * 2 ** -7)
    bad = ((got - ref).abs() > tol)
    assert bad.float().mean() < 2e-3, f"{int(bad.sum())} of {bad.numel()} elements off by > {ulps} bf16 ulp"
    return r


@pytest.mark.parametrize("Hq", [12, 4])
@pytest.mark.parametrize("B,shift", SLOTS)
def test_first_generation_attentions_against_fp64_and_each_other(hip, Hq, B, shift):
    """g2v_decode_attn (length by value), _dyn (length on the device, grid by max_len), _batch and _fused on one step: each
    slot of every form against fp64 attention with assert_bf16_close(ulps = 1.01); dyn == static, batch[z] == static and fused
    == qknorm_mrope_cache + batch bit for bit, the fused append included."""
    Hkv, sc = 2, 128 ** -0.5
    lens = slot_lengths(B, shift)
    s = make_step(hip, lens, Hq, Hkv, seed=200 * B + 10 * shift + Hq)
    max_len, rows = s["max_len"], s["rows"]
    qn, k, v = s["qn"], s["k_ref"], s["v_ref"]
    ws = torch.empty(B * hip.decode_attn_workspace(max_len, Hq) // 4, dtype=torch.float32, device="cuda")
    o_batch = D.nan_bf16(B, Hq * 128)
    hip.decode_attn_batch(qn, k, v, o_batch, s["ld"], rows, max_len, Hq, Hkv, sc, ws)
    o_fused = D.nan_bf16(B, Hq * 128)
    hip.decode_attn_fused(s["qkv"], s["qw"], s["kw"], 1e-6, 1, s["cos"], s["sin"], s["kc"], s["vc"], o_fused, s["ld"], rows, max_len,
                          Hq, Hkv, sc, ws)
    torch.cuda.synchronize()
    assert torch.equal(bits(o_fused), bits(o_batch))
    assert torch.equal(bits(s["kc"]), bits(k)) and torch.equal(bits(s["vc"]), bits(v))
    kc, vc, qc = k.cpu(), v.cpu(), qn.cpu()
    for z, n in enumerate(lens):
        o_static, o_dyn = D.nan_bf16(Hq, 128), D.nan_bf16(Hq, 128)
        ws1 = torch.empty(hip.decode_attn_workspace(n, Hq) // 4, dtype=torch.float32, device="cuda")
        hip.decode_attn(qn[z].view(Hq, 128), k[z], v[z], o_static, n, Hq, Hkv, sc, ws1)
        hip.decode_attn_dyn(qn[z].view(Hq, 128), k[z], v[z], o_dyn, s["ld"][z:z + 1], max_len, Hq, Hkv, sc, ws)
        torch.cuda.synchronize()
        assert torch.equal(bits(o_dyn), bits(o_static)), (z, n)
        assert torch.equal(bits(o_batch[z].view(Hq, 128)), bits(o_static)), (z, n)
        want = D.attention64(qc[z].view(Hq, 128), kc[z, :n], vc[z, :n], Hkv)
        r = assert_bf16_close(o_static, want.bfloat16(), ulps=1.01)
        _, e = D.row_metrics(o_static, want)
        worst("attn gen1", rel=r, elem=e)


# ------------------------------------------------------------------------------------------------ structured score profiles
def profile_step(hip, case, variant, lens, Hq, Hkv, seed, max_len, waves, kb=P.KB):
    """make_step with the cached rows of every slot replaced by the builder's (tests/attn_profile_check.py), built from the q
    that qknorm_mrope_cache leaves for the step's qkv; the rows at and behind the new one stay NaN."""
    new = P.new_row_slots(case, lens, variant)
    s = make_step(hip, lens, Hq, Hkv, seed, max_len, edit=lambda qkv: P.align_new_k(qkv, Hq, Hkv, new))
    knew = torch.stack([s["k_ref"][z, n - 1] for z, n in enumerate(lens)]).cpu()
    Ks, Vs, s["infos"] = P.build_step(case, s["qn"].cpu(), knew, lens, Hq, Hkv, waves, seed + 1, variant, kb=kb)
    for z, n in enumerate(lens):
        if n > 1:
            for name, rows in (("kc", Ks[z]), ("k_ref", Ks[z]), ("vc", Vs[z]), ("v_ref", Vs[z])):
                s[name][z, :n - 1] = rows.cuda()
        assert torch.isnan(s["kc"][z, n - 1:].float()).all() and torch.isnan(s["vc"][z, n - 1:].float()).all()
    return s


def check_profile(name, case, s, out, Hq, Hkv, gen1=False):
    """Every slot of out [B, Hq 128] against fp64 attention over the reference cache rows [0, n) under the hard and the sharp
    bound, no element exempt; an exact case (peak 200) must equal the peak key's V row bit for bit."""
    G_ = Hq // Hkv
    qn, k, v, out = s["qn"].cpu(), s["k_ref"].cpu(), s["v_ref"].cpu(), out.cpu()
    over = 0
    for z, n in enumerate(s["lens"]):
        o = out[z].view(Hq, 128)
        over += P.check_slot(PROFILE, name, case[0], o, qn[z].view(Hq, 128), k[z, :n], v[z, :n], Hkv, gen1=gen1)
        for h in range(Hkv):
            if s["infos"][z][h]["exact"]:
                assert torch.equal(bits(o[h * G_:(h + 1) * G_]), bits(v[z, s["infos"][z][h]["peak"], h].expand(G_, 128))), (z, h)
    w = PROFILE.worst[name]
    print(f"[{name}] |err| / hard {w['hard']:.3f}  |err| / sharp {w['sharp']:.3f}")
    assert over == 0, (name, over, w)


@pytest.mark.parametrize("shape,cv", [(sh, cv) for sh in ("b32", "b1", "g8") for cv in P.pg_cases(sh)],
                         ids=lambda v: v if isinstance(v, str) else P.pg_case_id(v))
def test_attn_pg_on_structured_score_profiles(hip, shape, cv):
    """g2v_decode_attn_pg on every family of tests/attn_profile_check.py at the shapes P.PG_SHAPES: the appended rows bit for
    bit, the rows below untouched, NaN behind, and the output inside both bounds."""
    case, variant = cv
    Hq, Hkv, max_len, lens = P.PG_SHAPES[shape]
    waves = P.pg_waves(max_len, P.pg_nbh(Hkv, len(lens)))
    s = profile_step(hip, case, variant, lens, Hq, Hkv, 50 + len(lens) + variant, max_len, waves)
    out = run_pg(hip, s, Hq, Hkv)
    torch.cuda.synchronize()
    assert torch.equal(bits(s["kc"]), bits(s["k_ref"])) and torch.equal(bits(s["vc"]), bits(s["v_ref"]))
    for z, n in enumerate(lens):
        assert torch.isfinite(s["kc"][z, :n].float()).all() and torch.isnan(s["kc"][z, n:].float()).all(), z
        assert torch.isnan(s["vc"][z, n:].float()).all(), z
    check_profile(f"attn_pg {shape} {P.case_id(case)}", case, s, out, Hq, Hkv)


@pytest.mark.parametrize("case", P.GEN1_CASES, ids=P.case_id)
def test_first_generation_attention_on_structured_score_profiles(hip, case):
    """g2v_decode_attn_batch (the other first-generation entries are bit-equal to it by the test above) on the sawtooth, the
    peak and the wide family at B = 8, max_len = 4160, under the first generation's own two bounds (fp32 weights)."""
    Hq, Hkv, max_len, lens = P.GEN1_SHAPE
    s = profile_step(hip, case, 0, lens, Hq, Hkv, 70, max_len, P.gen1_waves(max_len), kb=16)
    ws = torch.empty(len(lens) * hip.decode_attn_workspace(max_len, Hq) // 4, dtype=torch.float32, device="cuda")
    out = D.nan_bf16(len(lens), Hq * 128)
    hip.decode_attn_batch(s["qn"], s["k_ref"], s["v_ref"], out, s["ld"], s["rows"], max_len, Hq, Hkv, 128 ** -0.5, ws)
    torch.cuda.synchronize()
    check_profile(f"attn gen1 {P.case_id(case)}", case, s, out, Hq, Hkv, gen1=True)
