"""GPU: the kernels of the FP8 (e4m3) KV cache (csrc/decode_kv8.hip).

g2v_kv_quant_e4m3 / g2v_kv_dequant_e4m3 against the host quantiser (g2vlm_amd/quant.py), and g2v_decode_attn_pg_kv8 - one
decode-attention step over an e4m3 cache that appends the new token's row quantised - against an fp64 softmax attention over the
dequantised cache, against what qknorm_mrope_cache appends in bf16, and against g2v_decode_attn_pg on the unquantised rows.

Structured score profiles (tests/attn_profile_check.py, proven on the CPU by tests/test_attn_profile_cpu.py): the families
through the host quantiser at B = 32 / 2176, B = 1 / 4160 and G = 8 at B = 3 / 17000; rise 20 and fall 20 put nine distinct K
scales into one slot (at least six asserted).  Zero elements over the hard or the sharp bound, the peak-200 cases bit-equal to
the peak key's dequantised V row.  Measured maxima of |err| / hard and |err| / sharp on an MI355X | the CPU emulation:
  saw 0.75 / 0.40 | 0.68 / 0.39     saw_even 0.75 / 0.39 | 0.68 / 0.41     rise 0.75 / 0.40 | 0.68 / 0.39     fall 0.75 / 0.44 | 0.68 / 0.40
  peak 0.46 / 0.23 | 0.47 / 0.26    wide 0.71 / 0.35 | 0.67 / 0.34         offset 0.48 / 0.36 | 0.48 / 0.34   flat 0.75 / - | 0.68 / -"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from g2vlm_amd.quant import dequantize_rows, quantize_rows_e4m3  # noqa: E402
from test_kv8_cpu import attention64, magnitude_rows  # noqa: E402
import attn_profile_check as P  # noqa: E402

LENS = [1, 2, 32, 33, 65, 357, 4103]                         # cache lengths INCLUDING the new token, mixed over the slots
POISON = 0x7F                                                # the e4m3fn NaN code
PROFILE = P.Ratios()


@pytest.fixture(scope="module", autouse=True)
def measured():
    yield
    PROFILE.report("kv8 profiles")


@pytest.fixture(scope="module")
def hip():
    from g2vlm_amd import hip as h
    h.lib()
    return h


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def host_quant(x):
    """x bf16 [..., Hkv, 128] (any device) -> (codes uint8 like x, scales f32 [..., Hkv]) on the CPU, by the host quantiser."""
    q, s = quantize_rows_e4m3(x.reshape(-1, 128))
    return q.view(x.shape), s.view(x.shape[:-1])


def host_dequant(q, s):
    return dequantize_rows(q.reshape(-1, 128).cpu(), s.reshape(-1).cpu()).view(q.shape)


# ------------------------------------------------------------------------------------------------ the quantiser kernels
def cache_rows(rows, Hkv):
    """[rows, Hkv, 128] bf16: Gaussian rows whose magnitude cycles from 2^-20 to 3e4 over (row, head), with the edge rows of
    tests/test_kv8_cpu.py (all zero, amax = 448 / 224 / 225 x 2^k) among them."""
    g = torch.Generator(); g.manual_seed(rows + Hkv)
    mags = torch.tensor([2.0 ** -20, 2.0 ** -13, 3e-3, 0.07, 1.0, 5.5, 448.0, 1000.0, 30080.0])
    x = torch.randn((rows, Hkv, 128), generator=g) * (mags[torch.arange(rows * Hkv) % len(mags)].view(rows, Hkv, 1) / 4)
    x = x.to(torch.bfloat16)
    edge = magnitude_rows(Hkv)
    if rows >= len(edge):
        x[:len(edge)] = edge
    elif rows > 1:
        x[:] = edge[[9, 10, 13, 16, 0, 8, 5]][:rows]            # zero, 448, 224 and 225 x 2^-9, 2^-20, 30080, 5.5
    else:
        x[0] = edge[13]
    return x


@pytest.mark.parametrize("Hkv", [2, 1])
@pytest.mark.parametrize("rows", [1, 7, 4103])
def test_quantiser_kernels_match_the_host(hip, rows, Hkv):
    x = cache_rows(rows, Hkv)
    qh, sh = host_quant(x)
    codes = torch.full((rows, Hkv, 128), POISON, dtype=torch.uint8, device="cuda")
    scales = torch.full((rows, Hkv), float("nan"), dtype=torch.float32, device="cuda")
    hip.kv_quant_e4m3(x.cuda(), codes, scales)
    torch.cuda.synchronize()
    assert torch.equal(scales.cpu().view(torch.int32), sh.view(torch.int32))            # bit-equal
    assert not ((codes & 0x7F) == 0x7F).any()
    want = host_dequant(qh, sh)
    assert torch.equal(host_dequant(codes, scales), want)                                 # equal values
    got = hip.kv_dequant_e4m3(codes, scales)
    torch.cuda.synchronize()
    assert got.dtype == torch.bfloat16 and torch.equal(got.cpu(), want)                   # dequant is exact


def test_dequant_is_exact_for_every_code(hip):
    """All 254 non-NaN codes under scales from 2^-29 to 2^7: code * scale, exactly."""
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)
    codes = torch.cat([codes, codes[:2]]).view(1, 2, 128).repeat(37, 1, 1).contiguous()
    scales = torch.pow(2.0, torch.arange(-29, 8).float()).view(37, 1).repeat(1, 2).contiguous()
    got = hip.kv_dequant_e4m3(codes.cuda(), scales.cuda())
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), host_dequant(codes, scales))


# ------------------------------------------------------------------------------------------------ the attention
def make_step(hip, lens, Hq, Hkv, seed, cap=None, edit=None):
    """One decode step over B = len(lens) slots.  The cache rows [0, n - 1) of slot z are Gaussian bf16 rows through the host
    quantiser; the new row n - 1 and everything past it are poisoned: NaN codes, NaN scales.  cap: the capacity (default: the
    64-row bucket above the longest slot); edit: applied to the raw qkv rows on the host, in place."""
    B = len(lens)
    if cap is None:
        cap = (max(lens) + 40 + 63) // 64 * 64
    assert max(lens) <= cap
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
    kc = torch.full((B, cap, Hkv, 128), POISON, dtype=torch.uint8)
    vc = torch.full((B, cap, Hkv, 128), POISON, dtype=torch.uint8)
    ks = torch.full((B, cap, Hkv), float("nan"), dtype=torch.float32)
    vs = torch.full((B, cap, Hkv), float("nan"), dtype=torch.float32)
    k16 = torch.zeros((B, cap, Hkv, 128), dtype=torch.bfloat16)      # the unquantised rows, for the bf16 kernel
    v16 = torch.zeros((B, cap, Hkv, 128), dtype=torch.bfloat16)
    for z, n in enumerate(lens):
        if n > 1:
            k16[z, :n - 1] = torch.randn((n - 1, Hkv, 128), generator=g).bfloat16()
            v16[z, :n - 1] = torch.randn((n - 1, Hkv, 128), generator=g).bfloat16()
            kc[z, :n - 1], ks[z, :n - 1] = host_quant(k16[z, :n - 1])
            vc[z, :n - 1], vs[z, :n - 1] = host_quant(v16[z, :n - 1])
    return dict(qkv=qkv, qw=qw, kw=kw, cos=cos, sin=sin, kc=kc.cuda(), vc=vc.cuda(), ks=ks.cuda(), vs=vs.cuda(), k16=k16, v16=v16,
                lens=lens, cap=cap, ld=torch.tensor(lens, dtype=torch.int32, device="cuda"))


def run_kv8(hip, s, Hq, Hkv, out=None, ws=None):
    B, cap = len(s["lens"]), s["cap"]
    if out is None:
        out = torch.full((B, Hq * 128), float("nan"), dtype=torch.bfloat16, device="cuda")
    if ws is None:
        ws = torch.empty(hip.decode_attn_pg_workspace(Hq, Hkv, B) // 4, dtype=torch.float32, device="cuda")
    hip.decode_attn_pg_kv8(s["qkv"], s["qw"], s["kw"], 1e-6, 1, s["cos"], s["sin"], s["kc"], s["vc"], s["ks"], s["vs"], out, s["ld"], cap, cap,
                           Hq, Hkv, 128 ** -0.5, ws)
    return out


def check_step(hip, lens, Hq, Hkv, seed):
    B = len(lens)
    s = make_step(hip, lens, Hq, Hkv, seed)
    cap = s["cap"]
    kc0, vc0, ks0, vs0 = (s[n].cpu() for n in ("kc", "vc", "ks", "vs"))
    out = run_kv8(hip, s, Hq, Hkv)
    torch.cuda.synchronize()
    kc1, vc1, ks1, vs1 = (s[n].cpu() for n in ("kc", "vc", "ks", "vs"))
    assert torch.isfinite(out.float()).all()

    # what the separate kernel appends in bf16 (and its q, for the reference below), and the bf16 kernel on the unquantised rows
    qn = torch.empty((B, Hq * 128), dtype=torch.bfloat16, device="cuda")
    k3, v3 = s["k16"].cuda(), s["v16"].cuda()
    rows = torch.tensor([z * cap + n - 1 for z, n in enumerate(lens)], dtype=torch.int32, device="cuda")
    hip.qknorm_mrope_cache(s["qkv"], Hq, Hkv, s["qw"], s["qw"], s["kw"], s["kw"], 0, 1e-6, 1, s["cos"], s["sin"], qn, k3, v3, rows)
    k2, v2 = s["k16"].cuda(), s["v16"].cuda()
    o_pg = torch.empty_like(out)
    ws2 = torch.empty(hip.decode_attn_pg_workspace(Hq, Hkv, B) // 4, dtype=torch.float32, device="cuda")
    hip.decode_attn_pg(s["qkv"], s["qw"], s["kw"], 1e-6, 1, s["cos"], s["sin"], k2, v2, o_pg, s["ld"], cap, cap, Hq, Hkv, 128 ** -0.5, ws2)
    torch.cuda.synchronize()
    k3, v3, qn, out_c, o_pg = k3.cpu(), v3.cpu(), qn.cpu(), out.cpu(), o_pg.cpu()

    worst = dict(fp64=0.0, elem=0.0, bf16=0.0)
    for z, n in enumerate(lens):
        # rows below the new one untouched, rows past it still poison
        assert torch.equal(kc1[z, :n - 1], kc0[z, :n - 1]) and torch.equal(vc1[z, :n - 1], vc0[z, :n - 1]), z
        assert torch.equal(ks1[z, :n - 1], ks0[z, :n - 1]) and torch.equal(vs1[z, :n - 1], vs0[z, :n - 1]), z
        assert (kc1[z, n:] == POISON).all() and (vc1[z, n:] == POISON).all(), z
        assert torch.isnan(ks1[z, n:]).all() and torch.isnan(vs1[z, n:]).all(), z
        # the appended row: the quantised bf16 row of qknorm_mrope_cache, scales bit-equal, values equal
        for got_c, got_s, row in ((kc1, ks1, k3[z, n - 1]), (vc1, vs1, v3[z, n - 1])):
            qh, sh = host_quant(row)
            assert torch.equal(got_s[z, n - 1].view(torch.int32), sh.view(torch.int32)), z
            assert torch.equal(host_dequant(got_c[z, n - 1], got_s[z, n - 1]), host_dequant(qh, sh)), z
        # fp64 softmax attention over the dequantised cache, the dequantised new row included
        K, V = host_dequant(kc1[z, :n], ks1[z, :n]), host_dequant(vc1[z, :n], vs1[z, :n])
        want = attention64(qn[z].view(Hq, 128), K, V, Hkv)
        got = out_c[z].view(Hq, 128).double()
        r = rel(got, want)
        e = float(((got - want).abs() / want.pow(2).mean(dim=1, keepdim=True).sqrt()).max())
        rb = rel(out_c[z], o_pg[z])
        worst = dict(fp64=max(worst["fp64"], r), elem=max(worst["elem"], e), bf16=max(worst["bf16"], rb))
        print(f"[kv8 attn] B {B} Hq {Hq} slot {z} len {n}: vs fp64 rel {r:.3e} worst element {e:.3e} of rms; vs bf16 kernel rel {rb:.3e}")
        assert r < 4e-3, (z, n, r)
        assert e < 2.0 ** -6, (z, n, e)
        assert rb <= 6.5e-2, (z, n, rb)
    return worst


def slot_lengths(B, shift):
    return [LENS[(z + shift) % len(LENS)] for z in range(B)]


@pytest.mark.parametrize("Hq", [12, 4])                     # G = 6 (the model's), G = 2
@pytest.mark.parametrize("B,shift", [(1, i) for i in range(7)] + [(3, 0), (3, 3), (3, 6), (8, 0)])
def test_kv8_attention_appends_quantised_and_matches_fp64(hip, Hq, B, shift):
    """Every length at every batch size; at B = 8 the 4103-row slot's waves stream two 32-key batches.
    Measured over all slots of this file: vs fp64 rel <= 2.2e-3, worst element 1.3e-2 of the rms; vs the bf16 kernel 2.4e-2 to 4.1e-2."""
    check_step(hip, slot_lengths(B, shift), Hq, 2, seed=100 * B + 10 * shift + Hq)


@pytest.mark.parametrize("Hq,Hkv,shift", [(2, 2, 0), (3, 1, 3), (8, 2, 6), (8, 1, 1)])
def test_kv8_attention_at_the_edges_of_the_group_size(hip, Hq, Hkv, shift):
    """G = 1, 3, 4, 8 at B = 3: one to three passes of four rows over the G + 1 rows to normalise, and GMAX.  The same assertions
    and bounds as above: they are on the error against fp64 and do not depend on G."""
    check_step(hip, slot_lengths(3, shift), Hq, Hkv, seed=300 + 10 * shift + Hq + Hkv)


def test_kv8_attention_streams_five_batches_and_rescales(hip):
    """B = 8 at 17 000 rows: 32 blocks per kv head and scene, 534 keys per block, 134 per wave."""
    check_step(hip, [17000, 4103, 33, 357, 2, 17000, 1, 65], 12, 2, seed=17)


def test_kv8_attention_replays_from_a_graph_bit_identically(hip):
    """Three steps (attention, then the lengths advanced on the device) captured once and replayed equal the same three steps
    run eagerly, bit for bit: outputs, codes and scales."""
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
            run_kv8(hip, s, Hq, Hkv, out, ws)
            s["ld"].add_(1)
        if graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()                                        # warm-up outside the capture, then undone
            torch.cuda.current_stream().wait_stream(side)
            for n in ("ld", "kc", "vc", "ks", "vs"):
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
        runs.append((outs, [s[n].clone() for n in ("kc", "vc", "ks", "vs")], s["ld"].clone()))
    (oe, ce, le), (og, cg, lg) = runs
    assert all(torch.equal(a, b) for a, b in zip(oe, og)) and all(torch.isfinite(a.float()).all() for a in oe)
    assert torch.equal(le, lg) and le.tolist() == [n + 3 for n in lens]
    for a, b in zip(ce, cg):                                 # codes and scales: bits (the tail is NaN poison in both)
        a, b = (a, b) if a.dtype == torch.uint8 else (a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(a, b)
    for z, n in enumerate(lens):                             # the three new rows of every slot are written, poison beyond
        assert torch.isfinite(ce[2][z, :n + 2]).all() and torch.isnan(ce[2][z, n + 2:]).all(), z
        assert not (ce[0][z, n - 1:n + 2] == POISON).all(dim=-1).any() and (ce[0][z, n + 2:] == POISON).all(), z


# ------------------------------------------------------------------------------------------------ structured score profiles
def roundtrip(rows):
    """bf16 rows as the e4m3 cache holds them."""
    q, sc = host_quant(rows.reshape(-1, 1, 128))
    return host_dequant(q, sc).view(rows.shape)


@pytest.mark.parametrize("shape,cv", [(sh, cv) for sh in ("b32", "b1", "g8") for cv in P.pg_cases(sh)],
                         ids=lambda v: v if isinstance(v, str) else P.pg_case_id(v))
def test_kv8_attention_on_structured_score_profiles(hip, shape, cv):
    """g2v_decode_attn_pg_kv8 on every family of tests/attn_profile_check.py at the shapes P.PG_SHAPES, the rows through the
    host quantiser: poison at and behind the new row, the appended row's scale bit-equal and its values equal to the quantised
    row of qknorm_mrope_cache, the rows below untouched, and the output inside the hard and the sharp bound against fp64
    attention over the dequantised cache; an exact case (peak 200) equals the peak key's dequantised V row bit for bit."""
    case, variant = cv
    Hq, Hkv, cap, lens = P.PG_SHAPES[shape]
    B, G = len(lens), Hq // Hkv
    new = P.new_row_slots(case, lens, variant)
    s = make_step(hip, lens, Hq, Hkv, 60 + B + variant, cap=cap, edit=lambda qkv: P.align_new_k(qkv, Hq, Hkv, new))
    # the step's q and its new rows in bf16, from the separate kernel
    qn = torch.empty((B, Hq * 128), dtype=torch.bfloat16, device="cuda")
    k3, v3 = s["k16"].cuda(), s["v16"].cuda()
    at = torch.tensor([z * cap + n - 1 for z, n in enumerate(lens)], dtype=torch.int32, device="cuda")
    hip.qknorm_mrope_cache(s["qkv"], Hq, Hkv, s["qw"], s["qw"], s["kw"], s["kw"], 0, 1e-6, 1, s["cos"], s["sin"], qn, k3, v3, at)
    torch.cuda.synchronize()
    qn, k3, v3 = qn.cpu(), k3.cpu(), v3.cpu()
    knew = roundtrip(torch.stack([k3[z, n - 1] for z, n in enumerate(lens)]))
    waves = P.pg_waves(cap, P.pg_nbh(Hkv, B))
    Ks, Vs, infos = P.build_step(case, qn, knew, lens, Hq, Hkv, waves, 61 + variant, variant, quant=roundtrip)
    kc, vc, ks, vs = (s[n].cpu() for n in ("kc", "vc", "ks", "vs"))
    for z, n in enumerate(lens):
        if n > 1:
            kc[z, :n - 1], ks[z, :n - 1] = host_quant(Ks[z])
            vc[z, :n - 1], vs[z, :n - 1] = host_quant(Vs[z])
            assert torch.equal(host_dequant(kc[z, :n - 1], ks[z, :n - 1]), Ks[z])      # the builder's rows ARE cache values
        assert (kc[z, n - 1:] == POISON).all() and (vc[z, n - 1:] == POISON).all(), z
        assert torch.isnan(ks[z, n - 1:]).all() and torch.isnan(vs[z, n - 1:]).all(), z
    if case in (("rise", 20.0), ("fall", 20.0)) and lens[0] > 2000:
        nsc = int(torch.unique(ks[0, :lens[0] - 1, 0]).numel())
        assert nsc >= 6, nsc
    for n_, t in (("kc", kc), ("vc", vc), ("ks", ks), ("vs", vs)):
        s[n_] = t.cuda()
    out = run_kv8(hip, s, Hq, Hkv)
    torch.cuda.synchronize()
    kc1, vc1, ks1, vs1 = (s[n].cpu() for n in ("kc", "vc", "ks", "vs"))
    out = out.cpu()
    name, over = f"attn_pg_kv8 {shape} {P.case_id(case)}", 0
    for z, n in enumerate(lens):
        assert torch.equal(kc1[z, :n - 1], kc[z, :n - 1]) and torch.equal(vc1[z, :n - 1], vc[z, :n - 1]), z
        assert torch.equal(ks1[z, :n - 1], ks[z, :n - 1]) and torch.equal(vs1[z, :n - 1], vs[z, :n - 1]), z
        assert (kc1[z, n:] == POISON).all() and (vc1[z, n:] == POISON).all(), z
        assert torch.isnan(ks1[z, n:]).all() and torch.isnan(vs1[z, n:]).all(), z
        for got_c, got_s, row in ((kc1, ks1, k3[z, n - 1]), (vc1, vs1, v3[z, n - 1])):
            qh, sh = host_quant(row)
            assert torch.equal(got_s[z, n - 1].view(torch.int32), sh.view(torch.int32)), z
            assert torch.equal(host_dequant(got_c[z, n - 1], got_s[z, n - 1]), host_dequant(qh, sh)), z
        K, V = host_dequant(kc1[z, :n], ks1[z, :n]), host_dequant(vc1[z, :n], vs1[z, :n])
        o = out[z].view(Hq, 128)
        over += P.check_slot(PROFILE, name, case[0], o, qn[z].view(Hq, 128), K, V, Hkv)
        for h in range(Hkv):
            if infos[z][h]["exact"]:
                want = V[infos[z][h]["peak"], h].expand(G, 128)
                assert torch.equal(o[h * G:(h + 1) * G].view(torch.int16), want.view(torch.int16)), (z, h)
    w = PROFILE.worst[name]
    print(f"[{name}] |err| / hard {w['hard']:.3f}  |err| / sharp {w['sharp']:.3f}")
    assert over == 0, (name, over, w)
