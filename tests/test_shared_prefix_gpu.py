"""GPU: g2v_decode_attn_shared (csrc/decode_shared.hip), one decode-attention step of B query slots over one shared,
read-only prefix plus a suffix block per slot, against an fp64 softmax attention over [prefix | suffix_z] and against
g2v_decode_attn_pg on the concatenated caches.

Structured score profiles (tests/attn_profile_check.py, proven on the CPU by tests/test_attn_profile_cpu.py) at B = 16 over a
prefix of 17000 rows: the slots of a column group see a family and its mirror image through the same K batches.  Zero elements
over the hard or the sharp bound, the peak-200 cases bit-equal to the peak key's V row, in the prefix and in the suffix.
Measured maxima of |err| / hard and |err| / sharp on an MI355X | the CPU emulation:
  saw 0.08 / 0.43 | 0.08 / 0.39          rise 0.61 / 0.37 | 0.73 / 0.44         fall 0.52 / 0.38 | 0.65 / 0.43     wide 0.46 / 0.31 | 0.48 / 0.32
  peak_prefix 0.47 / 0.36 | 0.47 / 0.32  peak_suffix 0.42 / 0.34 | 0.39 / 0.34  offset 0.05 / 0.40 | 0.05 / 0.38   flat 0.02 / - | 0.02 / -
g2v_decode_attn_pg on the concatenated caches under the same bounds (saw 20 / 70, rise 20, fall 20, peak): 0.61 / 0.40 at most."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_profile_check as P  # noqa: E402

SUFFIX = [1, 2, 33, 300]                                     # suffix lengths INCLUDING the new token, mixed over the slots
SMAX = 320                                                   # suffix capacity (rows per slot)
PROFILE = P.Ratios()


@pytest.fixture(scope="module", autouse=True)
def measured():
    yield
    PROFILE.report("shared prefix profiles")


@pytest.fixture(scope="module")
def hip():
    from g2vlm_amd import hip as h
    h.lib()
    return h


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def make_step(hip, B, plen, Hq, Hkv, seed, smax=SMAX, q_target=None):
    """q_target fp32 [B, Hq, 128] (host): the raw q rows are chosen so that norm + rotation leave them along these rows
    (the rotation of the slot's position undone, divided by the norm weight; the norm fixes the length)."""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    nh = Hq + 2 * Hkv
    slen = [SUFFIX[(z + seed) % len(SUFFIX)] for z in range(B)]
    qkv = torch.randn((B, nh * 128), generator=g, device="cuda").bfloat16()
    qw = 1 + 0.1 * torch.randn(128, generator=g, device="cuda")
    kw = 1 + 0.1 * torch.randn(128, generator=g, device="cuda")
    pos = torch.tensor([[plen + n - 1 for n in slen]] * 3, dtype=torch.int32, device="cuda")
    inv_freq = (1.0 / (1e6 ** (torch.arange(0, 128, 2).float() / 128))).cuda()
    cos, sin = hip.mrope_table(pos, inv_freq)
    if q_target is not None:
        c, sn, o = cos.double().cpu().unsqueeze(1), sin.double().cpu().unsqueeze(1), q_target.double()
        det = c[..., :64] * c[..., 64:] + sn[..., :64] * sn[..., 64:]
        n0 = (o[..., :64] * c[..., 64:] + o[..., 64:] * sn[..., :64]) / det
        n1 = (o[..., 64:] * c[..., :64] - o[..., :64] * sn[..., 64:]) / det
        raw = torch.cat([n0, n1], -1) / qw.double().cpu()
        qkv[:, :Hq * 128] = raw.reshape(B, Hq * 128).bfloat16().cuda()
    kp = torch.randn((plen + 40, Hkv, 128), generator=g, device="cuda").bfloat16()
    vp = torch.randn((plen + 40, Hkv, 128), generator=g, device="cuda").bfloat16()
    kp[plen:] = float("nan"); vp[plen:] = float("nan")      # past the prefix: never to reach the output
    ks = torch.randn((B, smax, Hkv, 128), generator=g, device="cuda").bfloat16()
    vs = torch.randn((B, smax, Hkv, 128), generator=g, device="cuda").bfloat16()
    for z, n in enumerate(slen):
        ks[z, n - 1:] = float("nan"); vs[z, n - 1:] = float("nan")     # the new row and everything after it
    return dict(qkv=qkv, qw=qw, kw=kw, cos=cos, sin=sin, kp=kp, vp=vp, ks=ks, vs=vs, slen=slen,
                ld=torch.tensor(slen, dtype=torch.int32, device="cuda"))


def run_shared(hip, s, plen, Hq, Hkv, smax=SMAX):
    B = s["qkv"].shape[0]
    out = torch.full((B, Hq * 128), float("nan"), dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(hip.decode_attn_shared_workspace(Hq, Hkv, B, plen, smax) // 4, dtype=torch.float32, device="cuda")
    hip.decode_attn_shared(s["qkv"], s["qw"], s["kw"], 1e-6, 1, s["cos"], s["sin"], s["kp"], s["vp"], plen, s["ks"], s["vs"], s["ld"],
                           smax, smax, Hq, Hkv, 128 ** -0.5, out, ws)
    return out


@pytest.mark.parametrize("Hq", [12, 4])                     # G = 6 (the model's), G = 2
@pytest.mark.parametrize("B", [1, 5, 6, 16])
@pytest.mark.parametrize("plen", [1, 31, 33, 4103, 17000])
def test_shared_prefix_attention_matches_fp64_and_the_concatenated_cache(hip, Hq, B, plen):
    check_shared(hip, Hq, 2, B, plen)


@pytest.mark.parametrize("Hq,Hkv,plen", [(2, 2, 33), (3, 1, 4103), (8, 2, 31), (8, 1, 4103)])
def test_shared_prefix_attention_at_the_edges_of_the_group_size(hip, Hq, Hkv, plen):
    """G = 1, 3, 4, 8 at B = 3 (32, 10, 8 and 4 slots per column group): the same assertions and bounds, which do not depend on G."""
    check_shared(hip, Hq, Hkv, 3, plen)


def check_shared(hip, Hq, Hkv, B, plen):
    G = Hq // Hkv
    s = make_step(hip, B, plen, Hq, Hkv, seed=plen + 7 * B + Hq)
    kp0, vp0, ks0, vs0 = s["kp"].clone(), s["vp"].clone(), s["ks"].clone(), s["vs"].clone()
    out = run_shared(hip, s, plen, Hq, Hkv)
    torch.cuda.synchronize()
    slen = s["slen"]
    # the prefix is read only (its NaN tail included); suffix rows past the new one are untouched
    assert torch.equal(s["kp"][:plen], kp0[:plen]) and torch.equal(s["vp"][:plen], vp0[:plen])
    assert torch.isnan(s["kp"][plen:].float()).all() and torch.isnan(s["vp"][plen:].float()).all()
    for z, n in enumerate(slen):
        assert torch.equal(s["ks"][z, :n - 1], ks0[z, :n - 1]) and torch.equal(s["vs"][z, :n - 1], vs0[z, :n - 1]), z
        assert torch.isnan(s["ks"][z, n:].float()).all() and torch.isnan(s["vs"][z, n:].float()).all(), z
        assert torch.isfinite(s["ks"][z, n - 1].float()).all() and torch.isfinite(s["vs"][z, n - 1].float()).all(), z
    assert torch.isfinite(out.float()).all()

    # g2v_decode_attn_pg on the concatenated caches: the same appended rows, bit for bit, the same output up to fp32 order
    cap = plen + SMAX
    kc = torch.full((B, cap, Hkv, 128), float("nan"), dtype=torch.bfloat16, device="cuda")
    vc = torch.full_like(kc, float("nan"))
    for z, n in enumerate(slen):
        kc[z, :plen] = kp0[:plen]; vc[z, :plen] = vp0[:plen]
        kc[z, plen:plen + n - 1] = ks0[z, :n - 1]; vc[z, plen:plen + n - 1] = vs0[z, :n - 1]
    ld_cat = torch.tensor([plen + n for n in slen], dtype=torch.int32, device="cuda")
    o_pg = torch.empty_like(out)
    ws2 = torch.empty(hip.decode_attn_pg_workspace(Hq, Hkv, B) // 4, dtype=torch.float32, device="cuda")
    hip.decode_attn_pg(s["qkv"], s["qw"], s["kw"], 1e-6, 1, s["cos"], s["sin"], kc, vc, o_pg, ld_cat, cap, cap, Hq, Hkv, 128 ** -0.5, ws2)
    for z, n in enumerate(slen):
        assert torch.equal(kc[z, plen + n - 1], s["ks"][z, n - 1]) and torch.equal(vc[z, plen + n - 1], s["vs"][z, n - 1]), z
        assert rel(out[z], o_pg[z]) < 4e-3, (z, rel(out[z], o_pg[z]))

    # fp64 softmax attention over [prefix | suffix_z]; q after norm + rope from the separate kernel
    qn = torch.empty((B, Hq * 128), dtype=torch.bfloat16, device="cuda")
    k3, v3 = ks0.clone(), vs0.clone()
    rows = torch.tensor([z * SMAX + n - 1 for z, n in enumerate(slen)], dtype=torch.int32, device="cuda")
    hip.qknorm_mrope_cache(s["qkv"], Hq, Hkv, s["qw"], s["qw"], s["kw"], s["kw"], 0, 1e-6, 1, s["cos"], s["sin"], qn, k3, v3, rows)
    kpd, vpd = kp0[:plen].double().cpu(), vp0[:plen].double().cpu()
    for z, n in enumerate(slen):
        assert torch.equal(k3[z, n - 1], s["ks"][z, n - 1]), z
        K = torch.cat([kpd, s["ks"][z, :n].double().cpu()])             # [L, Hkv, 128]
        V = torch.cat([vpd, s["vs"][z, :n].double().cpu()])
        q = qn[z].view(Hq, 128).double().cpu()
        want = torch.empty((Hq, 128), dtype=torch.float64)
        for kvh in range(Hkv):
            qh = q[kvh * G:(kvh + 1) * G]
            p = torch.softmax((qh @ K[:, kvh].T) * 128 ** -0.5, dim=-1)
            want[kvh * G:(kvh + 1) * G] = p @ V[:, kvh]
        got = out[z].view(Hq, 128).double().cpu()
        assert rel(got, want) < 4e-3, (z, rel(got, want))
        assert float(((got - want).abs() / want.pow(2).mean(dim=1, keepdim=True).sqrt()).max()) < 2.0 ** -6, z


def test_shared_prefix_attention_replays_from_a_graph_bit_identically(hip):
    """Three steps (attention, then the lengths advanced on the device) captured once and replayed equal the same three
    steps run eagerly, bit for bit: output and appended rows."""
    Hq, Hkv, B, plen = 12, 2, 6, 4103
    base = make_step(hip, B, plen, Hq, Hkv, seed=99)
    runs = []
    for graph in (False, True):
        s = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in base.items()}
        out = torch.empty((B, Hq * 128), dtype=torch.bfloat16, device="cuda")
        ws = torch.empty(hip.decode_attn_shared_workspace(Hq, Hkv, B, plen, SMAX) // 4, dtype=torch.float32, device="cuda")
        outs = []

        def step():
            hip.decode_attn_shared(s["qkv"], s["qw"], s["kw"], 1e-6, 1, s["cos"], s["sin"], s["kp"], s["vp"], plen, s["ks"], s["vs"],
                                   s["ld"], SMAX, SMAX, Hq, Hkv, 128 ** -0.5, out, ws)
            s["ld"].add_(1)
        if graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()                                        # warm-up outside the capture, then undone
            torch.cuda.current_stream().wait_stream(side)
            s["ld"].copy_(base["ld"])
            s["ks"].copy_(base["ks"]); s["vs"].copy_(base["vs"])
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
        runs.append((outs, s["ks"].clone(), s["vs"].clone(), s["ld"].clone()))
    (oe, ke, ve, le), (og, kg, vg, lg) = runs
    assert all(torch.equal(a, b) for a, b in zip(oe, og))
    assert torch.equal(le, lg) and le.tolist() == [n + 3 for n in base["slen"]]
    # rows written: the three new rows of every slot; NaN beyond
    for z, n in enumerate(base["slen"]):
        assert torch.equal(ke[z, :n + 2], kg[z, :n + 2]) and torch.equal(ve[z, :n + 2], vg[z, :n + 2]), z
        assert torch.isfinite(ke[z, :n + 2].float()).all()
        assert torch.isnan(kg[z, n + 2:].float()).all()


# ------------------------------------------------------------------------------------------------ structured score profiles
@pytest.mark.parametrize("case", P.SHARED_CASES, ids=P.case_id)
def test_shared_prefix_attention_on_structured_score_profiles(hip, case):
    """g2v_decode_attn_shared at B = 16 over a prefix of 17000 rows (four column groups, 96 prefix rows per wave: three
    batches; 40 suffix rows per wave: two) on the families of tests/attn_profile_check.py.  The prefix rows are shared, so the
    profile comes from q: the slots of a column group alternate in the sign of their q along the profile direction and see the
    profile and its mirror image through the same K batches.  Checked: NaN at and behind every new row before the step, the
    appended rows bit for bit against qknorm_mrope_cache, the prefix and the rows below untouched, the output inside the hard
    and the sharp bound against fp64 (no element exempt), the exact cases bit for bit, and g2v_decode_attn_pg on the
    concatenated caches: rel < 4e-3 of the reference row where the output is a spread-out average (saw 0.5 / 3, rise 0.5, fall
    0.5, wide, offset, flat), and inside the same two bounds for the families whose output is a few V rows, where the norm of
    the row no longer says what a rounding of a weight may cost (saw 20 / 70, rise 20, fall 20, peak)."""
    Hq, Hkv, B, plen = (P.SHARED_SHAPE[k] for k in ("Hq", "Hkv", "B", "plen"))
    G = Hq // Hkv
    plan = P.shared_plan(Hq, Hkv, B, plen, SMAX)
    signs = P.slot_signs(B, plan["spg"])
    d = P.shared_directions(Hkv, 5)
    s = make_step(hip, B, plen, Hq, Hkv, seed=21, q_target=P.shared_targets(B, Hq, Hkv, d, signs, 6))
    slen = s["slen"]
    # q and the new rows from the separate kernel
    qn = torch.empty((B, Hq * 128), dtype=torch.bfloat16, device="cuda")
    k3, v3 = torch.zeros_like(s["ks"]), torch.zeros_like(s["vs"])
    rows = torch.tensor([z * SMAX + n - 1 for z, n in enumerate(slen)], dtype=torch.int32, device="cuda")
    hip.qknorm_mrope_cache(s["qkv"], Hq, Hkv, s["qw"], s["qw"], s["kw"], s["kw"], 0, 1e-6, 1, s["cos"], s["sin"], qn, k3, v3, rows)
    torch.cuda.synchronize()
    qn, k3, v3 = qn.cpu(), k3.cpu(), v3.cpu()
    knew = torch.stack([k3[z, n - 1] for z, n in enumerate(slen)])
    vnew = torch.stack([v3[z, n - 1] for z, n in enumerate(slen)])
    Kp, Vp, Ks, Vs, exact = P.build_shared(case, qn, knew, slen, Hq, Hkv, plen, SMAX, d, signs, seed=22)
    s["kp"][:plen], s["vp"][:plen] = Kp.cuda(), Vp.cuda()
    for z, n in enumerate(slen):
        s["ks"][z, :n - 1], s["vs"][z, :n - 1] = Ks[z].cuda(), Vs[z].cuda()
        assert torch.isnan(s["ks"][z, n - 1:].float()).all() and torch.isnan(s["vs"][z, n - 1:].float()).all(), z
    assert torch.isnan(s["kp"][plen:].float()).all() and torch.isnan(s["vp"][plen:].float()).all()
    out = run_shared(hip, s, plen, Hq, Hkv)
    torch.cuda.synchronize()
    assert torch.equal(s["kp"][:plen].cpu(), Kp) and torch.equal(s["vp"][:plen].cpu(), Vp)
    assert torch.isnan(s["kp"][plen:].float()).all() and torch.isnan(s["vp"][plen:].float()).all()
    # g2v_decode_attn_pg on the concatenated caches
    cap = plen + SMAX
    kc = torch.full((B, cap, Hkv, 128), float("nan"), dtype=torch.bfloat16, device="cuda")
    vc = torch.full_like(kc, float("nan"))
    for z, n in enumerate(slen):
        kc[z, :plen] = s["kp"][:plen]; vc[z, :plen] = s["vp"][:plen]
        kc[z, plen:plen + n - 1] = s["ks"][z, :n - 1]; vc[z, plen:plen + n - 1] = s["vs"][z, :n - 1]
    ld_cat = torch.tensor([plen + n for n in slen], dtype=torch.int32, device="cuda")
    o_pg = torch.full_like(out, float("nan"))
    ws2 = torch.empty(hip.decode_attn_pg_workspace(Hq, Hkv, B) // 4, dtype=torch.float32, device="cuda")
    hip.decode_attn_pg(s["qkv"], s["qw"], s["kw"], 1e-6, 1, s["cos"], s["sin"], kc, vc, o_pg, ld_cat, cap, cap, Hq, Hkv, 128 ** -0.5, ws2)
    torch.cuda.synchronize()
    ks1, vs1, out, o_pg = s["ks"].cpu(), s["vs"].cpu(), out.cpu(), o_pg.cpu()
    fam = "peak" if case[0].startswith("peak") else case[0]
    rel_ok = fam in ("wide", "offset", "flat") or (fam in ("saw", "rise", "fall") and case[1] <= 3.0)
    name, over = f"attn_shared {P.case_id(case)}", 0
    for z, n in enumerate(slen):
        assert torch.equal(ks1[z, :n - 1], Ks[z]) and torch.equal(vs1[z, :n - 1], Vs[z]), z
        assert torch.equal(ks1[z, n - 1].view(torch.int16), knew[z].view(torch.int16)), z
        assert torch.equal(vs1[z, n - 1].view(torch.int16), vnew[z].view(torch.int16)), z
        assert torch.isnan(ks1[z, n:].float()).all() and torch.isnan(vs1[z, n:].float()).all(), z
        assert torch.equal(kc[z, plen + n - 1].cpu().view(torch.int16), knew[z].view(torch.int16)), z
        K, V = torch.cat([Kp, ks1[z, :n]]), torch.cat([Vp, vs1[z, :n]])
        q, o = qn[z].view(Hq, 128), out[z].view(Hq, 128)
        over += P.check_slot(PROFILE, name, fam, o, q, K, V, Hkv)
        if rel_ok:
            assert rel(out[z], o_pg[z]) < 4e-3, (z, rel(out[z], o_pg[z]))
        else:
            over += P.check_slot(PROFILE, name + " (attn_pg, concatenated)", fam, o_pg[z].view(Hq, 128), q, K, V, Hkv)
        if exact[z] is not None:
            row = exact[z][1] + (plen if exact[z][0] == "suffix" else 0)
            want = V[row].unsqueeze(1).expand(Hkv, G, 128).reshape(Hq, 128)
            assert torch.equal(o.view(torch.int16), want.view(torch.int16)), (z, exact[z])
            assert torch.equal(o_pg[z].view(Hq, 128).view(torch.int16), want.view(torch.int16)), (z, exact[z])
    w = PROFILE.worst[name]
    print(f"[{name}] |err| / hard {w['hard']:.3f}  |err| / sharp {w['sharp']:.3f}")
    assert over == 0, (name, over, w)
