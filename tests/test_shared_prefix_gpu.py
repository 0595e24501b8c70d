"""GPU: g2v_decode_attn_shared (csrc/decode_shared.hip), one decode-attention step of B query slots over one shared,
read-only prefix plus a suffix block per slot, against an fp64 softmax attention over [prefix | suffix_z] and against
g2v_decode_attn_pg on the concatenated caches."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SUFFIX = [1, 2, 33, 300]                                     # suffix lengths INCLUDING the new token, mixed over the slots
SMAX = 320                                                   # suffix capacity (rows per slot)


@pytest.fixture(scope="module")
def hip():
    from g2vlm_amd import hip as h
    h.lib()
    return h


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def make_step(hip, B, plen, Hq, Hkv, seed, smax=SMAX):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    nh = Hq + 2 * Hkv
    slen = [SUFFIX[(z + seed) % len(SUFFIX)] for z in range(B)]
    qkv = torch.randn((B, nh * 128), generator=g, device="cuda").bfloat16()
    qw = 1 + 0.1 * torch.randn(128, generator=g, device="cuda")
    kw = 1 + 0.1 * torch.randn(128, generator=g, device="cuda")
    pos = torch.tensor([[plen + n - 1 for n in slen]] * 3, dtype=torch.int32, device="cuda")
    inv_freq = (1.0 / (1e6 ** (torch.arange(0, 128, 2).float() / 128))).cuda()
    cos, sin = hip.mrope_table(pos, inv_freq)
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
