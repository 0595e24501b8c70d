"""Do two builds of the library compute the same bits in the split-KV decode attention?

    python tools/decode_attn_ab.py LIB_A LIB_B

For each library a fresh child process (G2V_LIB_PATH set, its own timeout) runs g2v_decode_attn_pg, g2v_decode_attn_pg_kv8 and
g2v_decode_attn_shared over one fixed, seeded, CPU-generated case list and prints per case a SHA-256 of the output, of the
zero-initialised workspace after the launch and of the caches (codes and scales for kv8).  The parent compares the two lists and
prints every differing case; exit status 1 if any differs.  The kernels have no atomics and fixed reduction orders, so there is
no tolerance: a difference is a change of arithmetic.  The first child that does not exit 0 ends the run.
"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [1, 2, 32, 33, 65, 357, 4103]                         # cache lengths INCLUDING the new token (tests/test_decode_fp64_gpu.py)
SUFFIX, SMAX = [1, 2, 33, 300], 320                          # tests/test_shared_prefix_gpu.py
CHILD_TIMEOUT = 240


def cases():
    """(entry, name, Hq, Hkv, lens, max_len, und_rounding) for pg / kv8; (entry, name, Hq, Hkv, B, plen, und) for shared."""
    rot = lambda B, shift: [LENS[(z + shift) % len(LENS)] for z in range(B)]
    steps = []
    for Hq in (12, 4):                                       # G = 6, 2 at Hkv 2: every length at B = 1, 3, 8
        for B, shift in [(1, i) for i in range(7)] + [(3, 0), (3, 3), (3, 6), (8, 0)]:
            steps.append((f"G{Hq // 2} B{B} shift{shift}", Hq, 2, rot(B, shift), None))
    for Hq, Hkv in ((2, 2), (3, 1), (8, 2), (8, 1), (16, 2)):      # G = 1, 3, 4, 8: the edges of the norm passes and of GMAX
        for shift in (0, 3, 6):
            steps.append((f"G{Hq // Hkv} Hkv{Hkv} B3 shift{shift}", Hq, Hkv, rot(3, shift), None))
    for Hq in (12, 4):
        steps.append((f"G{Hq // 2} full slot", Hq, 2, [4160, 2, 357], 4160))
        steps.append((f"G{Hq // 2} full slots 357", Hq, 2, [357, 357], 357))
        for n in (1, 2, 129, 130):                           # max_len 130 at B = 1: waves 2 and 3 of every block idle
            steps.append((f"G{Hq // 2} idle waves len{n}", Hq, 2, [n], 130))
    steps.append(("G6 five batches", 12, 2, [17000, 4103, 33, 357, 2, 17000, 1, 65], None))
    out = []
    for entry in ("pg", "kv8"):
        for und in (1, 0):
            out += [(entry, f"{name} und{und}", Hq, Hkv, lens, ml, und) for name, Hq, Hkv, lens, ml in steps]
    for und in (1, 0):
        for Hq, Hkv in ((12, 2), (4, 2)):
            for B in (1, 5, 6, 16):
                for plen in (1, 31, 33, 4103, 17000):
                    out.append(("shared", f"G{Hq // Hkv} B{B} prefix{plen} und{und}", Hq, Hkv, B, plen, und))
        for Hq, Hkv in ((2, 2), (3, 1), (8, 2), (8, 1)):
            for plen in (33, 4103):
                out.append(("shared", f"G{Hq // Hkv} Hkv{Hkv} B3 prefix{plen} und{und}", Hq, Hkv, 3, plen, und))
    return out


def child():
    import torch
    sys.path.insert(0, ROOT)
    from g2vlm_amd import hip
    from g2vlm_amd.quant import quantize_rows_e4m3
    hip.lib()

    def digest(*ts):
        h = hashlib.sha256()
        for t in ts:
            h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
        return h.hexdigest()[:32]

    def quant(x):                                            # bf16 [n, Hkv, 128] -> codes like x, scales [n, Hkv]
        q, s = quantize_rows_e4m3(x.reshape(-1, 128))
        return q.view(x.shape), s.view(x.shape[:-1])

    def common(g, B, Hq, Hkv, pos):
        qkv = torch.randn((B, (Hq + 2 * Hkv) * 128), generator=g).bfloat16().cuda()
        qw = (1 + 0.1 * torch.randn(128, generator=g)).cuda()
        kw = (1 + 0.1 * torch.randn(128, generator=g)).cuda()
        inv_freq = (1.0 / (1e6 ** (torch.arange(0, 128, 2).float() / 128))).cuda()
        cos, sin = hip.mrope_table(torch.tensor([pos] * 3, dtype=torch.int32, device="cuda"), inv_freq)
        return qkv, qw, kw, cos, sin

    scale = 128 ** -0.5
    for ci, c in enumerate(cases()):
        g = torch.Generator(); g.manual_seed(1000 + ci)
        entry, name, Hq, Hkv = c[:4]
        if entry == "shared":
            B, plen, und = c[4:]
            slen = [SUFFIX[(z + ci) % len(SUFFIX)] for z in range(B)]
            qkv, qw, kw, cos, sin = common(g, B, Hq, Hkv, [plen + n - 1 for n in slen])
            kp = torch.randn((plen + 40, Hkv, 128), generator=g).bfloat16()
            vp = torch.randn((plen + 40, Hkv, 128), generator=g).bfloat16()
            kp[plen:] = float("nan"); vp[plen:] = float("nan")
            ks = torch.randn((B, SMAX, Hkv, 128), generator=g).bfloat16()
            vs = torch.randn((B, SMAX, Hkv, 128), generator=g).bfloat16()
            for z, n in enumerate(slen):
                ks[z, n - 1:] = float("nan"); vs[z, n - 1:] = float("nan")
            kp, vp, ks, vs = kp.cuda(), vp.cuda(), ks.cuda(), vs.cuda()
            ld = torch.tensor(slen, dtype=torch.int32, device="cuda")
            out = torch.zeros((B, Hq * 128), dtype=torch.bfloat16, device="cuda")
            ws = torch.zeros(hip.decode_attn_shared_workspace(Hq, Hkv, B, plen, SMAX) // 4, dtype=torch.float32, device="cuda")
            hip.decode_attn_shared(qkv, qw, kw, 1e-6, und, cos, sin, kp, vp, plen, ks, vs, ld, SMAX, SMAX, Hq, Hkv, scale, out, ws)
            caches = (kp, vp, ks, vs)
        else:
            lens, max_len, und = c[4:]
            B = len(lens)
            if max_len is None:
                max_len = (max(lens) + 40 + 63) // 64 * 64
            rows = max_len + 192                             # max_len < scene_rows: the engine's form
            qkv, qw, kw, cos, sin = common(g, B, Hq, Hkv, [n - 1 for n in lens])
            k16 = torch.full((B, rows, Hkv, 128), float("nan"), dtype=torch.bfloat16)
            v16 = torch.full((B, rows, Hkv, 128), float("nan"), dtype=torch.bfloat16)
            for z, n in enumerate(lens):
                if n > 1:
                    k16[z, :n - 1] = torch.randn((n - 1, Hkv, 128), generator=g).bfloat16()
                    v16[z, :n - 1] = torch.randn((n - 1, Hkv, 128), generator=g).bfloat16()
            ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
            out = torch.zeros((B, Hq * 128), dtype=torch.bfloat16, device="cuda")
            ws = torch.zeros(hip.decode_attn_pg_workspace(Hq, Hkv, B) // 4, dtype=torch.float32, device="cuda")
            if entry == "pg":
                kc, vc = k16.cuda(), v16.cuda()
                hip.decode_attn_pg(qkv, qw, kw, 1e-6, und, cos, sin, kc, vc, out, ld, rows, max_len, Hq, Hkv, scale, ws)
                caches = (kc, vc)
            else:
                kc = torch.full((B, rows, Hkv, 128), 0x7F, dtype=torch.uint8)       # the e4m3fn NaN code
                vc = torch.full((B, rows, Hkv, 128), 0x7F, dtype=torch.uint8)
                ksc = torch.full((B, rows, Hkv), float("nan"), dtype=torch.float32)
                vsc = torch.full((B, rows, Hkv), float("nan"), dtype=torch.float32)
                for z, n in enumerate(lens):
                    if n > 1:
                        kc[z, :n - 1], ksc[z, :n - 1] = quant(k16[z, :n - 1])
                        vc[z, :n - 1], vsc[z, :n - 1] = quant(v16[z, :n - 1])
                kc, vc, ksc, vsc = kc.cuda(), vc.cuda(), ksc.cuda(), vsc.cuda()
                hip.decode_attn_pg_kv8(qkv, qw, kw, 1e-6, und, cos, sin, kc, vc, ksc, vsc, out, ld, rows, max_len, Hq, Hkv, scale, ws)
                caches = (kc, vc, ksc, vsc)
        torch.cuda.synchronize()
        print(f"CASE {entry} | {name} | out {digest(out)} ws {digest(ws)} caches {digest(*caches)}", flush=True)
    print(f"DONE {len(cases())}", flush=True)


def main():
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        return child()
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    lists = []
    for lib in sys.argv[1:]:
        env = dict(os.environ, G2V_LIB_PATH=os.path.abspath(lib))
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit(f"{lib}: the child did not end within {CHILD_TIMEOUT} s; nothing more is run")
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("CASE ")]
        if r.returncode != 0 or f"DONE {len(cases())}" not in r.stdout:
            print(r.stdout[-2000:], r.stderr[-4000:], sep="\n")
            sys.exit(f"{lib}: the child ended with status {r.returncode} after {len(lines)} cases; nothing more is run")
        print(f"{lib}: {len(lines)} cases")
        lists.append(lines)
    diff = [(a, b) for a, b in zip(*lists) if a != b]
    for a, b in diff:
        print("DIFFERS\n  A " + a + "\n  B " + b)
    print(f"{len(lists[0])} cases, {len(diff)} differ")
    sys.exit(1 if diff else 0)


if __name__ == "__main__":
    main()
