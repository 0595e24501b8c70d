"""Do two builds of the library compute the same bits in the two 256x256 GEMM forms (csrc/gemm_8p.hip, csrc/gemm_4w.hip)?

    python tools/gemm_ab.py LIB_A LIB_B

For each library a fresh child process (G2V_LIB_PATH set, its own timeout) runs g2v_gemm_bf16 over one fixed, seeded case list and
prints per case a SHA-256 of the whole C buffer - padding columns, gap and sentinel rows included.  The parent compares the two
lists and prints every differing case; exit status 1 if any differs.  The kernels have fixed summation orders, so there is no
tolerance: a difference is a change of arithmetic.  The first child that does not exit 0 ends the run.

Cases (the form is forced by flags, never chosen by shape; operands and layout are tests/test_gemm_fp64_gpu.py's Launch):
  heights   both forms x every tile height x every epilogue variant of EPIS, M = h + {1, h/2 + 1, h}, N 512, K 128 / 192
  ab        the lockstep two-barrier and the pipelined loop at heights 160 and 288, bf16 and fp32 residual
  groups    the two-group cases of test_two_groups: either order, either group empty, gamma on one group, in place
  persist   more tiles than CUs at height 128, N 2048: groups of 128 ceil(CUs / 8) + 1 and 6 rows in both orders, so that
            a workgroup finishes a tile of one group and prefetches a tile of the other
"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300


def cases(hip, T, n_cu):
    """(name, Launch keyword arguments, flags)"""
    forms = {"8p": hip.FORCE_8P | hip.P8_EIGHT_WAVES, "4w": hip.FORCE_8P | hip.P8_FOUR_WAVES}
    out = []
    for form, fl in forms.items():
        for h in T.HEIGHTS:
            K = 128 if h in (128, 192, 256) else 192
            for name, (epi, kw) in T.EPIS.items():
                for j, t in enumerate((1, h // 2 + 1, h)):
                    out.append((f"heights {form} h{h} M{h + t} K{K} {name}",
                                dict(epi=epi, Ms=[h + t], N=512, K=K, lda_pad=64, ldc_pad=16, seed=1000 * h + j, **kw), fl | T.hflag(hip, h)))
    for loop, fl in (("two_barrier", hip.P8_TWO_BARRIER), ("pipelined", hip.P8_PIPELINED)):
        for h in (160, 288):
            for name in ("bf16", "res_f32_gamma_round"):
                epi, kw = T.EPIS[name]
                for j, t in enumerate((1, h // 2 + 1, h)):
                    out.append((f"ab {loop} h{h} M{h + t} {name}",
                                dict(epi=epi, Ms=[h + t], N=512, K=192, lda_pad=64, ldc_pad=16, seed=90 + h + j, **kw), hip.FORCE_8P | fl | T.hflag(hip, h)))
    two = [(700, u) for u in (1, 6, 16, 128, 129)] + [(700, 0), (0, 300)]
    persist = (128 * ((n_cu + 7) // 8) + 1, 6)
    for form, fl in forms.items():
        for j, pair in enumerate(two):
            for order in ((0, 1), (1, 0)):
                Ms = [pair[o] for o in order]
                gam = tuple((True, False)[o] for o in order)
                for name, epi, kw in (("res_f32_mot", T.G.EPI_RES_F32, dict(gammas=gam, round_gamma=True, inplace=True, bias=False, ldc_pad=8)),
                                      ("bf16", T.G.EPI_BF16, dict(ldc_pad=16)), ("swiglu", T.G.EPI_SWIGLU, dict(ldc_pad=16))):
                    out.append((f"groups {form} {Ms} {name}", dict(epi=epi, Ms=Ms, N=512, K=256, lda_pad=64, seed=150 + 10 * j + order[0], **kw),
                                fl | hip.P8_H256))
        for order in ((0, 1), (1, 0)):
            Ms = [persist[o] for o in order]
            for name in ("swiglu", "res_f32_gamma_inplace"):
                epi, kw = T.EPIS[name]
                out.append((f"persist {form} {Ms} {name}", dict(epi=epi, Ms=Ms, N=2048, K=128, lda_pad=64, ldc_pad=16, seed=170 + order[0], **kw),
                            fl | hip.P8_H128))
    return out


def child():
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gemm_fp64_gpu as T
    from g2vlm_amd import hip
    hip.lib()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    cs = cases(hip, T, n_cu)
    for name, kw, fl in cs:
        kw = dict(kw)
        L = T.Launch(hip, kw.pop("epi"), kw.pop("Ms"), kw.pop("N"), kw.pop("K"), **kw)
        form = name.split()[1] if name.split()[0] != "ab" else "8p"
        route = L.route(fl)
        assert route[0] == form, (name, route)
        L.run(fl)
        digest = hashlib.sha256(L.Cbuf.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]
        print(f"CASE {name} | C {digest}", flush=True)
    print(f"DONE {len(cs)}", flush=True)


def main():
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        return child()
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    lists = []
    for lib in sys.argv[1:]:
        env = dict(os.environ, G2V_LIB_PATH=os.path.abspath(lib))
        env.pop("G2V_GEMM_FLAGS", None); env.pop("G2V_GEMM_4W_MASK", None)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            sys.exit(f"{lib}: the child did not end within {CHILD_TIMEOUT} s; nothing more is run")
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("CASE ")]
        if r.returncode != 0 or f"DONE {len(lines)}" not in r.stdout or not lines:
            print(r.stdout[-2000:], r.stderr[-4000:], sep="\n")
            sys.exit(f"{lib}: the child ended with status {r.returncode} after {len(lines)} cases; nothing more is run")
        print(f"{lib}: {len(lines)} cases")
        lists.append(lines)
    if len(lists[0]) != len(lists[1]):
        sys.exit("the two children ran different case lists")
    diff = [(a, b) for a, b in zip(*lists) if a != b]
    for a, b in diff:
        print("DIFFERS\n  A " + a + "\n  B " + b)
    print(f"{len(lists[0])} cases, {len(diff)} differ")
    sys.exit(1 if diff else 0)


if __name__ == "__main__":
    main()
