"""Per-kernel split of the LAST pass of a repeated workload from a rocprofv3 rocpd database: the launches behind the last but one
launch of the marker kernel (the one that ends a pass) up to the last one, grouped by name, and the pass's final launches one by one.
    rocprofv3 --kernel-trace --stats -d prof -o choices -- python tools/bench_choices.py --only score
    python3 tools/rocpd_last_pass.py prof/choices_results.db logprob_rows_bf16_kernel [tail] > profiles/choices_c5_pass_split.txt
With the scoring pass the tail (default 3) is the final norm, the lm_head GEMM and the log-probability kernel."""
import sqlite3
import sys

from rocpd_stats import short


def main():
    db = sqlite3.connect(sys.argv[1])
    marker = sys.argv[2]
    tail = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    ks = [(short(n), s, e) for n, s, e in db.execute("select name, start, end from kernels order by start")]
    ends = [i for i, k in enumerate(ks) if marker in k[0]]
    if not ends:
        sys.exit(f"no launch of {marker} in {sys.argv[1]}")
    ks = ks[ends[-2] + 1 if len(ends) > 1 else 0:ends[-1] + 1]
    busy = sum(e - s for _, s, e in ks)
    print(f"last pass ending in {marker}: {len(ks)} kernels, span {(ks[-1][2] - ks[0][1]) / 1e3:.1f} us, kernel time {busy / 1e3:.1f} us")
    by = {}
    for n, s, e in ks:
        c, t = by.get(n, (0, 0))
        by[n] = (c + 1, t + e - s)
    for n, (c, t) in sorted(by.items(), key=lambda kv: -kv[1][1]):
        print(f"{n[:70]:70s} {c:6d} calls {t / 1e3:9.1f} us {100.0 * t / busy:5.1f} %")
    print(f"the last {min(tail, len(ks))} launches of the pass, in order:")
    for n, s, e in ks[-tail:]:
        print(f"{n[:70]:70s}              {(e - s) / 1e3:9.1f} us {100.0 * (e - s) / busy:5.1f} %")


if __name__ == "__main__":
    main()
