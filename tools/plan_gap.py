"""Idle time of the chained LocalMapping step's plan build, from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace -d DIR -- python bench.py --steps 20 --warmup 5
    python tools/rocpd_to_csv.py DIR/.../*_results.db PREFIX
    python tools/plan_gap.py PREFIX_kernel_trace.csv [--skip N]

Per step: the time from the end of k_db_sorted (phase 1 of the device plan build) to the start of the
k_db_gather that follows it, and from that gather's end to the start of the next k_ba_* kernel (the LM
graph).  Prints every step's figures and the median / min / max over the steps after the first N."""
import argparse
import csv
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--skip", type=int, default=5, help="leading steps left out of the summary (warm-up)")
    args = ap.parse_args()
    with open(args.trace, newline="") as f:
        rows = [(r["Kernel_Name"], int(float(r["Start_Timestamp"])), int(float(r["End_Timestamp"]))) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    gaps, to_lm, sorted_end, gather_end = [], [], None, None
    for name, s, e in rows:
        if "k_db_sorted" in name:  # (names may be mangled)
            sorted_end, gather_end = e, None
        elif "k_db_gather" in name and sorted_end is not None:
            gaps.append((s - sorted_end) / 1e3)
            sorted_end, gather_end = None, e
        elif "k_ba_" in name and gather_end is not None:
            to_lm.append((s - gather_end) / 1e3)
            gather_end = None
    for i, g in enumerate(gaps):
        lm = f"{to_lm[i]:8.2f}" if i < len(to_lm) else "       -"
        print(f"step {i:3d}  sorted end -> gather start {g:8.2f} us   gather end -> first k_ba {lm} us")
    for label, v in (("sorted end -> gather start", gaps[args.skip:]), ("gather end -> first k_ba", to_lm[args.skip:])):
        if v:
            print(f"{label}: median {statistics.median(v):.2f} us, min {min(v):.2f}, max {max(v):.2f} over {len(v)} steps")


if __name__ == "__main__":
    main()
