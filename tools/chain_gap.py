"""The chained LocalMapping step's serial chain between one LM solve and the next, from a rocprofv3
kernel trace (the sibling of tools/plan_gap.py; same input).

    rocprofv3 --kernel-trace -d DIR -- python bench.py --steps 20 --warmup 5
    python tools/rocpd_to_csv.py DIR/.../*_results.db PREFIX
    python tools/chain_gap.py PREFIX_kernel_trace.csv [--skip N] [--names]

Per step: the window from the end of a solve's last k_ba_bs2 to the start of the next solve's
k_ba_init, split into kernel time (the union of the dispatches inside the window, clipped to it:
the trace has no stream column, so a side-stream kernel that happens to run there counts as busy
time too) and idle time (the rest).  Prints every window and the median / min / max over the windows
after the first N; --names adds the kernels of the last window in start order."""
import argparse
import csv
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--skip", type=int, default=5, help="leading windows left out of the summary (warm-up)")
    ap.add_argument("--names", action="store_true")
    args = ap.parse_args()
    with open(args.trace, newline="") as f:
        rows = [(r["Kernel_Name"], int(float(r["Start_Timestamp"])), int(float(r["End_Timestamp"]))) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    windows, bs2_end = [], None
    for name, s, e in rows:
        if "k_ba_bs2" in name:  # (names may be mangled)
            bs2_end = e
        elif "k_ba_init" in name and bs2_end is not None:
            windows.append((bs2_end, s))
            bs2_end = None
    out, last = [], []
    for a, b in windows:
        inside = sorted((max(s, a), min(e, b), n) for n, s, e in rows if e > a and s < b and "k_ba_bs2" not in n)
        busy, cur = 0, a
        for s, e, _ in inside:
            if e > cur:
                busy += e - max(s, cur)
                cur = e
        out.append(((b - a) / 1e3, busy / 1e3, (b - a - busy) / 1e3, len(inside)))
        last = inside
    for i, (w, k, idle, n) in enumerate(out):
        print(f"step {i:3d}  last bs2 end -> k_ba_init start {w:8.2f} us   kernels {k:8.2f} us ({n:2d})   idle {idle:8.2f} us")
    for label, j in (("window", 0), ("kernel time", 1), ("idle time", 2)):
        v = [o[j] for o in out[args.skip:]]
        if v:
            print(f"{label}: median {statistics.median(v):.2f} us, min {min(v):.2f}, max {max(v):.2f} over {len(v)} steps")
    if args.names and windows:
        a = windows[-1][0]
        for s, e, n in last:
            print(f"  +{(s - a) / 1e3:7.2f} us  {(e - s) / 1e3:6.2f} us  {n[:60]}")


if __name__ == "__main__":
    main()
