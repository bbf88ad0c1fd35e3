"""When did each kernel of a traced run start and end?  Reads the kernel-trace CSV of a `rocprofv3 --kernel-trace
--output-format csv` run and prints, for every dispatch whose name holds one of the given substrings, its queue, its
start and end in milliseconds from the first listed dispatch and its duration -- and for every dispatch that began
while an earlier listed one was still running, which one and for how long the two overlapped.

    python tools/kernel_intervals.py run_kernel_trace.csv [k_paths k_accum ...] [--last N]

--last N keeps the last N listed dispatches (the timed step of a bench run after its warm-up)."""
import argparse
import csv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("names", nargs="*", default=["k_paths", "k_accum"])
    ap.add_argument("--last", type=int, default=0)
    a = ap.parse_args()
    rows = []
    with open(a.csv, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if any(n in name for n in a.names):
                short = name.split("(")[0].replace("art::", "")
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short, r.get("Queue_Id", "?")))
    rows.sort()
    if a.last:
        rows = rows[-a.last:]
    if not rows:
        print("no dispatch matches")
        return
    t0 = rows[0][0]
    print(f"{'kernel':<24} {'queue':>6} {'start ms':>10} {'end ms':>10} {'ms':>9}")
    for i, (s, e, name, q) in enumerate(rows):
        line = f"{name:<24} {q:>6} {(s - t0) / 1e6:10.3f} {(e - t0) / 1e6:10.3f} {(e - s) / 1e6:9.3f}"
        for s2, e2, name2, _q2 in rows[:i]:
            both = min(e, e2) - max(s, s2)
            if both > 0:
                line += f"  | {both / 1e6:.3f} ms inside {name2} [{(s2 - t0) / 1e6:.3f}, {(e2 - t0) / 1e6:.3f}]"
        print(line)
    print(f"first start to last end: {(max(r[1] for r in rows) - t0) / 1e6:.3f} ms")


if __name__ == "__main__":
    main()
