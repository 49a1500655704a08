#!/usr/bin/env python3
"""What a rocprofv3 kernel trace says about consecutive channel-kernel launches:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o k -- python bench.py --gpus 1 --steps 20 --warmup 5
    python tools/launch_overlap_trace.py <dir> [last N launches, default 20]

For the last N channel-kernel launches: duration, the time from one launch's end to the next one's start (negative: the next
one started that long before the end - the launches overlap) and the period from start to start; where the engine's carry
kernel (mfm_carry_kernel) ran relative to the end of the channel kernel in flight when it started and to the start of the
launch that reads what it copied; and which queue the dispatches of each kernel went to."""
import csv
import glob
import os
import sys


def main():
    d = sys.argv[1]
    last = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    tr = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not tr:
        raise SystemExit("no *kernel_trace.csv under %s" % d)
    rows = list(csv.DictReader(open(tr[0])))
    for r in rows:
        r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    ch = sorted([r for r in rows if "mfm_channel_kernel" in r["Kernel_Name"]], key=lambda r: r["s"])
    ca = sorted([r for r in rows if "mfm_carry_kernel" in r["Kernel_Name"]], key=lambda r: r["s"])
    print("%d channel-kernel dispatches, %d carry-kernel dispatches in %s" % (len(ch), len(ca), os.path.basename(tr[0])))
    tail = ch[-last:]
    dur = [(r["e"] - r["s"]) / 1e3 for r in tail]
    gap = [(b["s"] - a["e"]) / 1e3 for a, b in zip(tail[:-1], tail[1:])]
    per = [(b["s"] - a["s"]) / 1e3 for a, b in zip(tail[:-1], tail[1:])]
    mean = lambda v: sum(v) / len(v) if v else float("nan")
    print("last %d launches: duration mean %.2f us (min %.2f max %.2f)" % (len(tail), mean(dur), min(dur), max(dur)))
    print("  end of launch n -> start of launch n+1: mean %+.2f us (min %+.2f max %+.2f); negative = overlap" % (mean(gap), min(gap), max(gap)))
    print("  start -> start: mean %.2f us; first start -> last end over %d launches: %.2f us per launch"
          % (mean(per), len(tail), (tail[-1]["e"] - tail[0]["s"]) / 1e3 / len(tail)))
    qs = {}
    for r in tail:
        qs.setdefault(r.get("Queue_Id", "?"), 0)
        qs[r.get("Queue_Id", "?")] += 1
    print("  queues of these launches: " + ", ".join("queue %s x %d" % kv for kv in sorted(qs.items())))
    if ca:
        t0 = tail[0]["s"]
        cc = [r for r in ca if r["s"] >= t0]
        after_start, before_end, lead = [], [], []
        for r in cc:
            running = [k for k in ch if k["s"] <= r["s"] < k["e"]]
            nxt = [k for k in ch if k["s"] > r["e"]]
            if running:
                after_start.append((r["s"] - running[-1]["s"]) / 1e3)
                before_end.append((running[-1]["e"] - r["e"]) / 1e3)
            if nxt:
                lead.append((nxt[0]["s"] - r["e"]) / 1e3)
        print("carry kernel, %d dispatches among them: duration mean %.2f us, queue(s) %s" % (
            len(cc), mean([(r["e"] - r["s"]) / 1e3 for r in cc]), sorted(set(r.get("Queue_Id", "?") for r in cc))))
        if after_start:
            print("  started %.2f us (mean) after the start of the channel kernel running then, ended %.2f us before that kernel's end"
                  % (mean(after_start), mean(before_end)))
        if lead:
            print("  ended %.2f us (mean, min %.2f) before the next channel kernel started" % (mean(lead), min(lead)))


if __name__ == "__main__":
    main()
