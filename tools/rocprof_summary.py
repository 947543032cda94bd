#!/usr/bin/env python3
"""rocprof_summary.py DIR KERNEL OUT.json — one kernel's evidence from a rocprofv3 run directory: the --kernel-trace --stats table (calls, mean duration) and,
per --pmc pass, every counter summed over the kernel's dispatches and divided by their number (per launch).  Expects the layout tools/profile_exact_plain.sh writes:
DIR/trace/... *_kernel_stats.csv, DIR/pmc_<name>/... *_counter_collection.csv, DIR/trace.log (the bench line is its last JSON line)."""
import csv
import glob
import json
import os
import sys
from collections import defaultdict


def files(root, suffix):
    return sorted(glob.glob(os.path.join(root, "**", "*" + suffix), recursive=True))


def main(d, kernel, out):
    res = {"kernel": kernel, "dir": os.path.basename(os.path.normpath(d)), "kernel_stats": None, "counters_per_launch": {}, "launches": {}}
    for f in files(os.path.join(d, "trace"), "_kernel_stats.csv"):
        for row in csv.DictReader(open(f)):
            if kernel in row["Name"]:
                res["kernel_stats"] = {"calls": int(row["Calls"]), "mean_ms": float(row["AverageNs"]) / 1e6, "min_ms": float(row["MinNs"]) / 1e6, "max_ms": float(row["MaxNs"]) / 1e6}
    for p in sorted(glob.glob(os.path.join(d, "pmc_*"))):
        per = defaultdict(lambda: defaultdict(float))               # counter -> dispatch -> value
        for f in files(p, "_counter_collection.csv"):
            for row in csv.DictReader(open(f)):
                if kernel in row["Kernel_Name"]:
                    per[row["Counter_Name"]][row["Dispatch_Id"]] += float(row["Counter_Value"])
        for name, by in per.items():
            res["counters_per_launch"][name] = sum(by.values()) / len(by)
            res["launches"][name] = len(by)
    log = os.path.join(d, "trace.log")
    if os.path.exists(log):
        lines = [ln for ln in open(log) if ln.startswith("{") and '"metric"' in ln]
        if lines:
            b = json.loads(lines[-1])
            res["bench_line"] = {k: b.get(k) for k in ("ms_per_step",)}
            res["bench_line"]["roofline"] = {k: b.get("roofline", {}).get(k) for k in ("kernel", "kernel_ms", "units_per_launch")}
    rec = os.path.join(d, "bench_records.json")
    if os.path.exists(rec):
        recs = json.load(open(rec))
        recs = recs.get("records", recs) if isinstance(recs, dict) else recs
        for r in recs if isinstance(recs, list) else []:
            if isinstance(r, dict) and r.get("id") == "genome/exact/plain":
                rf = r.get("roofline", {})
                res["record"] = {"kernel_ms": rf.get("kernel_ms"), "lf_steps_per_launch": rf.get("units_per_launch"),
                                 "loaded": rf.get("loaded"), "clocks": r.get("clocks")}
    c = res["counters_per_launch"]
    if "TCC_EA0_RDREQ_sum" in c and res["kernel_stats"]:
        res["fabric_read_requests_per_s"] = c["TCC_EA0_RDREQ_sum"] / (res["kernel_stats"]["mean_ms"] * 1e-3)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res)[:2000])


if __name__ == "__main__":
    main(*sys.argv[1:4])
