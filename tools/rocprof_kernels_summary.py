#!/usr/bin/env python3
"""rocprof_kernels_summary.py DIR SUBSTRING OUT.json — like rocprof_summary.py, for a search that takes several kernels: every kernel whose name holds SUBSTRING, each with its
--kernel-trace --stats row (calls, mean ms) and, per --pmc pass, every counter per launch; `per_search` adds them up (each of the kernels runs once per search call).
Expects the layout tools/profile_exact_chain.sh writes: DIR/trace, DIR/pmc_<name>."""
import csv
import glob
import json
import os
import re
import sys
from collections import defaultdict


def files(root, suffix):
    return sorted(glob.glob(os.path.join(root, "**", "*" + suffix), recursive=True))


def short(name):
    m = re.search(r"(k_\w+)<[^,>]*(?:, (\w+))?>", name)       # (k_exact_p<Q, 1> -> k_exact_p<1>, k_exact_chain<Q, true> -> k_exact_chain<true>: its list form)
    return (m.group(1) + ("<%s>" % m.group(2) if m.group(2) else "")) if m else name.split("(")[0]


def main(d, sub, out):
    res = {"dir": os.path.basename(os.path.normpath(d)), "kernels": defaultdict(dict), "per_search": defaultdict(float)}
    for f in files(os.path.join(d, "trace"), "_kernel_stats.csv"):
        for row in csv.DictReader(open(f)):
            if sub in row["Name"]:
                res["kernels"][short(row["Name"])].update({"calls": int(row["Calls"]), "mean_ms": float(row["AverageNs"]) / 1e6, "min_ms": float(row["MinNs"]) / 1e6, "max_ms": float(row["MaxNs"]) / 1e6})
    for p in sorted(glob.glob(os.path.join(d, "pmc_*"))):
        per = defaultdict(lambda: defaultdict(lambda: defaultdict(float)))          # kernel -> counter -> dispatch -> value
        for f in files(p, "_counter_collection.csv"):
            for row in csv.DictReader(open(f)):
                if sub in row["Kernel_Name"]:
                    per[short(row["Kernel_Name"])][row["Counter_Name"]][row["Dispatch_Id"]] += float(row["Counter_Value"])
        for k, counters in per.items():
            for name, by in counters.items():
                res["kernels"][k][name] = sum(by.values()) / len(by)
    for k, v in res["kernels"].items():
        for name, val in v.items():
            if name not in ("calls", "min_ms", "max_ms"):
                res["per_search"][name] += val
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res)[:3000])


if __name__ == "__main__":
    main(*sys.argv[1:4])
