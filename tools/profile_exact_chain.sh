#!/bin/bash
# rocprofv3 evidence for exact search along the sample chain on the headline record, in the pattern of tools/profile_exact_plain.sh: one --kernel-trace --stats pass, then the
# L2 / fabric counters in --pmc passes of their own (never combined with tracing), every k_exact_* kernel summarised by tools/rocprof_kernels_summary.py.
# usage: tools/profile_exact_chain.sh <tree whose bench.py and library are profiled> <output dir>
set -o pipefail
T=$(cd "$1" && pwd)
S=$(cd "$(dirname "$0")" && pwd)
OUT=$(mkdir -p "$2" && cd "$2" && pwd)
export TMPDIR=/tmp
B="python3 $T/bench.py --gpus 1 --steps 5 --warmup 1"
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- $B > $OUT/trace.log 2>&1 &&
timeout -k 10 300 rocprofv3 --pmc TCC_EA0_RDREQ_sum TCC_HIT_sum TCC_MISS_sum --output-format csv -d $OUT/pmc_tcc -- $B > $OUT/pmc_tcc.log 2>&1 &&
timeout -k 10 300 rocprofv3 --pmc TCP_TCC_READ_REQ_sum --output-format csv -d $OUT/pmc_tcp -- $B > $OUT/pmc_tcp.log 2>&1
rc=$?
python3 $S/rocprof_kernels_summary.py $OUT k_exact $OUT/summary.json > $OUT/summary.log 2>&1
find $OUT -type f \( -name "*.db" -o -name "*_kernel_trace.csv" -o -name "*agent_info.csv" -o -name "*_counter_collection.csv" \) -delete
exit $rc
