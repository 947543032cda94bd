#!/bin/bash
# rocprofv3 evidence for the headline record (genome/exact/plain, k_exact_p) of the tree this script lives in: one --kernel-trace --stats pass, then the L2 / fabric
# counters in --pmc passes of their own (never combined with tracing), summarised by tools/rocprof_summary.py.
# usage: tools/profile_exact_plain.sh <output dir>
set -o pipefail
T=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "$1" && cd "$1" && pwd)
export TMPDIR=/tmp FMGPU_BENCH_RECORDS=$OUT/bench_records.json
B="python3 $T/bench.py --full --texts genome --no-protein --no-cpu-baseline --only genome/exact/plain --steps 5 --warmup 1"
cd /tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- $B > $OUT/trace.log 2>&1 &&
timeout -k 10 400 rocprofv3 --pmc TCC_EA0_RDREQ_sum TCC_HIT_sum TCC_MISS_sum --output-format csv -d $OUT/pmc_tcc -- $B > $OUT/pmc_tcc.log 2>&1 &&
timeout -k 10 400 rocprofv3 --pmc TCP_TCC_READ_REQ_sum TCC_REQ_sum --output-format csv -d $OUT/pmc_tcp -- $B > $OUT/pmc_tcp.log 2>&1 &&
timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -- $B > $OUT/pmc_fetch.log 2>&1
rc=$?
python3 $T/tools/rocprof_summary.py $OUT k_exact_p $OUT/summary.json > $OUT/summary.log 2>&1
find $OUT -type f \( -name "*.db" -o -name "*_kernel_trace.csv" -o -name "*agent_info.csv" \) -delete
exit $rc
