#!/bin/bash
# Distance-GEMM microbench + its rocprofv3 kernel stats. Usage: gpu_matchbench.sh TAG
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/bench_out}; mkdir -p "$OUT"; export OUT=$(cd "$OUT" && pwd)
cd "$R"
mkdir -p $OUT
export TMPDIR=/tmp
TAG=${1:-mb}
timeout -k 10 120 python -u tools/matchbench.py 100 > $OUT/matchbench_${TAG}.json 2>$OUT/matchbench_${TAG}.err
rc=$?; cat $OUT/matchbench_${TAG}.json; [ $rc -eq 0 ] || { tail $OUT/matchbench_${TAG}.err; exit $rc; }
timeout -k 10 180 rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG} -o run -- python3 tools/matchbench.py 100 \
    > $OUT/prof_${TAG}.log 2>&1
rc=$?; f=$(find $OUT/prof_${TAG} -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -8 "$f"; exit $rc
