#!/bin/bash
# One GPU call: the GPU test suite, one bench line, and the rocprofv3 kernel stats of the same bench command.
#   tools/gpu_check.sh TAG [bench args...]      (writes $OUT/*_TAG*)
# Every GPU step has its own time limit and the call stops at the first failing step.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/bench_out}; mkdir -p "$OUT"; export OUT=$(cd "$OUT" && pwd)
cd "$R"
export TMPDIR=/tmp
TAG=${1:-r02}
shift
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu --maxfail=5 -v --timeout 240 --timeout-method thread \
    > $OUT/pytest_${TAG}.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -4 $OUT/pytest_${TAG}.log; [ $rc -eq 0 ] || { grep -E "FAIL|Error|error" $OUT/pytest_${TAG}.log | head -20; exit $rc; }
timeout -k 10 300 python -u __graft_entry__.py smoke > $OUT/smoke_${TAG}.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -2 $OUT/smoke_${TAG}.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python -u bench.py --full "$@" > $OUT/bench_${TAG}.json 2> $OUT/bench_${TAG}.err
rc=$?; echo "bench rc=$rc"; cat $OUT/bench_${TAG}.json; [ $rc -eq 0 ] || { tail -20 $OUT/bench_${TAG}.err; exit $rc; }
cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_${TAG}" \
    -o run -- python "$R/bench.py" --steps 2 --warmup 1 --no-cpu-baseline "$@" \
    > "$OUT/prof_${TAG}.log" 2>&1
rc=$?; echo "prof rc=$rc"; [ $rc -eq 0 ] || exit $rc
cd "$R" && python tools/kstats.py "$(find $OUT/prof_${TAG} -name "*kernel_stats.csv" | sort | tail -n 1)"
exit 0
