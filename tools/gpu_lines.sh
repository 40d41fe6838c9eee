#!/bin/bash
# The other BASELINE configs' bench lines with their CPU baselines.   tools/gpu_lines.sh TAG cfg...
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/bench_out}; mkdir -p "$OUT"; export OUT=$(cd "$OUT" && pwd)
cd "$R"; mkdir -p $OUT; export TMPDIR=/tmp
TAG=$1; shift
for cfg in "$@"; do
  timeout -k 10 600 python -u bench.py --full --config $cfg > $OUT/bench_${TAG}_$cfg.json 2> $OUT/bench_${TAG}_$cfg.err
  rc=$?; echo "$cfg rc=$rc"; cut -c1-300 $OUT/bench_${TAG}_$cfg.json; [ $rc -eq 0 ] || { tail -20 $OUT/bench_${TAG}_$cfg.err; exit $rc; }
done
