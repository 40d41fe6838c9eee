#!/bin/bash
# HBM bytes per kernel over a one-step bench run (FETCH_SIZE and WRITE_SIZE, one rocprofv3 pass each).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/bench_out}; mkdir -p "$OUT"; export OUT=$(cd "$OUT" && pwd)
cd "$R"
export TMPDIR=/tmp
TAG=${1:-hbm}
mkdir -p $OUT
for grp in "FETCH_SIZE" "WRITE_SIZE"; do
  (cd /tmp && timeout -s KILL 300 rocprofv3 --pmc $grp --output-format csv -d $OUT/pmc_${TAG}_$grp -o run -- python $R/bench.py --steps 1 --warmup 0 --no-cpu-baseline > $OUT/pmc_${TAG}_$grp.log 2>&1)
  rc=$?; echo "pmc $grp rc=$rc"; [ $rc -eq 0 ] || { tail -5 $OUT/pmc_${TAG}_$grp.log; exit $rc; }
  python $R/tools/pmc_summary.py $OUT/pmc_${TAG}_$grp > $OUT/pmc_${TAG}_$grp.txt
  rm -rf $OUT/pmc_${TAG}_$grp
done
