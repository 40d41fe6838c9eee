#!/bin/bash
# One extra PMC pass (LDS / VALU / wait counters) over a short bench run; per-kernel summary.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/bench_out}; mkdir -p "$OUT"; export OUT=$(cd "$OUT" && pwd)
cd "$R"
export TMPDIR=/tmp
TAG=${1:-r01}
grp="SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VALU SQ_WAIT_ANY SQ_INSTS_VMEM"
(cd /tmp && timeout -s KILL 300 rocprofv3 --pmc $grp --output-format csv -d $OUT/pmc_${TAG}_lds -o run -- python $R/bench.py --steps 1 --warmup 0 --no-cpu-baseline > $OUT/pmc_${TAG}_lds.log 2>&1)
rc=$?; echo "pmc lds rc=$rc"; [ $rc -eq 0 ] || { tail -5 $OUT/pmc_${TAG}_lds.log; exit $rc; }
python $R/tools/pmc_summary.py $OUT/pmc_${TAG}_lds > $OUT/pmc_${TAG}_lds.txt && rm -rf $OUT/pmc_${TAG}_lds
