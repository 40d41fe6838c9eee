#!/bin/bash
# SIFT kernel A/B: per variant library (abvar/libgtsfm_hip_<v>.so) the C2 bench under rocprofv3 --stats (SIFT rows),
# then FETCH_SIZE per kernel for the variants named in FETCH_VARS.   tools/gpu_sift_ab.sh TAG v1 v2 ...
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/bench_out}; mkdir -p "$OUT"; export OUT=$(cd "$OUT" && pwd)
cd "$R"; export TMPDIR=/tmp
TAG=$1; shift
mkdir -p $OUT/sab_$TAG
for v in "$@"; do
  export GTSFM_HIP_LIB=$R/${ABDIR:-abvar}/libgtsfm_hip_$v.so
  (cd /tmp && timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/sab_$TAG/p_$v -o run -- python -u $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/sab_$TAG/$v.json 2> $OUT/sab_$TAG/$v.err)
  rc=$?; echo "== $v rc=$rc"; [ $rc -eq 0 ] || { tail -5 $OUT/sab_$TAG/$v.err; exit $rc; }
  python -c "import json,sys; d=json.load(open(sys.argv[1])); print(d['value'], d['stage_ms'])" $OUT/sab_$TAG/$v.json
  f=$(find $OUT/sab_$TAG/p_$v -name "*kernel_stats.csv" | head -1); python tools/kstats.py $f | grep -E "${KRE:-blur|extrema|orient|descr|topk|refine_k}" > $OUT/sab_$TAG/$v.k; cat $OUT/sab_$TAG/$v.k; rm -rf $OUT/sab_$TAG/p_$v
done
for v in $FETCH_VARS; do
  export GTSFM_HIP_LIB=$R/${ABDIR:-abvar}/libgtsfm_hip_$v.so
  (cd /tmp && timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/sab_$TAG/f_$v -o run -- python $R/bench.py --steps 1 --warmup 0 --no-cpu-baseline > $OUT/sab_$TAG/f_$v.log 2>&1)
  rc=$?; echo "== fetch $v rc=$rc"; [ $rc -eq 0 ] || { tail -5 $OUT/sab_$TAG/f_$v.log; exit $rc; }
  python tools/pmc_summary.py $OUT/sab_$TAG/f_$v | grep -E "blur|extrema|orient|descr" > $OUT/sab_$TAG/f_$v.txt; cat $OUT/sab_$TAG/f_$v.txt; rm -rf $OUT/sab_$TAG/f_$v
done
