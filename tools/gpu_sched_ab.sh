set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/bench_out}; mkdir -p "$OUT"; export OUT=$(cd "$OUT" && pwd)
cd "$R"; export TMPDIR=/tmp; mkdir -p $OUT/sched
for v in s2 s4 s8; do
  for r in 0 7; do
    GTSFM_HIP_LIB=$R/abvar/libgtsfm_hip_$v.so timeout -k 10 300 python -u bench.py --full --emulate-world 8 --emulate-rank $r --steps 5 --warmup 2 --no-cpu-baseline > $OUT/sched/${v}_r$r.json 2> $OUT/sched/${v}_r$r.err || { tail -5 $OUT/sched/${v}_r$r.err; exit 1; }
    python -c "import json,sys; d=json.load(open(sys.argv[1])); print('$v r$r', d['ms_per_step'], d['stage_ms'])" $OUT/sched/${v}_r$r.json
  done
done
