set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/bench_out}; mkdir -p "$OUT"; export OUT=$(cd "$OUT" && pwd)
cd "$R"; export TMPDIR=/tmp; mkdir -p $OUT/chunk
for c in 100 25 10 4; do
  timeout -k 10 200 python -u bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --resident-chunk $c > $OUT/chunk/b$c.json 2> $OUT/chunk/b$c.err || exit 1
  python -c "import json;d=json.load(open('$OUT/chunk/b$c.json'));print($c, d['value'], d['stage_ms'])"
done
cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$OUT/chunk/prof10" -o run -- python "$R/bench.py" --steps 1 --warmup 1 --no-cpu-baseline --resident-chunk 10 > "$OUT/chunk/prof10.log" 2>&1
