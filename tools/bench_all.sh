#!/bin/bash
# every BASELINE workload's full bench line on one box (each run under its own limit; stop at the first fault)
# usage: bash tools/bench_all.sh TAG [workload ...]   (logs and lines under $OUT, default bench_out/)
set -u
TAG=$1; shift
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for w in "$@"; do
  timeout -k 10 400 python bench.py --full --workload $w --steps 20 --warmup 3 > "$OUT/bench_${TAG}_$w.log" 2>&1
  rc=$?
  echo "$w rc=$rc"
  [ $rc -ne 0 ] && exit $rc
  grep '^{' "$OUT/bench_${TAG}_$w.log" > "$OUT/bench_${TAG}_$w.jsonl"
done
exit 0
