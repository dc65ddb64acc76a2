#!/bin/bash
# Selected GPU tests (-k $2) + short bench + kernel-trace profile.  Test tooling.
# Logs go to $OUT (default ./bench_out).
TAG=${1:-q}
OUT=${OUT:-$PWD/bench_out}
export TMPDIR=/tmp
mkdir -p "$OUT"
timeout -k 10 300 python -u -m pytest tests -m gpu -k "$2" -v --timeout 120 --timeout-method thread -p no:cacheprovider > "$OUT/qtests_$TAG.log" 2>&1
rc=$?; echo "tests_rc=$rc"; grep -E "passed|failed" "$OUT/qtests_$TAG.log" | tail -2; [ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline > "$OUT/qbench_$TAG.log" 2>&1
rc=$?; echo "bench_rc=$rc"; tail -1 "$OUT/qbench_$TAG.log" | cut -c1-200; [ $rc -ne 0 ] && exit $rc
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$TAG" -o run \
  --output-format csv -- python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > "$OUT/prof_$TAG.log" 2>&1
echo "prof_rc=$?"
