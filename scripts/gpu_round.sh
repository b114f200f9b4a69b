#!/bin/bash
# One GPU-box session: parity tests, bench lines, rocprof kernel stats.  Usage: scripts/gpu_round.sh <tag> [skip_tests]
set -o pipefail
TAG=${1:-r1}
: "${OUT:?set OUT to the directory the results go to}"; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
cd "$(dirname "$0")/.."
R=$(pwd)
export TMPDIR=/tmp
if [ "$2" != "skip_tests" ]; then
  timeout -k 10 700 python -m pytest tests -m gpu -q -p no:cacheprovider --timeout=300 > $OUT/pytest_gpu_$TAG.log 2>&1
  echo "pytest exit=$?" | tee -a $OUT/pytest_gpu_$TAG.log
  tail -3 $OUT/pytest_gpu_$TAG.log
fi
timeout -k 10 300 python bench.py --config cfg2 --steps 3 --warmup 1 --no-cpu-baseline > $OUT/bench_cfg2_$TAG.json 2> $OUT/bench_cfg2_$TAG.err || { echo "bench cfg2 failed"; tail -5 $OUT/bench_cfg2_$TAG.err; }
cat $OUT/bench_cfg2_$TAG.json
timeout -k 10 600 python bench.py --config cfg3 --steps 3 --warmup 1 --full > $OUT/bench_cfg3_$TAG.json 2> $OUT/bench_cfg3_$TAG.err || { echo "bench cfg3 failed"; tail -5 $OUT/bench_cfg3_$TAG.err; }
cat $OUT/bench_cfg3_$TAG.json
timeout -k 10 300 python scripts/microbench.py > $OUT/microbench_$TAG.json 2> $OUT/microbench_$TAG.err; cat $OUT/microbench_$TAG.json | tr -d "\n" | cut -c1-3000; echo
cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o cfg3 -- python3 $R/bench.py --config cfg3 --steps 2 --warmup 1 --no-cpu-baseline > $OUT/prof_$TAG.log 2>&1
echo "rocprof exit=$?"
cd $R && find $OUT/prof_$TAG -name "*stats*" | head; find $OUT/prof_$TAG -name "*kernel_stats*" -exec head -25 {} \;
# keep the merge-back small: drop the per-dispatch trace, keep the stats
find $OUT/prof_$TAG -name "*kernel_trace*" -size +20M -delete
