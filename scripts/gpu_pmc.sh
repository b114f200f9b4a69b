#!/bin/bash
# HBM traffic of one bench step from the TCC counters (separate --pmc passes, kernel-trace only, as the guide prescribes).
TAG=${1:-r1}
CFG=${2:-cfg3}
export TMPDIR=/tmp
R=$(cd "$(dirname "$0")/.." && pwd)
: "${OUT:?set OUT to the directory the results go to}"; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
cd /tmp
for C in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 500 rocprofv3 --pmc $C --kernel-trace --output-format csv -d $OUT/pmc_${TAG}_$C -o $CFG -- python3 $R/bench.py --config $CFG --steps 1 --warmup 0 --no-cpu-baseline > $OUT/pmc_${TAG}_$C.log 2>&1
  echo "$C exit=$?"
done
cd $R
ls -la $OUT/pmc_${TAG}_FETCH_SIZE/ | head
python3 scripts/pmc_traffic.py $OUT/pmc_${TAG}_FETCH_SIZE $OUT/pmc_${TAG}_WRITE_SIZE $CFG > $OUT/pmc_${TAG}_traffic.json && cat $OUT/pmc_${TAG}_traffic.json
# keep only the per-kernel aggregate (the per-dispatch CSVs are large)
find $OUT/pmc_${TAG}_FETCH_SIZE $OUT/pmc_${TAG}_WRITE_SIZE -name "*.csv" -size +8M -delete
