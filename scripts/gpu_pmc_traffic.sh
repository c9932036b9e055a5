#!/bin/bash
# HBM traffic counters of one bench step (two separate --pmc passes: FETCH_SIZE and WRITE_SIZE do not fit one
# pass); summarised by scripts/pmc_traffic.py into profiles/<tag>_pmc_traffic.json
R=$(cd "$(dirname "$0")/.." && pwd); cd $R; export OUT=${OUT:-$R/gpu_out}; mkdir -p $OUT; rm -rf $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE
cd /tmp && export TMPDIR=/tmp
B="python $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-roofline --no-also --no-graph"
for c in FETCH_SIZE WRITE_SIZE; do
  (timeout 300 rocprofv3 --kernel-trace --pmc $c -d $OUT/pmc_$c -o pmc -- $B 2>&1 | tail -3) > $OUT/pmc_$c.log
done
cd $R; python scripts/pmc_traffic.py $OUT/pmc_FETCH_SIZE/*.db $OUT/pmc_WRITE_SIZE/*.db ${PMC_TAG:-r01}
