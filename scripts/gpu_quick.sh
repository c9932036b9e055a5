#!/bin/bash
# quick check after a kernel change: kernel tests (KEXPR), config tests, one cfg2 bench line, kernel stats of 4 steps
R=$(cd "$(dirname "$0")/.." && pwd); cd $R; export OUT=${OUT:-$R/gpu_out}; mkdir -p $OUT
(timeout 900 python -m pytest tests/test_kernels_gpu.py -m gpu -q -p no:cacheprovider -k "${KEXPR:-conv or gemm or wgrad}" 2>&1 | tail -3) > $OUT/q_tests.log
(timeout 900 python -m pytest tests/test_configs_gpu.py tests/test_engine_gpu.py -m gpu -q -p no:cacheprovider 2>&1 | tail -3) >> $OUT/q_tests.log
(timeout 300 python bench.py --full --no-cpu-baseline 2>&1 | tail -1) > $OUT/q_bench_cfg2.log
cd /tmp && export TMPDIR=/tmp
(timeout 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_q -o bench -- python $R/bench.py --no-graph --steps 3 --warmup 1 --no-cpu-baseline --no-roofline 2>&1 | tail -3) > $OUT/q_rocprof.log
cd $R
f=$(ls $OUT/prof_q/*.db 2>/dev/null | head -1)
[ -n "$f" ] && python scripts/rocpd_stats.py $f > $OUT/prof_q_stats.txt 2>&1
rm -rf $OUT/prof_q/*.db
cat $OUT/q_tests.log; python -c "import json,sys; d=json.loads(open('$OUT/q_bench_cfg2.log').read().strip().splitlines()[-1]); print('cfg2', d['value'], d['ms_per_step'], d['roofline']['frac'], d['wgrad_kernel'])"; grep -E "${KGREP:-igemm|wgrad}" $OUT/prof_q_stats.txt
