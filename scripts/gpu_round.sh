R=$(cd "$(dirname "$0")/.." && pwd); cd $R; export OUT=${OUT:-$R/gpu_out}; mkdir -p $OUT
rocm-smi --showproductname 2>/dev/null | head -5 > $OUT/env.log
(timeout 1500 python -m pytest tests -m gpu -q -p no:cacheprovider 2>&1 | tail -150) > $OUT/test_gpu.log
echo "pytest done" >> $OUT/test_gpu.log
(timeout 300 python __graft_entry__.py smoke 2>&1 | tail -20) > $OUT/smoke.log
(timeout 600 python bench.py --full --steps 5 --warmup 2 2>&1 | tail -20) > $OUT/bench.log
cd /tmp && export TMPDIR=/tmp
(timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_r01 -o bench -- python $R/bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-roofline 2>&1 | tail -15) > $OUT/rocprof.log
ls -R $OUT/prof_r01 | head -30 >> $OUT/rocprof.log
cd $R
(timeout 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 1 --steps 3 --warmup 1 --no-cpu-baseline --no-roofline 2>&1 | tail -5) > $OUT/bench_torchrun.log
