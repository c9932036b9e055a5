#!/bin/bash
# round-2 GPU full session: full gpu tier, smoke, bench lines (cfg2/cfg4/cfg5, f32, torchrun), CLI smokes, profiles, PMC traffic
R=$(cd "$(dirname "$0")/.." && pwd); cd $R; export OUT=${OUT:-$R/gpu_out}; mkdir -p $OUT
(timeout 1700 python -m pytest tests -m gpu -q -rP -p no:cacheprovider 2>&1) > $OUT/k_test_full.log
grep -E "passed|failed|error|bf16 anchor:|cfg5 fused|LC gradients|resnet|Error|assert " $OUT/k_test_full.log | tail -60 > $OUT/k_test.log
(timeout 300 python __graft_entry__.py smoke 2>&1 | tail -3) > $OUT/k_smoke.log
(timeout 600 python bench.py --full 2>&1 | tail -2) > $OUT/k_bench_cfg2.log
(timeout 300 python bench.py --full --score-path fused --steps 100 --no-cpu-baseline 2>&1 | tail -2) > $OUT/k_bench_cfg2_fused.log
(timeout 300 python bench.py --full --no-graph --steps 100 --no-cpu-baseline 2>&1 | tail -2) > $OUT/k_bench_cfg2_nograph.log
(timeout 300 python bench.py --full --config cfg4 --steps 30 --warmup 3 --no-cpu-baseline 2>&1 | tail -2) > $OUT/k_bench_cfg4.log
(timeout 300 python bench.py --full --config cfg5 --steps 30 --warmup 3 --no-cpu-baseline 2>&1 | tail -2) > $OUT/k_bench_cfg5.log
(timeout 300 python bench.py --full --config cfg5 --score-path materialised --steps 30 --warmup 3 --no-cpu-baseline 2>&1 | tail -2) > $OUT/k_bench_cfg5_mat.log
(timeout 400 python bench.py --full --dtype f32 --steps 20 --warmup 2 --no-cpu-baseline 2>&1 | tail -2) > $OUT/k_bench_cfg2_f32.log
(timeout 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 1 --steps 100 --warmup 3 --no-cpu-baseline --no-roofline 2>&1 | tail -2) > $OUT/k_bench_torchrun.log
(timeout 300 python -m dpc_amd.main --net resnet18 --img_dim 128 --batch_size 32 --gpu 0 --epochs 1 --synthetic 6 --print_freq 2 --save_dir $OUT/ck_dpc 2>&1 | tail -8) > $OUT/k_main.log
(timeout 300 python -m dpc_amd.lc_main --net resnet18 --img_dim 128 --batch_size 16 --gpu 0 --epochs 1 --synthetic 6 --print_freq 2 --pretrain $OUT/ck_dpc/epoch1.pth.tar 2>&1 | tail -8) > $OUT/k_lc_main.log
rm -rf $OUT/ck_dpc
cd /tmp && export TMPDIR=/tmp
(timeout 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_r02k -o bench -- python $R/bench.py --no-graph --steps 3 --warmup 1 --no-cpu-baseline --no-roofline 2>&1 | tail -3) > $OUT/k_rocprof.log
(timeout 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_r02k_cfg4 -o bench -- python $R/bench.py --config cfg4 --no-graph --steps 2 --warmup 1 --no-cpu-baseline --no-roofline 2>&1 | tail -3) > $OUT/k_rocprof4.log
(timeout 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_r02k_cfg5 -o bench -- python $R/bench.py --config cfg5 --no-graph --steps 2 --warmup 1 --no-cpu-baseline --no-roofline 2>&1 | tail -3) > $OUT/k_rocprof5.log
cd $R
for d in prof_r02k prof_r02k_cfg4 prof_r02k_cfg5; do
  f=$(ls $OUT/$d/*.db 2>/dev/null | head -1)
  [ -n "$f" ] && python scripts/rocpd_stats.py $f > $OUT/${d}_stats.txt 2>&1
done
f=$(ls $OUT/prof_r02k/*.db 2>/dev/null | head -1); [ -n "$f" ] && python scripts/timeline.py $f "." > $OUT/prof_r02k_timeline.txt 2>&1
rm -rf $OUT/prof_r02k/*.db $OUT/prof_r02k_cfg4/*.db $OUT/prof_r02k_cfg5/*.db
PMC_TAG=r02 bash scripts/gpu_pmc_traffic.sh > $OUT/k_pmc_traffic.log 2>&1
cp profiles/r02_pmc_traffic.json $OUT/ 2>/dev/null
rm -rf $OUT/pmc_FETCH_SIZE/*.db $OUT/pmc_WRITE_SIZE/*.db
ls $OUT | head -80
