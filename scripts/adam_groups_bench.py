#!/usr/bin/env python
"""The grouped Adam kernel against dpc_adam_dev over the r18 LC arena, and the LC step time with a frozen extractor, on the MI355X.

    python scripts/adam_groups_bench.py [--iters 50] [--rounds 5] [--batch 32] [--steps 10]

Part 1 (the mechanism of scripts/elt_bench.py: HIP events around --iters launches through the C ABI, --rounds rounds in one process,
so the spread is the session's own): dpc_adam_dev; dpc_adam_groups_dev with one segment, with one segment per parameter (alternating
lr so that nothing merges), and with the head's parameters only.  Part 2: LCEngine.train_step at r18 / 128 px / bf16 on one fixed
batch, --steps steps after 3 warm-up steps, wall clock between device synchronisations: all parameters (dpc_adam_dev) against
`head` (set_param_groups over final_bn / final_fc: the backward stops in front of the ConvGRU), and the train-mode forward alone.
(dpc_amd.lc_main prints no per-step time; this is its train step.)  docs/kernels.md and docs/design_parts/10_beyond.md quote the output."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpc_amd.lc import LC, LCEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--steps", type=int, default=10)
a = ap.parse_args()
dev = "cuda:0"
eng = LCEngine("resnet18", 128, 8, 5, a.batch, dev, torch.bfloat16, num_class=101)
eng.load_params({k: v.detach() for k, v in LC(128, 8, 5, "resnet18", 0.5, 101, seed=0).state_dict().items()})
eng.flat_g.normal_()
names = list(eng.offsets)
head = [k for k in names if k.startswith(("final_bn.", "final_fc."))]
print(f"arena {eng.numel} floats, {len(names)} parameters, head {sum(eng.offsets[k][1] for k in head)} floats", flush=True)
eng.call("dpc_step_advance", eng.dev_step, eng.dev_bc, 0.9, 0.999)

def timed(fn, iters=a.iters):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3   # us

def plain():
    eng.call("dpc_adam_dev", eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v, eng.numel, 1e-4, 0.9, 0.999, 1e-8, 1e-3, eng.dev_bc, 1.0)
def grouped():
    eng.call("dpc_adam_groups_dev", eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v, eng.numel, eng._seg_dev, eng._seg_n, 0.9, 0.999, 1e-8, eng.dev_bc, 1.0)
cases = [("dpc_adam_dev", None),
         ("groups: one segment", [{"params": names, "lr": 1e-4, "weight_decay": 1e-3}]),
         ("groups: per parameter", [{"params": [k], "lr": 1e-4 * (1 + i % 2), "weight_decay": 1e-3} for i, k in enumerate(names)]),
         ("groups: head only", [{"params": head, "lr": 1e-4, "weight_decay": 1e-3}])]
res = {n: [] for n, _ in cases}
for rnd in range(a.rounds):
    for n, g in cases:
        if g is None:
            res[n].append(timed(plain))
        else:
            eng.set_param_groups(g)
            res[n].append(timed(grouped))
for n, _ in cases:
    v = res[n]
    print(f"ADAM {n}: us per launch " + " ".join(f"{x:.1f}" for x in v) + f"  (min {min(v):.1f} max {max(v):.1f})", flush=True)
bytes_moved = eng.numel * 4 * 7
print(f"ADAM bytes per full update {bytes_moved / 1e6:.1f} MB", flush=True)

# ---- step time: --train_what all (one group) against head, engine-owned train_step as lc_main runs it
gen = torch.Generator(dev).manual_seed(1000)
x = torch.randn((a.batch, 8, 3, 5, 128, 128), device=dev, generator=gen)
y = torch.randint(0, 101, (a.batch,), device=dev, generator=gen)
def step_ms(n=a.steps):
    for _ in range(3):
        eng.train_step(x, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        eng.train_step(x, y)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3
for rnd in range(2):
    eng.set_param_groups(None)
    t_all = step_ms()
    eng.set_param_groups([{"params": head, "lr": 1e-3, "weight_decay": 1e-3}])
    h = step_ms()
    print(f"STEP r18/128/B={a.batch} bf16: all {t_all:.2f} ms, head {h:.2f} ms", flush=True)
eng.set_param_groups(None)
def fwd_ms(n=a.steps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n):
        eng.forward(x, y, train=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3
print(f"STEP forward only {fwd_ms():.2f} ms", flush=True)
