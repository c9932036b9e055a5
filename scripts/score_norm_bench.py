#!/usr/bin/env python
"""Times the cosine score's two kernels singly (csrc/score_norm.hip: dpc_rownorm_fwd, dpc_rownorm_bwd, both operands in one launch) at
one R and D in bf16, beside dpc_transpose2d_bf16x2 on the same operands -- the sibling of the same bytes class -- and beside the
project's launch floor, the one-thread dpc_step_advance_sched.  HIP events around each launch, the median of 50 launches, two rounds
with the arms alternating in one process.  Prints one line per arm and round, then one JSON line.

    python scripts/score_norm_bench.py [--R 6144] [--D 256] [--temperature 0.07] [--reps 50] [--rounds 2]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpc_amd import _lib as L  # noqa: E402


def median_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(1e3 * a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=6144)
    ap.add_argument("--D", type=int, default=256)
    ap.add_argument("--temperature", type=float, default=0.07)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    lib = L.load_hip()
    dev = torch.device("cuda", 0)
    R, D = args.R, args.D
    bf, f32 = torch.bfloat16, torch.float32
    gen = torch.Generator(dev).manual_seed(1)
    pred = torch.randn((R, D), device=dev, generator=gen).to(bf)
    finf = torch.randn((R, D), device=dev, generator=gen).to(bf)
    pred_n, finf_n = torch.empty_like(pred), torch.empty_like(finf)
    rnorm = torch.empty(2 * R, dtype=f32, device=dev)
    d_pred = torch.randn((R, D), device=dev, generator=gen)
    d_finf = torch.randn((R, D), device=dev, generator=gen)
    ldT = (R + 7) // 8 * 8
    predT, finfT = torch.zeros((D, ldT), dtype=bf, device=dev), torch.zeros((D, ldT), dtype=bf, device=dev)
    step, bc = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(2, dtype=f32, device=dev)
    lr_state = torch.zeros(4, dtype=torch.int32, device=dev)
    sched = L.LrSchedule(kind=L.LR_CONSTANT)
    scale = 1.0 / args.temperature
    st = lambda: lib.stream()   # noqa: E731
    arms = {
        "dpc_step_advance_sched (floor)": lambda: lib.call("dpc_step_advance_sched", step, bc, 0.9, 0.999, None, C.byref(sched), lr_state, st()),
        "dpc_transpose2d_bf16x2": lambda: lib.call("dpc_transpose2d_bf16x2", finf, pred, D, finfT, predT, ldT, R, D, st()),
        "dpc_rownorm_fwd": lambda: lib.call("dpc_rownorm_fwd", pred, finf, pred_n, finf_n, rnorm, R, D, L.BF16, scale, 1.0, 1e-12, st()),
        # in place: the gradients shrink or grow by 1 / (T |x|) per launch; the time does not depend on the values
        "dpc_rownorm_bwd": lambda: lib.call("dpc_rownorm_bwd", pred, finf, rnorm, d_pred, d_finf, R, D, L.BF16, 1.0, 1.0, 1e-12, st()),
    }
    arms["dpc_rownorm_fwd"]()
    out = {name: [] for name in arms}
    for rnd in range(args.rounds):
        for name, fn in arms.items():
            us = median_us(fn, args.reps)
            out[name].append(round(us, 1))
            print(f"round {rnd}  {name:32s} {us:9.1f} us", flush=True)
    mb = {"dpc_rownorm_fwd": (4 * R * D * 2 + 8 * R) / 1e6, "dpc_rownorm_bwd": (2 * R * D * 2 + 4 * R * D * 4 + 8 * R) / 1e6,
          "dpc_transpose2d_bf16x2": 4 * R * D * 2 / 1e6}
    print(json.dumps({"R": R, "D": D, "reps": args.reps, "megabytes": {k: round(v, 1) for k, v in mb.items()}, "median_us": out}))


if __name__ == "__main__":
    main()
