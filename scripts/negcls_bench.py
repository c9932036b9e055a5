#!/usr/bin/env python
"""Times dpc_ce_topk_cls / dpc_ce_topk_bf16_cls (csrc/loss_cls.hip) singly beside their siblings dpc_ce_topk / dpc_ce_topk_bf16: the same
logits, the same gradient buffer, weights (1, 1, 1), (0.5, 2, 0.25) and the latter with the report.  HIP events around each call (row
kernel + finalize, and the report's means where they are on), the median of 50 calls, two rounds with the arms alternating in one
process.  Prints one line per arm and round, then one JSON line.

    python scripts/negcls_bench.py [--geom 128 3 16] [--reps 50] [--rounds 2]
"""
import argparse
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
    ap.add_argument("--geom", type=int, nargs=3, default=[128, 3, 16], metavar=("B", "P", "SQ"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    lib = L.load_hip()
    dev = torch.device("cuda", 0)
    B, P, SQ = args.geom
    R = B * P * SQ
    bf, f32 = torch.bfloat16, torch.float32
    gen = torch.Generator(dev).manual_seed(1)
    s32 = 4.0 * torch.randn((R, R), device=dev, generator=gen)
    s16 = s32.to(bf)
    d16 = torch.empty((R, R), dtype=bf, device=dev)
    row_ws, res = torch.empty((R, 2), dtype=f32, device=dev), torch.empty(4, dtype=f32, device=dev)
    rrows, rep = torch.empty((R, 8), dtype=f32, device=dev), torch.empty(8, dtype=f32, device=dev)
    st = lambda: lib.stream()   # noqa: E731
    desc = lambda w: L.NegClasses(B, P, SQ, 0, w[0], w[1], w[2], 0.0)   # noqa: E731
    ones, wts = desc((1.0, 1.0, 1.0)), desc((0.5, 2.0, 0.25))
    arms = {
        "bf16 logits: dpc_ce_topk_bf16": lambda: lib.call("dpc_ce_topk_bf16", s16, R, R, R, row_ws, res, d16, R, st()),
        "bf16 logits: _cls (1,1,1)": lambda: lib.call("dpc_ce_topk_bf16_cls", s16, R, R, R, row_ws, res, d16, R, None, None, ones, None, None, st()),
        "bf16 logits: _cls (0.5,2,0.25)": lambda: lib.call("dpc_ce_topk_bf16_cls", s16, R, R, R, row_ws, res, d16, R, None, None, wts, None, None, st()),
        "bf16 logits: _cls weights + report": lambda: lib.call("dpc_ce_topk_bf16_cls", s16, R, R, R, row_ws, res, d16, R, None, None, wts, rrows, rep, st()),
        "f32 logits: dpc_ce_topk": lambda: lib.call("dpc_ce_topk", s32, R, R, R, row_ws, res, d16, L.BF16, R, st()),
        "f32 logits: _cls (1,1,1)": lambda: lib.call("dpc_ce_topk_cls", s32, R, R, R, row_ws, res, d16, L.BF16, R, None, None, ones, None, None, st()),
        "f32 logits: _cls (0.5,2,0.25)": lambda: lib.call("dpc_ce_topk_cls", s32, R, R, R, row_ws, res, d16, L.BF16, R, None, None, wts, None, None, st()),
        "f32 logits: _cls weights + report": lambda: lib.call("dpc_ce_topk_cls", s32, R, R, R, row_ws, res, d16, L.BF16, R, None, None, wts, rrows, rep, st()),
    }
    out = {name: [] for name in arms}
    for rnd in range(args.rounds):
        for name, fn in arms.items():
            us = median_us(fn, args.reps)
            out[name].append(round(us, 1))
            print(f"round {rnd}  {name:36s} {us:9.1f} us", flush=True)
    print(json.dumps({"geom": [B, P, SQ], "R": R, "reps": args.reps, "median_us": out}))


if __name__ == "__main__":
    main()
