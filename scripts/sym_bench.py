#!/usr/bin/env python
"""Times dpc_ce_topk_bf16_sym (csrc/loss_sym.hip) singly beside its sibling dpc_ce_topk_bf16, and the column pass alone (dpc_ce_colpass)
with its effective bytes per second: the same bf16 logits, the same gradient buffer, W = 0.5.  HIP events around each call, the median of
50 calls after a warm-up, two rounds with the arms alternating in one process.  Prints one line per arm and round, then one JSON line.

    python scripts/sym_bench.py [--R 6144 15680] [--reps 50] [--rounds 2]
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
    ap.add_argument("--R", type=int, nargs="+", default=[6144, 15680])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    lib = L.load_hip()
    dev = torch.device("cuda", 0)
    bf, f32 = torch.bfloat16, torch.float32
    st = lambda: lib.stream()   # noqa: E731
    result = {}
    for R in args.R:
        gen = torch.Generator(dev).manual_seed(1)
        s16 = (4.0 * torch.randn((R, R), device=dev, generator=gen)).to(bf)
        d16 = torch.empty((R, R), dtype=bf, device=dev)
        row_ws, res = torch.empty((R, 2), dtype=f32, device=dev), torch.empty(4, dtype=f32, device=dev)
        nf = C.c_int64(0)
        slabs = lib.call("dpc_ce_sym_ws_floats", R, 0, C.byref(nf))
        cl, cw = torch.empty(R, dtype=f32, device=dev), torch.empty((R, 2), dtype=f32, device=dev)
        ws, sr = torch.empty(nf.value, dtype=f32, device=dev), torch.empty(8, dtype=f32, device=dev)
        arms = {
            "dpc_ce_topk_bf16": lambda: lib.call("dpc_ce_topk_bf16", s16, R, R, R, row_ws, res, d16, R, st()),
            "dpc_ce_topk_bf16_sym W 0.5": lambda: lib.call("dpc_ce_topk_bf16_sym", s16, R, R, R, row_ws, res, d16, R, None, None, 0.5, 0, cl, cw, ws, sr, st()),
            "dpc_ce_colpass": lambda: lib.call("dpc_ce_colpass", s16, L.BF16, R, R, 1, 0, cl, cw, ws, st()),
        }
        out = {name: [] for name in arms}
        for rnd in range(args.rounds):
            for name, fn in arms.items():
                us = median_us(fn, args.reps)
                out[name].append(round(us, 1))
                rate = f"  {2.0 * R * R / us / 1e6:6.2f} TB/s of logits" if name == "dpc_ce_colpass" else ""
                print(f"R {R:6d} round {rnd}  {name:30s} {us:9.1f} us{rate}", flush=True)
        result[str(R)] = {"slabs": slabs, "median_us": out, "colpass_TBps": [round(2.0 * R * R / us / 1e6, 2) for us in out["dpc_ce_colpass"]]}
    print(json.dumps({"reps": args.reps, "R": result}))


if __name__ == "__main__":
    main()
