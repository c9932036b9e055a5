#!/usr/bin/env python
"""Times the negative queue's kernels singly (csrc/neg_queue.hip) beside their in-batch siblings of csrc/score_fused.hip, which run the
same contraction per slot: dpc_negq_fwd against dpc_score_fwd, dpc_negq_bwd against dpc_score_bwd(by_owner = 1), at one R and D and a
full bank of K = 1, 4, 8 slots.  HIP events around each launch, the median of 50 launches, two rounds with the arms alternating in one
process.  Prints one line per arm and round, then one JSON line.

    python scripts/negq_bench.py [--R 6144] [--D 256] [--slots 1 4 8] [--reps 50] [--rounds 2]
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
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    lib = L.load_hip()
    dev = torch.device("cuda", 0)
    R, D = args.R, args.D
    bf, f32 = torch.bfloat16, torch.float32
    gen = torch.Generator(dev).manual_seed(1)
    pred = (0.05 * torch.randn((R, D), device=dev, generator=gen)).to(bf)
    finf = (0.05 * torch.randn((R, D), device=dev, generator=gen)).to(bf)
    ldT = (R + 7) // 8 * 8
    finfT = torch.zeros((D, ldT), dtype=bf, device=dev)
    finfT[:, :R] = finf.t()
    st = lambda: lib.stream()   # noqa: E731
    arms = {}
    # the in-batch siblings
    nf, nb = C.c_int64(0), C.c_int64(0)
    lib.call("dpc_score_ws_floats", R, D, C.byref(nf), C.byref(nb))
    ws = torch.empty(max(nf.value, nb.value), dtype=f32, device=dev)
    diag, lse2, row_ws = (torch.empty(n, dtype=f32, device=dev) for n in (R, R, 2 * R))
    arms["dpc_score_fwd"] = (1, lambda: lib.call("dpc_score_fwd", pred, finf, R, D, diag, lse2, row_ws, None, ws, st()))
    arms["dpc_score_fwd"][1]()
    arms["dpc_score_bwd by_owner=1"] = (1, lambda: lib.call("dpc_score_bwd", pred, finf, finfT, ldT, R, D, lse2, 1, ws, st()))
    keep = []
    for K in args.slots:
        pitch = L.negq_pitch(R)
        ring = torch.zeros((K, pitch, D), dtype=bf, device=dev)
        ringT = torch.zeros((K, D, pitch), dtype=bf, device=dev)
        state = torch.zeros(4, dtype=torch.int32, device=dev)
        for _ in range(K):   # a full bank
            lib.call("dpc_negq_push", finf, finfT, ldT, ring, ringT, state, R, D, K, st())
        qf, qb = C.c_int64(0), C.c_int64(0)
        lib.call("dpc_negq_ws_floats", R, D, K, C.byref(qf), C.byref(qb))
        qws = torch.empty(max(qf.value, qb.value), dtype=f32, device=dev)
        stats, lse = torch.empty((R, 4), dtype=f32, device=dev), torch.empty(R, dtype=f32, device=dev)
        tgt = torch.zeros(R, dtype=f32, device=dev)
        keep.append((ring, ringT, state, qws, stats, lse, tgt))

        def fwd(K=K, ring=ring, state=state, tgt=tgt, stats=stats, qws=qws):
            lib.call("dpc_negq_fwd", pred, ring, state, R, D, K, tgt, 1, L.F32, stats, qws, st())
        fwd()
        torch.cuda.synchronize()
        lse.copy_(stats[:, 0] + torch.log(stats[:, 1]))

        def bwd(K=K, ring=ring, ringT=ringT, state=state, lse=lse, qws=qws):
            lib.call("dpc_negq_bwd", pred, ring, ringT, state, R, D, K, lse, qws, st())
        push = lambda K=K, ring=ring, ringT=ringT, state=state: lib.call("dpc_negq_push", finf, finfT, ldT, ring, ringT, state, R, D, K, st())   # noqa: E731
        arms[f"dpc_negq_fwd K={K}"] = (K, fwd)
        arms[f"dpc_negq_bwd K={K}"] = (K, bwd)
        arms[f"dpc_negq_push K={K}"] = (1, push)
    out = {name: [] for name in arms}
    for rnd in range(args.rounds):
        for name, (slots, fn) in arms.items():
            us = median_us(fn, args.reps)
            out[name].append(round(us, 1))
            print(f"round {rnd}  {name:28s} {us:9.1f} us  ({us / slots:8.1f} us per slot)", flush=True)
    print(json.dumps({"R": R, "D": D, "reps": args.reps, "median_us": out}))


if __name__ == "__main__":
    main()
