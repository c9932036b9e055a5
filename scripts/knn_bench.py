#!/usr/bin/env python
"""dpc_knn_topk against torch.topk(Q @ G.T, K) at the UCF101 split-1 size, on the MI355X.

    python scripts/knn_bench.py [--nq 3783] [--ng 9537] [--dim 256] [--iters 20] [--rounds 5] [--slabs 0]

Both sides run in one process on the same unit-norm f32 rows, K = 50 and K = 1, HIP events around --iters calls after a warm-up
call, --rounds rounds with the two sides alternating, so the spread is the session's own.  dpc_knn_topk goes through the C ABI with
its workspace and outputs allocated once (the wrapper of dpc_amd/retrieval.py allocates per call); the torch side is what the
README's "every arithmetic op is a kernel" rules out of a product file: it writes the nq x ng similarity matrix (137 MB) and
selects from it.  The neighbours of the two sides are compared once per K (indices equal wherever the f32 similarities of torch's
own list are distinct).  docs/design_parts/10_beyond.md quotes the output."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpc_amd import _lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nq", type=int, default=3783)
ap.add_argument("--ng", type=int, default=9537)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--slabs", type=int, default=0)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("knn_bench.py measures on the MI355X: no device found")
dev = "cuda:0"
lib = L.load_hip()
gen = torch.Generator(dev).manual_seed(11)
Q = torch.nn.functional.normalize(torch.randn(a.nq, a.dim, device=dev, generator=gen))
G = torch.nn.functional.normalize(torch.randn(a.ng, a.dim, device=dev, generator=gen))


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.iters * 1e3   # us


flop = 2.0 * a.nq * a.ng * a.dim
for K in (50, 1):
    ws_bytes = lib.call("dpc_knn_ws_bytes", a.nq, K, a.slabs)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    top_sim = torch.empty(a.nq, K, device=dev)
    top_idx = torch.empty(a.nq, K, dtype=torch.int32, device=dev)

    def ours():
        lib.call("dpc_knn_topk", Q, a.nq, a.dim, G, a.ng, a.dim, a.dim, K, None, a.slabs, top_sim, top_idx, ws, ws_bytes, lib.stream())

    def ref():
        return torch.topk(Q @ G.T, K)

    ours()
    want = ref()
    torch.cuda.synchronize()
    distinct = torch.ones_like(want.values, dtype=torch.bool)
    if K > 1:
        gap = want.values[:, :-1] != want.values[:, 1:]
        distinct[:, :-1] &= gap
        distinct[:, 1:] &= gap
    same = (top_idx.long() == want.indices) | ~distinct
    print(f"KNN K={K}: indices equal to torch.topk in {float(same.float().mean()):.6f} of the slots with distinct similarities, "
          f"max |sim difference| {float((top_sim - want.values).abs().max()):.3g}", flush=True)
    t_ours, t_ref = [], []
    for _ in range(a.rounds):
        t_ours.append(timed(ours))
        t_ref.append(timed(ref))
    for name, v in (("dpc_knn_topk", t_ours), ("torch.topk(Q @ G.T)", t_ref)):
        med = sorted(v)[len(v) // 2]
        print(f"KNN K={K} nq={a.nq} ng={a.ng} D={a.dim} slabs={a.slabs} {name}: us per call " + " ".join(f"{x:.0f}" for x in v) +
              f"  (min {min(v):.0f} median {med:.0f} max {max(v):.0f}; {flop / med / 1e6:.1f} TFLOP/s of the product alone)", flush=True)
