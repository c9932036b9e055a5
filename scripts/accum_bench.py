#!/usr/bin/env python
"""The two modes of dpc_grad_accumulate (csrc/grad_accum.hip) launched singly on the MI355X: DPC_ACCUM_ADD and DPC_ACCUM_FINISH over
the r18 DPC arena, FINISH over its two buckets (the split of the two-bucket exchange), and both modes over the r18 LC arena with the
`head` groups (only final_bn / final_fc live).  HIP events around one launch, median and minimum of 50, two rounds; the method and
its floor (a one-thread launch) are those of scripts/ema_bench.py.

    python scripts/accum_bench.py

docs/kernels.md and docs/design_parts/10_beyond.md ("Gradient accumulation") quote the output."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpc_amd import _lib as L  # noqa: E402
from dpc_amd.engine import DPCEngine  # noqa: E402
from dpc_amd.lc import LCEngine  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def report(tag, eng):
    eng.flat_g.normal_(0.0, 1e-3)
    eng.set_grad_accum(4)
    n, split = eng.numel, eng.grad_split
    live = n if not eng.param_groups else sum(eng.offsets[k][1] for gr in eng.param_groups if not gr["frozen"] for k in gr["params"])
    print(f"== {tag}: arena {n} floats ({n * 4 / 1e6:.1f} MB), live {live} floats ({live * 4 / 1e6:.2f} MB), first bucket {split} floats")
    rows = [("step_advance (floor)", lambda: eng.call("dpc_step_advance", eng.dev_step, eng.dev_bc, 0.9, 0.999), 0),
            ("ADD", lambda: eng._accum_launch(L.ACCUM_ADD, 0, n), live * 12),
            ("FINISH", lambda: eng._accum_launch(L.ACCUM_FINISH, 0, n), live * 16)]
    if not eng.param_groups:
        rows += [("FINISH, tail bucket", lambda: eng._accum_launch(L.ACCUM_FINISH, split, n), (n - split) * 16),
                 ("FINISH, first bucket", lambda: eng._accum_launch(L.ACCUM_FINISH, 0, split), split * 16)]
    for name, fn, nbytes in rows * 2:   # two rounds, alternating
        med, mn = timed(fn)
        rate = f", {nbytes / med / 1e6:.2f} TB/s" if nbytes else ""
        print(f"{name:22s} median {med:8.1f} us  min {mn:8.1f} us{rate}", flush=True)


report("DPC resnet18", DPCEngine("resnet18", 64, 4, 5, 1, 2, DEV, torch.bfloat16))
lc = LCEngine("resnet18", 64, 4, 5, 2, DEV, torch.bfloat16, num_class=101)
lc.set_param_groups([{"params": [k for k in lc.offsets if k.startswith(("final_bn.", "final_fc."))], "lr": 1e-3, "weight_decay": 1e-3}])
report("LC resnet18, head groups", lc)
