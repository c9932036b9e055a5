#!/usr/bin/env python
"""The EMA arm of the Adam kernels (dpc_adam_dev_ema / dpc_adam_groups_dev_ema) against the entries it extends, and dpc_arena_swap, on
the MI355X, launched singly: HIP events around one launch, median and minimum of 50, over the r18 DPC arena and over the r18 LC arena
with the `head` groups (only final_bn / final_fc live).  The method is that of scripts/grad_guard_bench.py; its floor (a one-thread
launch) is printed with it.

    python scripts/ema_bench.py

docs/kernels.md and docs/design_parts/10_beyond.md ("EMA weights") quote the output."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
    eng.flat_g.normal_()
    eng.set_ema(0.999)
    seg, nseg = (eng._seg_dev, eng._seg_n) if eng.param_groups else (None, 0)
    n, p, g, m, v, e = eng.numel, eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v, eng.flat_ema
    live = n if not eng.param_groups else sum(eng.offsets[k][1] for gr in eng.param_groups if not gr["frozen"] for k in gr["params"])
    print(f"== {tag}: arena {n} floats ({n * 4 / 1e6:.1f} MB), live {live} floats ({live * 4 / 1e6:.2f} MB)")
    eng.call("dpc_step_advance", eng.dev_step, eng.dev_bc, 0.9, 0.999)
    rows = [("step_advance", lambda: eng.call("dpc_step_advance", eng.dev_step, eng.dev_bc, 0.9, 0.999), 0)]
    if eng.param_groups:
        rows += [("adam_groups_dev_ex", lambda: eng.call("dpc_adam_groups_dev_ex", p, g, m, v, n, seg, nseg, 0.9, 0.999, 1e-8, eng.dev_bc, 1.0, None), live * 28),
                 ("adam_groups_dev_ema", lambda: eng.call("dpc_adam_groups_dev_ema", p, g, m, v, n, seg, nseg, 0.9, 0.999, 1e-8, eng.dev_bc, 1.0, None,
                                                          e, eng.dev_step, 0.999), live * 36)]
    else:
        rows += [("adam_dev_ex", lambda: eng.call("dpc_adam_dev_ex", p, g, m, v, n, 1e-4, 0.9, 0.999, 1e-8, 1e-3, eng.dev_bc, 1.0, None), n * 28),
                 ("adam_dev_ema", lambda: eng.call("dpc_adam_dev_ema", p, g, m, v, n, 1e-4, 0.9, 0.999, 1e-8, 1e-3, eng.dev_bc, 1.0, None,
                                                   e, eng.dev_step, 0.999), n * 36)]
    rows += [("arena_swap", lambda: eng.call("dpc_arena_swap", p, e, n), n * 16)]
    for name, fn, nbytes in rows * 2:   # two rounds, alternating
        med, mn = timed(fn)
        rate = f", {nbytes / med / 1e6:.2f} TB/s" if nbytes else ""
        print(f"{name:22s} median {med:8.1f} us  min {mn:8.1f} us{rate}", flush=True)


report("DPC resnet18", DPCEngine("resnet18", 64, 4, 5, 1, 2, DEV, torch.bfloat16))
lc = LCEngine("resnet18", 64, 4, 5, 2, DEV, torch.bfloat16, num_class=101)
lc.set_param_groups([{"params": [k for k in lc.offsets if k.startswith(("final_bn.", "final_fc."))], "lr": 1e-3, "weight_decay": 1e-3}])
report("LC resnet18, head groups", lc)
