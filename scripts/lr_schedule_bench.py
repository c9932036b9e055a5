#!/usr/bin/env python
"""The scheduled arm of the fused step (dpc_step_advance_sched, dpc_adam_dev_sched / dpc_adam_groups_dev_sched) against the entries it
stands in for, on the MI355X, launched singly: HIP events around one launch, median and minimum of 50, over the r18 DPC arena and over
the r18 LC arena with the `head` groups (only final_bn / final_fc live).  The method is that of scripts/ema_bench.py.

    python scripts/lr_schedule_bench.py

docs/kernels.md and docs/design_parts/10_beyond.md ("Learning-rate schedule") quote the output."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dpc_amd.engine import DPCEngine  # noqa: E402
from dpc_amd.lc import LCEngine  # noqa: E402
from dpc_amd.optim import LRSchedule  # noqa: E402

DEV = "cuda:0"
SCHED = LRSchedule("cosine", warmup_steps=10, total_steps=100000)


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
    eng.set_lr_schedule(SCHED)
    seg, nseg = (eng._seg_dev, eng._seg_n) if eng.param_groups else (None, 0)
    n, p, g, m, v, e = eng.numel, eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v, eng.flat_ema
    st, bc, rec, desc = eng.dev_step, eng.dev_bc, eng._lr_state, C.byref(eng._lr_desc)
    live = n if not eng.param_groups else sum(eng.offsets[k][1] for gr in eng.param_groups if not gr["frozen"] for k in gr["params"])
    print(f"== {tag}: arena {n} floats ({n * 4 / 1e6:.1f} MB), live {live} floats ({live * 4 / 1e6:.2f} MB)")
    eng.call("dpc_step_advance_sched", st, bc, 0.9, 0.999, None, desc, rec)
    rows = [("step_advance", lambda: eng.call("dpc_step_advance", st, bc, 0.9, 0.999), 0),
            ("step_advance_sched", lambda: eng.call("dpc_step_advance_sched", st, bc, 0.9, 0.999, None, desc, rec), 0)]
    if eng.param_groups:
        head = ("dpc_adam_groups_dev", (p, g, m, v, n, seg, nseg, 0.9, 0.999, 1e-8, bc, 1.0, None))
    else:
        head = ("dpc_adam_dev", (p, g, m, v, n, 1e-4, 0.9, 0.999, 1e-8, 1e-3, bc, 1.0, None))
    name, args = head
    rows += [(name[4:] + "_ex", lambda: eng.call(name + "_ex", *args), live * 28),
             (name[4:] + "_sched", lambda: eng.call(name + "_sched", *args, None, None, 0.0, rec), live * 28),
             (name[4:] + "_ema", lambda: eng.call(name + "_ema", *args, e, st, 0.999), live * 36),
             (name[4:] + "_sched + ema", lambda: eng.call(name + "_sched", *args, e, st, 0.999, rec), live * 36)]
    for label, fn, nbytes in rows * 2:   # two rounds, alternating
        med, mn = timed(fn)
        rate = f", {nbytes / med / 1e6:.2f} TB/s" if nbytes else ""
        print(f"{label:28s} median {med:8.1f} us  min {mn:8.1f} us{rate}", flush=True)


report("DPC resnet18", DPCEngine("resnet18", 64, 4, 5, 1, 2, DEV, torch.bfloat16))
lc = LCEngine("resnet18", 64, 4, 5, 2, DEV, torch.bfloat16, num_class=101)
lc.set_param_groups([{"params": [k for k in lc.offsets if k.startswith(("final_bn.", "final_fc."))], "lr": 1e-3, "weight_decay": 1e-3}])
report("LC resnet18, head groups", lc)
