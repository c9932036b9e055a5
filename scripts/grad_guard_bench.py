#!/usr/bin/env python
"""The gradient guard's launches (csrc/grad_guard.hip) against the Adam kernels on the MI355X, launched singly: HIP events around one
launch, median and minimum of 50, over the r18 DPC arena and over the r18 LC arena with the `head` groups (only final_bn / final_fc
live).  A one-thread launch (dpc_step_advance) shows the floor of the method.

    python scripts/grad_guard_bench.py

docs/kernels.md and docs/design_parts/10_beyond.md ("Gradient guard") quote the output."""
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
    eng.flat_g.normal_()
    eng.set_grad_guard(max_norm=1.0, skip_nonfinite=True)
    seg, nseg = (eng._seg_dev, eng._seg_n) if eng.param_groups else (None, 0)
    st, part, n = eng._guard_state, eng._guard_partials, eng.numel
    live = n if not eng.param_groups else sum(eng.offsets[k][1] for g in eng.param_groups if not g["frozen"] for k in g["params"])
    print(f"== {tag}: arena {n} floats ({n * 4 / 1e6:.1f} MB), live {live} floats ({live * 4 / 1e6:.2f} MB)")
    rows = [("grad_sumsq", lambda: eng.call("dpc_grad_sumsq", eng.flat_g, n, seg, nseg, part), live * 4),
            ("grad_verdict", lambda: eng.call("dpc_grad_verdict", part, L.GRAD_PARTIALS, 1.0, 1, st), 0),
            ("step_advance_gated", lambda: eng.call("dpc_step_advance_gated", eng.dev_step, eng.dev_bc, 0.9, 0.999, st), 0),
            ("step_advance", lambda: eng.call("dpc_step_advance", eng.dev_step, eng.dev_bc, 0.9, 0.999), 0)]
    if eng.param_groups:
        rows += [("adam_groups_dev", lambda: eng.call("dpc_adam_groups_dev", eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v, n, seg, nseg, 0.9, 0.999, 1e-8, eng.dev_bc, 1.0), live * 28),
                 ("adam_groups_dev_ex", lambda: eng.call("dpc_adam_groups_dev_ex", eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v, n, seg, nseg, 0.9, 0.999, 1e-8, eng.dev_bc, 1.0, st), live * 28)]
    else:
        rows += [("adam_dev", lambda: eng.call("dpc_adam_dev", eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v, n, 1e-4, 0.9, 0.999, 1e-8, 1e-3, eng.dev_bc, 1.0), n * 28),
                 ("adam_dev_ex", lambda: eng.call("dpc_adam_dev_ex", eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v, n, 1e-4, 0.9, 0.999, 1e-8, 1e-3, eng.dev_bc, 1.0, st), n * 28)]
    for name, fn, nbytes in rows:
        med, mn = timed(fn)
        rate = f", {nbytes / med / 1e6:.2f} TB/s" if nbytes else ""
        print(f"{name:22s} median {med:8.1f} us  min {mn:8.1f} us{rate}", flush=True)


report("DPC resnet18", DPCEngine("resnet18", 64, 4, 5, 1, 2, DEV, torch.bfloat16))
lc = LCEngine("resnet18", 64, 4, 5, 2, DEV, torch.bfloat16, num_class=101)
lc.set_param_groups([{"params": [k for k in lc.offsets if k.startswith(("final_bn.", "final_fc."))], "lr": 1e-3, "weight_decay": 1e-3}])
report("LC resnet18, head groups", lc)
