#!/usr/bin/env python
"""The update rules of the fused step launched singly on the MI355X: dpc_adam_dev_ex against dpc_adamw_dev and the three LAMB launches
(dpc_lamb_moments / dpc_lamb_ratios / dpc_lamb_apply), over the r18 DPC arena and over the r18 LC arena with the `head` groups (only
final_bn / final_fc live).  HIP events around one launch, median and minimum of 50, two rounds; the method and its floor (a one-thread
launch) are those of scripts/ema_bench.py.

    python scripts/optim_bench.py

docs/kernels.md and docs/design_parts/10_beyond.md ("AdamW and LAMB") quote the output."""
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
    eng.flat_g.normal_(0.0, 1e-3)
    eng.set_optimizer("lamb")
    lm = eng._lamb
    seg, nseg = (eng._seg_dev, eng._seg_n) if eng.param_groups else (None, 0)
    n, p, g, m, v, bc = eng.numel, eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v, eng.dev_bc
    live = n if not eng.param_groups else sum(eng.offsets[k][1] for gr in eng.param_groups if not gr["frozen"] for k in gr["params"])
    print(f"== {tag}: arena {n} floats ({n * 4 / 1e6:.1f} MB), live {live} floats ({live * 4 / 1e6:.2f} MB), "
          f"{lm['n_seg']} segments, {lm['n_chunks']} chunks")
    eng.call("dpc_step_advance", eng.dev_step, bc, 0.9, 0.999)
    rows = [("step_advance", lambda: eng.call("dpc_step_advance", eng.dev_step, bc, 0.9, 0.999), 0)]
    if eng.param_groups:
        rows += [("adam_groups_dev_ex", lambda: eng.call("dpc_adam_groups_dev_ex", p, g, m, v, n, seg, nseg, 0.9, 0.999, 1e-8, bc, 1.0, None), live * 28),
                 ("adamw_groups_dev", lambda: eng.call("dpc_adamw_groups_dev", p, g, m, v, n, seg, nseg, 0.9, 0.999, 1e-8, bc, 1.0, None, None, None,
                                                       0.0, None), live * 28)]
    else:
        rows += [("adam_dev_ex", lambda: eng.call("dpc_adam_dev_ex", p, g, m, v, n, 1e-4, 0.9, 0.999, 1e-8, 1e-3, bc, 1.0, None), n * 28),
                 ("adamw_dev", lambda: eng.call("dpc_adamw_dev", p, g, m, v, n, 1e-4, 0.9, 0.999, 1e-8, 1e-3, bc, 1.0, None, None, None, 0.0, None), n * 28)]
    rows += [("lamb_moments", lambda: eng.call("dpc_lamb_moments", p, g, m, v, n, lm["seg"], lm["n_seg"], lm["chunks"], lm["n_chunks"], 0.9, 0.999,
                                               1e-8, bc, 1.0, None, lm["partials"]), live * 24),
             ("lamb_ratios", lambda: eng.call("dpc_lamb_ratios", lm["seg"], lm["n_seg"], lm["partials"], lm["n_chunks"], None, lm["records"]), 0),
             ("lamb_apply", lambda: eng.call("dpc_lamb_apply", p, m, v, n, lm["seg"], lm["n_seg"], lm["chunks"], lm["n_chunks"], 1e-8, bc, None,
                                             lm["records"], None, None, 0.0, None), live * 16)]

    launches = [fn for _, fn, _ in rows[-3:]]

    def three():
        for fn in launches:
            fn()
    rows += [("lamb, three launches", three, live * 40)]
    for name, fn, nbytes in rows * 2:   # two rounds, alternating
        med, mn = timed(fn)
        rate = f", {nbytes / med / 1e6:.2f} TB/s" if nbytes else ""
        print(f"{name:22s} median {med:8.1f} us  min {mn:8.1f} us{rate}", flush=True)


report("DPC resnet18", DPCEngine("resnet18", 64, 4, 5, 1, 2, DEV, torch.bfloat16))
lc = LCEngine("resnet18", 64, 4, 5, 2, DEV, torch.bfloat16, num_class=101)
lc.set_param_groups([{"params": [k for k in lc.offsets if k.startswith(("final_bn.", "final_fc."))], "lr": 1e-3, "weight_decay": 1e-3}])
report("LC resnet18, head groups", lc)
