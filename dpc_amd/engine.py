"""Static-schedule engine for the DPC-RNN training step on one MI355X.

Host side of the hot path named in BASELINE.json: it owns the device buffers
(torch tensors are used only as device memory), the flat f32 parameter /
gradient / Adam-state arenas, and issues the hand-written gfx950 kernels of
``libdpc_hip.so`` through the C ABI (include/dpc_hip.h) on torch's current HIP
stream.  No autograd graph, no eager-PyTorch math: forward, loss, backward and
the optimizer are explicit kernel sequences with a fixed buffer plan, so the
step is capturable in a hipGraph and the backward can hand finished gradient
ranges to RCCL while it is still running.

What it restates (reference file:line):
  forward        dpc/model_3d.py:46-98, backbone/resnet_2d3d.py:259-270,47-116,
                 backbone/convrnn.py:24-34,62-88
  loss / top-k   dpc/main.py:178-185,213-218, utils/utils.py:38-55
  backward       torch autograd of the above (dpc/main.py:229-230)
  optimizer      torch.optim.Adam(lr, weight_decay) dpc/main.py:80-81,231

Data layout in HBM: activations channels-last [N][T][H][W][C] in the compute
dtype (f32 parity mode / bf16 throughput mode); parameters stay f32 in the
reference's state_dict layout and are repacked (K-contiguous, compute dtype) once
per optimizer step.

In file order: KernelTimer and the cost model; the conv unit and the block; ``BackboneEngine``, what the DPC-RNN step and the
LC classifier (lc.LCEngine) share, their captured steps included (capture_train_step / capture_eval_step over the heads'
``_forward_loss`` / ``_backward_reaches_backbone``; entry.StepDriver is what replays them in a run); ``DPCEngine``: the contrastive head.
"""
from __future__ import annotations

import atexit
import contextlib
import ctypes as C
import os
import weakref
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib as L
from .plan import LAYER_PLAN, LAYER_WIDTH, block_geometry, fold_decision, out_shape_of, unit_descs, walk_blocks  # shared with the plan query
BN_EPS = 1e-5
SCORE_NORM_EPS = 1e-12   # F.normalize's eps (the cosine score, DPCEngine.set_score_norm)


def param_shapes(network: str, widths: Sequence[int] = LAYER_WIDTH) -> "Dict[str, Tuple[int, ...]]":
    """state_dict keys/shapes of the reference DPC_RNN (without the agg.cell_list alias;
    dpc/model_3d.py:28-40, backbone/resnet_2d3d.py:205-257, backbone/convrnn.py:13-15)."""
    D = widths[3]
    out: Dict[str, Tuple[int, ...]] = {}
    out["backbone.conv1.weight"] = (widths[0], 3, 1, 7, 7)
    out["backbone.bn1.weight"] = (widths[0],)
    out["backbone.bn1.bias"] = (widths[0],)
    for pre, cin, planes, is3d, stride, has_ds, _ in walk_blocks(network, widths):
        pre, k = "backbone." + pre, block_geometry(is3d, stride)[0]
        out[pre + "conv1.weight"] = (planes, cin) + k
        out[pre + "bn1.weight"] = (planes,)
        out[pre + "bn1.bias"] = (planes,)
        out[pre + "conv2.weight"] = (planes, planes) + k
        out[pre + "bn2.weight"] = (planes,)
        out[pre + "bn2.bias"] = (planes,)
        if has_ds:
            out[pre + "downsample.0.weight"] = (planes, cin, 1, 1, 1)
            out[pre + "downsample.1.weight"] = (planes,)
            out[pre + "downsample.1.bias"] = (planes,)
    for gate in ("reset_gate", "update_gate", "out_gate"):
        out[f"agg.ConvGRUCell_00.{gate}.weight"] = (D, 2 * D, 1, 1)
        out[f"agg.ConvGRUCell_00.{gate}.bias"] = (D,)
    for idx in (0, 2):
        out[f"network_pred.{idx}.weight"] = (D, D, 1, 1)
        out[f"network_pred.{idx}.bias"] = (D,)
    return out


class KernelTimer:
    """HIP-event timing of selected C-ABI entry points on the launch stream (bench.py roofline leg).
    Every timed launch is bracketed by two events recorded on torch's current stream -- the stream the
    kernel is launched on -- and tagged with its algorithmic FLOPs / bytes.  Launches made inside
    ``with eng.tag("score")`` are additionally summed under ``tag:score``."""

    def __init__(self, names):
        self.names = set(names)
        self.records = []  # (name, tag, start_event, end_event, flops, bytes, executed flops)
        self.enabled = True

    def timed(self, eng, name, args):
        if not self.enabled:
            return eng.lib.call(name, *args, eng.lib.stream())
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = eng.lib.call(name, *args, eng.lib.stream())
        b.record()
        fl, by = algorithmic_cost(name, args)
        xf = fl * executed_fraction(name, args, L.last_kernel(eng.lib)) if fl else 0.0
        self.records.append((TIMER_FAMILY.get(name, name), eng._tag, a, b, fl, by, xf))
        return rc

    def summary(self, steps: int = 1):
        """Totals per entry point (and per tag).  The schedule is static, so with ``steps`` identical steps recorded every launch
        position has ``steps`` samples: its MEDIAN is charged for each of them -- an event pair also contains whatever time the
        host took between recording the first event and enqueueing the kernel, and one scheduler hiccup in a 60-launch family
        once doubled the family's reported time."""
        torch.cuda.synchronize()
        out = {}
        times = [r[2].elapsed_time(r[3]) for r in self.records]
        n = len(times)
        if steps > 1 and n % steps == 0:
            per = n // steps
            same = all(self.records[i][0] == self.records[i % per][0] for i in range(n))
            if same:
                for i in range(per):
                    col = sorted(times[i + k * per] for k in range(steps))
                    med = col[len(col) // 2] if len(col) % 2 else 0.5 * (col[len(col) // 2 - 1] + col[len(col) // 2])
                    for k in range(steps):
                        times[i + k * per] = med
        for (name, tag, a, b, fl, by, xf), ms in zip(self.records, times):
            for key in (name,) + ((f"tag:{tag}",) if tag else ()):
                d = out.setdefault(key, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0, "executed_flops": 0.0})
                d["launches"] += 1
                d["ms"] += ms
                d["flops"] += fl
                d["bytes"] += by
                d["executed_flops"] += xf
        return out


TIMER_FAMILY = {"dpc_conv_igemm_ex": "dpc_conv_igemm"}  # same kernels, fused backward pieces in the epilogue
HBM_FAMILY = ("dpc_bn_apply", "dpc_bn_bwd_reduce", "dpc_bn_bwd_apply", "dpc_bn_relu_maxpool_fwd", "dpc_pool_bn_bwd_apply",
              "dpc_pooled_bn_bwd_reduce", "dpc_pack_input_s2d")


def _esz(dc):
    return 2 if dc == L.BF16 else 4


def algorithmic_cost(name, args):
    """algorithmic FLOPs and HBM bytes (operands read once + output written once) of one launch"""
    if name == "dpc_bn_apply":          # x, y, dtype, rows, C, scale, shift, res, rscale, rshift, relu, mask
        n = args[3] * args[4] * _esz(args[2])
        return 0.0, float(n * (2 + (args[7] is not None)) + (n // 16 if args[11] is not None else 0))
    if name == "dpc_bn_bwd_reduce":     # dy, y, mask, x, dtype, rows, C, ...
        n = args[5] * args[6] * _esz(args[4])
        return 0.0, float(2 * n + (n // 16 if args[2] is not None else (n if args[1] is not None else 0)))
    if name == "dpc_bn_bwd_apply":      # dy, y, mask, x, dtype, rows, C, mean, invstd, gamma, coef, relu, dx, dz
        n = args[5] * args[6] * _esz(args[4])
        return 0.0, float(3 * n + (n if args[13] is not None else 0) + (n // 16 if args[2] is not None else (n if args[1] is not None else 0)))
    if name == "dpc_bn_relu_maxpool_fwd":   # raw, dtype, NT, H, W, C, scale, shift, pooled, arg
        e, NT, H, W, Cc = _esz(args[1]), args[2], args[3], args[4], args[5]
        return 0.0, float(NT * H * W * Cc * e + NT * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * Cc * (e + 1))
    if name == "dpc_pool_bn_bwd_apply":     # dy, arg, x, dtype, NT, H, W, C, ..., dx
        e, NT, H, W, Cc = _esz(args[3]), args[4], args[5], args[6], args[7]
        return 0.0, float(2 * NT * H * W * Cc * e + NT * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * Cc * (e + 1))
    if name == "dpc_pooled_bn_bwd_reduce":  # dy, arg, ypool, dtype, rows, C
        return 0.0, float(args[4] * args[5] * (2 * _esz(args[3]) + 1))
    if name == "dpc_pack_input_s2d":        # block, x_s2d, dtype, BN, SL, H, W
        px = args[3] * args[4] * args[5] * args[6]
        return 0.0, float(px * 3 * 4 + px * 4 * _esz(args[2]))
    if name == "dpc_score_fwd":            # pred, finf, R, D, ...: algorithmic = one R x R x D contraction, operands read once
        return 2.0 * args[2] * args[2] * args[3], float(2 * args[2] * args[3] * 2)
    if name == "dpc_score_bwd":            # own, oth, othT, ldT, R, D, ...: one R x R x D contraction (the recompute is not counted)
        return 2.0 * args[4] * args[4] * args[5], float(2 * args[4] * args[5] * 2 + args[4] * args[5] * 4)
    if name == "dpc_negq_fwd":             # pred, ring, state, R, D, K, ...: R x (K R) x D against a FULL bank (the live share is on the device)
        return 2.0 * args[3] * args[3] * args[5] * args[4], float((1 + args[5]) * args[3] * args[4] * 2)
    if name == "dpc_negq_bwd":             # pred, ring, ringT, state, R, D, K, ...: the same contraction (the recompute is not counted)
        return 2.0 * args[4] * args[4] * args[6] * args[5], float((1 + 2 * args[6]) * args[4] * args[5] * 2 + args[4] * args[5] * 4)
    if name in ("dpc_gemm_nt_splitk", "dpc_gemm_tn_splitk"):       # dtype, M, N, K, A, lda, B, ldb, part, nsplit
        e = _esz(args[0])
        return 2.0 * args[1] * args[2] * args[3], float((args[1] + args[2]) * args[3] * e + args[1] * args[2] * 4)
    if name not in ("dpc_conv_igemm", "dpc_conv_igemm_ex", "dpc_conv_wgrad"):
        return 0.0, 0.0
    d = args[0]._obj
    esz = 2 if d.dtype_in == L.BF16 else 4
    osz = 2 if d.dtype_out == L.BF16 else 4
    taps = d.KT * d.KH * d.KW
    rows_out = d.N * d.RT * d.RH * d.RW
    rows_src = d.N * d.ST * d.SH * d.SW
    if name in ("dpc_conv_igemm", "dpc_conv_igemm_ex") and d.mode == 1:
        # input-gradient: same MACs as the forward conv it differentiates (rows_src = forward output positions)
        macs = rows_src * d.Ci * d.Co * taps
    else:
        macs = rows_out * d.Co * d.Ci * taps
    if taps == 16 and d.Ci == 16 and d.KT == 1:  # space-to-depth stem: 147 of the 256 k-slots are real
        macs = macs * 147 // 256
    if name == "dpc_conv_igemm":
        by = rows_src * d.Ci * esz + d.Co * d.Ci * taps * esz + rows_out * d.Co * osz
    elif name == "dpc_conv_igemm_ex":  # + residual addend, the reduced unit's raw output, their byte masks
        ep = args[4]._obj
        n = rows_out * d.Co * osz
        by = rows_src * d.Ci * esz + d.Co * d.Ci * taps * esz + n
        by += (n if ep.addend else 0) + (n // 16 if ep.addend_mask else 0) + (n if ep.bn_raw else 0) + (n // 16 if ep.bn_mask else 0)
        name = "dpc_conv_igemm"
    else:
        by = rows_src * d.Ci * esz + rows_out * d.Co * esz + d.Co * d.Ci * taps * 4
    return 2.0 * macs, float(by)


def executed_fraction(name, args, kernel: str) -> float:
    """share of a launch's algorithmic FLOPs the matrix pipe actually executes.  The loader / compute kernel walks a 3x3x3 unit-stride
    convolution (forward or input-gradient) frame by frame and skips the temporal taps that would read zero padding as a K sub-range
    (csrc/conv_igemm_ws.hip `tgroup`): of the KT taps of output frame t only those with 0 <= t - pt + kt < ST run -- 7 of 9 at T = 3
    (layer3), 4 of 6 at T = 2 (layer4).  Everything else executes what it is charged (1.0); the stem's 147/256 is already in the
    algorithmic count."""
    if name not in ("dpc_conv_igemm", "dpc_conv_igemm_ex") or not kernel.startswith("igemm_ws_kernel"):
        return 1.0
    if os.environ.get("DPC_IGEMM_WS_TGROUP", "1") == "0":   # the A/B switch of the temporal grouping: every tap runs
        return 1.0
    d = args[0]._obj
    unit = d.st == 1 and d.sh == 1 and d.sw == 1
    if not (d.KT > 1 and unit and d.RT == d.ST and d.RT > 1):
        return 1.0
    live = sum(1 for t in range(d.RT) for kt in range(d.KT) if 0 <= t - d.pt + kt < d.ST)
    return live / float(d.RT * d.KT)


def _idle_at_exit():
    # nothing of this process is still queued on the GPU when the interpreter starts tearing streams, graphs and buffers down
    try:
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            torch.cuda.synchronize()
    except Exception:
        pass


atexit.register(_idle_at_exit)

# Captured train steps: ONE capture per (engine, input buffer, exchange) and no destruction while the process is running.
#   * capture_train_step() caches its result on the engine: asking again with the same static input buffer and the same exchange
#     returns the replay that exists (a trainer that "re-captures" every epoch holds one set of graphs, not one per epoch).
#   * hipGraphs are not destroyed while the process goes on.  Destroying the graphs of an engine (two streams forked and joined
#     inside the capture) and then building the next engine was followed, about once in five first runs of the GPU test tier on a
#     fresh box, by corrupted HOST memory -- a freshly built dict of this module losing a key (`load_params`: "in PRM: True, in
#     shapes: False"), a segfault in the next fork() -- and in 0 of 10 + 10 runs once the graphs were kept (profiles/r04_probes.txt).
#     A warm-process loop of 60 capture / destroy cycles reproduces nothing either way (scripts/probes/graph_destroy_probe.py), so
#     the mechanism inside the runtime is NOT established; what is established is the cost of the workaround, which this module
#     bounds: a graph set is parked in _LIVE_GRAPHS when its engine drops it (the engine dies, or release_captures() is called) and
#     stays there, with the private memory pool it captured into (= whatever the capture itself allocated: nothing after the two
#     eager warm-up steps, which size every lazy buffer), until the interpreter exits.  The list therefore grows with the number of
#     ENGINES that captured, not with the number of capture calls; DPC_KEEP_GRAPHS=0 destroys instead of parking.
_LIVE_GRAPHS: list = []


class _Capture:
    """the hipGraphs of one captured train step and the fork / join events that were recorded into them"""

    def __init__(self, graphs, events):
        self.graphs, self.events = graphs, events

    def destroy(self):
        """DPC_KEEP_GRAPHS=0 only: graphs first, then the events captured into them"""
        self.graphs.clear()
        if self.events is not None:
            self.events.clear()


def _park_graphs(captures):
    """keep the graphs of `captures` (list of _Capture) alive until the interpreter exits -- not even module teardown destroys them;
    DPC_KEEP_GRAPHS=0: destroy them now, in order"""
    if os.environ.get("DPC_KEEP_GRAPHS", "1") == "0":
        for c in captures:
            c.destroy()
        return
    for c in captures:
        for g_ in c.graphs:
            C.pythonapi.Py_IncRef(C.py_object(g_))
        _LIVE_GRAPHS.extend(c.graphs)
        _LIVE_GRAPHS.append(c.events)   # (a list of torch events, or None)


class _ConvBN:
    """one Conv3d (no bias) + BatchNorm3d(batch stats) unit and its saved tensors"""

    def __init__(self, eng: "BackboneEngine", wname: str, bnname: str, Ci: int, Co: int, k, s, p, in_shape, stem=False):
        self.eng, self.wname, self.bnname = eng, wname, bnname
        self.Ci, self.Co, self.k, self.s, self.p, self.stem = Ci, Co, k, s, p, stem
        N, T, H, W = in_shape
        self.in_shape = in_shape
        self.out_shape = out_shape_of(in_shape, k, s, p, stem)
        self.taps = k[0] * k[1] * k[2]
        dt = eng.cdtype
        dc = L.dtype_code(dt)
        No, To, Ho, Wo = self.out_shape
        self.rows = No * To * Ho * Wo
        Kp = self.taps * Ci
        self.desc_f, self.desc_d, self.desc_w = unit_descs(Ci, Co, k, s, p, in_shape, dt, stem)
        self.wp = eng.empty((Co, Kp), dt)
        self.wd = None if stem else eng.empty((Ci, self.taps * Co), dt)
        self.raw = eng.empty((No, To, Ho, Wo, Co), dt)
        self.mask = None  # ReLU sign mask of the activation that follows, allocated on first use
        self.stat_rows = eng.lib.call("dpc_conv_stats_rows", C.byref(self.desc_f))
        eng.need_stats(self.stat_rows * 2 * Co)
        self.mean, self.invstd, self.scale, self.shift = (eng.empty((Co,), torch.float32) for _ in range(4))
        if eng.bn_running:  # track_running_stats=True (eval/model_3d_lc.py:27-29): buffers in the reference's state_dict layout
            eng.BUF[bnname + ".running_mean"] = torch.zeros(Co, dtype=torch.float32, device=eng.device)
            eng.BUF[bnname + ".running_var"] = torch.ones(Co, dtype=torch.float32, device=eng.device)
            eng.BUF[bnname + ".num_batches_tracked"] = torch.zeros((), dtype=torch.int64, device=eng.device)
        ns = C.c_int32(0)
        eng.lib.call("dpc_conv_wgrad", C.byref(self.desc_w), None, None, Co, None, C.byref(ns), eng.lib.stream())
        eng.need_part(ns.value * Co * Kp)
        pr = C.c_int32(0)
        eng.lib.call("dpc_bn_bwd_reduce", None, None, None, None, dc, self.rows, Co, None, None, 0, None, C.byref(pr), eng.lib.stream())
        eng.need_stats(pr.value * 2 * Co)
        # the input-gradient launch can carry the BatchNorm-backward reduction of the unit upstream (dpc_conv_igemm_ex)
        self.stat_rows_d = 0 if stem else eng.lib.call("dpc_conv_stats_rows", C.byref(self.desc_d))
        eng.need_stats(self.stat_rows_d * 2 * Ci)
        self.reduced_rows = 0  # > 0: the partial sums of THIS unit's backward reduction are already in eng.stats (that many rows)
        self._coef_ready = False  # bn_prepare ran: eng.coef holds this unit's backward coefficients

    # ---- per-optimizer-step repack of the f32 parameter into MFMA operand layouts
    def pack_entries(self):
        """(source, destination, d0, d1, d2, s0, s1, s2) of this unit's repacks; the engine runs them all in one launch"""
        w = self.eng.PRM[self.wname]
        Ci, Co, t = self.Ci, self.Co, self.taps
        # wp[co][tap][ci] = w[co][ci][tap] ; wd[ci][tap][co] = w[co][ci][tap]
        return [(w, self.wp, Co, t, Ci, Ci * t, 1, t), (w, self.wd, Ci, t, Co, t, 1, Ci * t)]

    def forward(self, x: torch.Tensor):
        e = self.eng
        g, b = e.PRM[self.bnname + ".weight"], e.PRM[self.bnname + ".bias"]
        if e.bn_running and not e.train_mode:  # eval: coefficients from the running buffers, no batch statistics
            e.call("dpc_conv_igemm", C.byref(self.desc_f), x, self.wp, self.raw, None, None)
            e.call("dpc_bn_eval_coeffs", g, b, e.BUF[self.bnname + ".running_mean"], e.BUF[self.bnname + ".running_var"], BN_EPS,
                   self.Co, self.mean, self.invstd, self.scale, self.shift)
            return
        e.call("dpc_conv_igemm", C.byref(self.desc_f), x, self.wp, self.raw, None, e.stats)
        if e.bn_running:
            e.call("dpc_bn_finalize_running", e.stats, self.stat_rows, self.Co, float(self.rows), g, b, BN_EPS, self.mean, self.invstd,
                   self.scale, self.shift, e.BUF[self.bnname + ".running_mean"], e.BUF[self.bnname + ".running_var"],
                   e.BUF[self.bnname + ".num_batches_tracked"], e.BN_MOMENTUM)
        else:
            e.call("dpc_bn_finalize", e.stats, self.stat_rows, self.Co, float(self.rows), g, b, BN_EPS, self.mean, self.invstd,
                   self.scale, self.shift)

    def apply(self, y: torch.Tensor, relu: bool, res: Optional[torch.Tensor] = None, res_unit: "Optional[_ConvBN]" = None):
        e = self.eng
        if relu and self.mask is None:  # byte per 16-byte unit: what the backward reads instead of y
            self.mask = e.empty((self.rows * self.Co * self.raw.element_size() // 16,), torch.uint8)
        e.call("dpc_bn_apply", self.raw, y, L.dtype_code(e.cdtype), self.rows, self.Co, self.scale, self.shift, res,
               res_unit.scale if res_unit else None, res_unit.shift if res_unit else None, int(relu),
               self.mask if relu else None)

    # ---- backward pieces
    def bn_backward(self, dy: torch.Tensor, y: Optional[torch.Tensor], relu: bool, dx: torch.Tensor,
                    dz: Optional[torch.Tensor] = None, ext_mask: Optional[torch.Tensor] = None):
        """BatchNorm backward of this unit: dz = dy gated by the ReLU that follows it (its own sign mask, or `ext_mask`: the
        downsample branch sees the block output's gate) -> partial sums -> coefficients -> dx (and dz, when a caller still
        wants it as a tensor).  The reduction pass is skipped when the launch that produced dy already took the sums."""
        e = self.eng
        dc = L.dtype_code(e.cdtype)
        mask = ext_mask if ext_mask is not None else (self.mask if relu else None)
        gated = int(relu or ext_mask is not None)
        if not self._coef_ready:
            self.bn_prepare(dy, y, relu, ext_mask)
        self._coef_ready = False
        e.call("dpc_bn_bwd_apply", dy, None if mask is not None else y, mask, self.raw, dc, self.rows, self.Co, self.mean,
               self.invstd, e.PRM[self.bnname + ".weight"], e.coef, gated, dx, dz)

    def bn_prepare(self, dy: torch.Tensor, y: Optional[torch.Tensor], relu: bool, ext_mask: Optional[torch.Tensor] = None):
        """first half of bn_backward: partial sums (unless the launch that produced dy took them) -> coefficients in eng.coef.
        Callable on its own so that the 2..8-workgroup finalize kernel is enqueued BEFORE a weight gradient is forked onto the side
        stream: behind it, it waits for a CU -- its 1 024-thread workgroups fit on no CU beside two wgrad_patch workgroups -- until
        the first weight-gradient workgroup retires, 120..230 us on the critical path (profiles/r03_r18_128_step_timeline.txt:
        bn_bwd_finalize 212 us at 23.07 ms against 5 us elsewhere; 0.75 ms per step in profiles/r04_*_sessionC against 0.15 ms
        of work).  Nothing else may write eng.coef between this call and the matching bn_backward."""
        e = self.eng
        dc = L.dtype_code(e.cdtype)
        mask = ext_mask if ext_mask is not None else (self.mask if relu else None)
        gated = int(relu or ext_mask is not None)
        if self.reduced_rows:
            prow, self.reduced_rows = self.reduced_rows, 0
        else:
            pr = C.c_int32(0)
            e.call("dpc_bn_bwd_reduce", dy, None if mask is not None else y, mask, self.raw, dc, self.rows, self.Co, self.mean,
                   self.invstd, gated, e.stats, C.byref(pr))
            prow = pr.value
        e.call("dpc_bn_bwd_finalize", e.stats, prow, self.Co, float(self.rows), e.G[self.bnname + ".weight"],
               e.G[self.bnname + ".bias"], e.coef)
        self._coef_ready = True

    def wgrad(self, x: torch.Tensor, draw: torch.Tensor):
        e = self.eng
        ns = C.c_int32(0)
        e.call("dpc_conv_wgrad", C.byref(self.desc_w), x, draw, self.Co, e.part, C.byref(ns))
        g = e.G[self.wname]
        if self.stem:
            e.call("dpc_unpack_stem_wgrad", e.part, ns.value, g, self.Co)
        else:
            Ci, t = self.Ci, self.taps
            e.call("dpc_reduce_unpack", e.part, ns.value, g, self.Co, t, Ci, Ci * t, 1, t, 0)

    def dgrad(self, draw: torch.Tensor, dx: torch.Tensor, addend: Optional[torch.Tensor], addend_mask: Optional[torch.Tensor] = None,
              red: "Optional[_ConvBN]" = None):
        """input-gradient (+ residual addend).  addend_mask: the addend is gated by that ReLU sign mask (the block's dz is never
        a tensor).  red: the unit whose output gradient dx is -- its BatchNorm-backward partial sums are taken in this launch's
        epilogue and `red.bn_backward` skips its reduction pass."""
        e = self.eng
        e.side_wait()   # no side-stream work beside an input-gradient (see side())
        if addend_mask is None and red is None:
            e.call("dpc_conv_igemm", C.byref(self.desc_d), draw, self.wd, dx, addend, None)
            return
        ep = L.ConvEpilogue()
        ep.addend = addend.data_ptr() if addend is not None else None
        ep.addend_mask = addend_mask.data_ptr() if addend_mask is not None else None
        if red is not None:
            ep.bn_raw, ep.bn_mean, ep.bn_invstd = red.raw.data_ptr(), red.mean.data_ptr(), red.invstd.data_ptr()
            ep.bn_mask = red.mask.data_ptr() if red.mask is not None else None
            ep.stats = e.stats.data_ptr()
        e.call("dpc_conv_igemm_ex", C.byref(self.desc_d), draw, self.wd, dx, C.byref(ep))
        if red is not None:  # rows of THIS launch (a CU carve-out in force shrinks the persistent grid)
            red.reduced_rows = self.stat_rows_d if not e.reserve_cus else e.lib.call("dpc_conv_stats_rows", C.byref(self.desc_d))


class _Block:
    """BasicBlock2d / BasicBlock3d (backbone/resnet_2d3d.py:47-116)"""

    def __init__(self, eng, pre: str, Ci: int, Co: int, is3d: bool, stride: int, in_shape, has_ds: bool, final_relu: bool):
        self.eng = eng
        k, s, p = block_geometry(is3d, stride)
        self.c1 = _ConvBN(eng, pre + "conv1.weight", pre + "bn1", Ci, Co, k, s, p, in_shape)
        self.c2 = _ConvBN(eng, pre + "conv2.weight", pre + "bn2", Co, Co, k, (1, 1, 1), p, self.c1.out_shape)
        self.ds = _ConvBN(eng, pre + "downsample.0.weight", pre + "downsample.1", Ci, Co, (1, 1, 1), s, (0, 0, 0),
                          in_shape) if has_ds else None
        self.final_relu = final_relu
        self.site = pre[len("backbone."):]   # "layer2.0.": names this block's side-stream sites (BackboneEngine.side_off)
        self.out_shape = self.c2.out_shape
        self.Co = Co
        self.act1 = eng.empty(self.c1.out_shape + (Co,), eng.cdtype)
        self.out = eng.empty(self.out_shape + (Co,), eng.cdtype)
        self.x_in: Optional[torch.Tensor] = None

    def units(self):
        return [u for u in (self.c1, self.c2, self.ds) if u is not None]

    def forward(self, x):
        self.x_in = x
        self.c1.forward(x)
        self.c1.apply(self.act1, relu=True)
        self.c2.forward(self.act1)
        if self.ds is not None:
            self.ds.forward(x)
            self.c2.apply(self.out, relu=self.final_relu, res=self.ds.raw, res_unit=self.ds)
        else:
            self.c2.apply(self.out, relu=self.final_relu, res=x)
        return self.out

    def plan_backward(self, prev: "Optional[_Block]"):
        """which backward pieces ride in input-gradient epilogues (decided once): plan.fold_decision, under the engine's switches"""
        e = self.eng
        fold_c1, gate, fold_prev = (False, False, False) if not e.fold else fold_decision(
            e.lib, self.c1.desc_d, self.c2.desc_d, self.ds is not None, self.final_relu, prev is not None)
        red = bool(int(os.environ.get("DPC_FOLD_RED", "1")))   # probe: the reductions as their own launches, the gated addend stays fused
        self.fold_c1, self.gate, self.fold_prev = red and fold_c1, gate, red and fold_prev
        self.prev = prev

    def backward(self, dout: torch.Tensor, need_dx: bool = True) -> Optional[torch.Tensor]:
        e = self.eng
        oshape = tuple(self.out.shape)
        ishape = tuple(self.x_in.shape)
        omask = self.c2.mask if self.final_relu else None  # gate of everything behind the block output: dz = dout * (out > 0)
        draw2 = e.scratch(oshape, exclude=[dout])
        # the masked gradient dz as a tensor only when a consumer cannot gate on the fly
        dz = None
        if self.ds is None and not self.gate and need_dx:
            dz = e.scratch(oshape, exclude=[dout, draw2])
        self.c2.bn_backward(dout, self.out if self.final_relu else None, self.final_relu, draw2, dz)
        draw_d = None
        if self.ds is not None:
            draw_d = e.scratch(oshape, exclude=[dout, draw2])  # lives until the block's last input-gradient
            self.ds.bn_backward(dout, None, False, draw_d, ext_mask=omask)
        dact1 = e.scratch(oshape, exclude=[dout, draw2, draw_d, dz])
        self.c2.dgrad(draw2, dact1, None, red=self.c1 if self.fold_c1 else None)
        if self.fold_c1:   # coefficients of bn1 before the side stream fills the chip (bn_prepare)
            self.c1.bn_prepare(dact1, self.act1, True)
        with e.side(reads=[draw2, draw_d], site=self.site + "c2"):   # beside bn1's backward on the main stream
            if self.ds is not None:
                self.ds.wgrad(self.x_in, draw_d)
            self.c2.wgrad(self.act1, draw2)
        # in place over the consumed draw2 unless the side stream may still be reading it
        draw1 = draw2 if e._side is None or e.timer is not None else e.scratch(oshape, exclude=[dout, draw2, draw_d, dz, dact1])
        self.c1.bn_backward(dact1, self.act1, True, draw1)
        if not need_dx:
            with e.side(reads=[draw1], site=self.site + "c1"):
                self.c1.wgrad(self.x_in, draw1)
            return None
        if self.ds is not None:
            # dx = main path; the strided 1x1 downsample then accumulates IN PLACE on the positions it reads (1/4 of dx in 2D,
            # 1/8 in 3D) -- round 1 wrote a full, 75-88 % zero tensor and re-read it as the addend
            dx = e.scratch(ishape, exclude=[])
            self.c1.dgrad(draw1, dx, None)
            self.ds.dgrad(draw_d, dx, dx)
        elif self.gate:
            # in place over dout: every lane reads its addend unit before it stores the same unit (all kernels behind the entry)
            dx = dout
            self.c1.dgrad(draw1, dx, dout, addend_mask=omask, red=self.prev.c2 if self.fold_prev else None)
            if self.fold_prev:   # the previous block's bn2 (its backward is the next thing on the main stream)
                pv = self.prev
                pv.c2.bn_prepare(dx, pv.out if pv.final_relu else None, pv.final_relu)
        else:
            dx = dact1  # same shape as the input; dact1 is dead
            self.c1.dgrad(draw1, dx, dz)
        with e.side(reads=[draw1], site=self.site + "c1"):   # beside the previous block's bn2 backward (beside conv1's own input-gradient: slower)
            self.c1.wgrad(self.x_in, draw1)
        return dx


# live engines by the address of their parameter arena (weak: an engine dies with its owner)
ENGINES: "weakref.WeakValueDictionary[int, BackboneEngine]" = weakref.WeakValueDictionary()


def engine_of(param: torch.Tensor) -> "Optional[BackboneEngine]":
    """the engine whose flat parameter arena `param` is a view of (None: an ordinary tensor)"""
    a = param.data_ptr()
    for base, eng in list(ENGINES.items()):
        if base <= a < base + eng.flat_p.numel() * 4:
            return eng
    return None


class BackboneEngine:
    """What both models run on: the flat arenas and their offsets, streams and scratch, the 2d3d-ResNet with its backward, the
    ConvGRU host wiring, the device counters and the fused Adam.  A head (DPCEngine below, lc.LCEngine) calls this constructor
    with its parameter shapes, builds its own buffers (_build_gru for the recurrence) and ends with _finish_buffers()."""
    BN_MOMENTUM = 0.1  # torch.nn.BatchNorm3d default

    def __init__(self, shapes: "Dict[str, Tuple[int, ...]]", network: str, sample_size: int, num_seq: int, seq_len: int, batch: int,
                 device, compute_dtype, widths: Sequence[int], lib: Optional[L.Lib], lr: float, wd: float, gru_dropout: float, seed: int,
                 stem_fused: bool | None = None, fold: bool | None = None, reserve_cus: int | None = None,
                 f32_matmul: str | None = None, bn_running: bool = False):
        self.device = torch.device(device)
        self.lib = L.lib_for(self.device, lib)  # raises unless HIP device (or an explicit simulator handle in tests)
        self.cdtype = compute_dtype
        self.network, self.size, self.N, self.SL, self.B = network, sample_size, num_seq, seq_len, batch
        self.widths = tuple(widths)
        self.D = widths[3]
        self.lr, self.wd, self.p_drop = lr, wd, gru_dropout
        self.last_duration = int(math.ceil(seq_len / 4))   # dpc/model_3d.py:24
        self.last_size = int(math.ceil(sample_size / 32))  # dpc/model_3d.py:25
        self.SQ = self.last_size ** 2
        if sample_size % 2:
            raise ValueError("sample_size must be even (space-to-depth stem)")
        self._stats_need = 0
        self._part_need = 0
        self._scratch: Dict[Tuple[int, ...], List[torch.Tensor]] = {}
        self._step_count = 0
        self._groups, self._groups_key, self._seg_host, self._seg_dev, self._seg_n = None, None, None, None, 0   # parameter groups of the fused Adam (set_param_groups)
        self._guard, self._guard_state, self._guard_partials = None, None, None   # gradient guard of the fused Adam (set_grad_guard)
        self._steps_unsure = False   # a step may have been skipped on the device since _step_count was last read from dev_step
        self._ema, self.flat_ema, self._ema_swapped = None, None, False   # parameter average of the fused Adam (set_ema, swap_ema)
        self._lr_sched, self._lr_desc, self._lr_state = None, None, None   # per-step learning-rate schedule of the fused Adam (set_lr_schedule)
        self._opt_kind, self._opt_x1d, self._opt_key, self._opt_host = "adam", False, None, b""   # update rule of the fused step (set_optimizer)
        self._lamb, self._aw_seg_dev, self._aw_seg_n = None, None, 0   # LAMB's device tables; AdamW's own segment table under exclude_1d
        self._accum_n, self._accum_pos, self.flat_acc = 1, 0, None   # gradient accumulation in front of the fused step (set_grad_accum)
        self._negq, self._negq_gen = 0, 0   # slots of the negative queue (DPCEngine.set_neg_queue; 0: off) and how often its ring was allocated
        self.seg_uploads = 0          # host-to-device copies of the segment table so far
        self.no_grad_params = frozenset()   # parameters whose gradient nobody wants (requires_grad = False at the module boundary)
        self.seed = int(seed)  # dropout stream (the reference seeds the device generator with 233, dpc/model_3d.py:18); per rank
        self.timer: Optional["KernelTimer"] = None
        self._tag: Optional[str] = None
        self._capture_events: Optional[list] = None   # fork / join events of the capture in progress (_capture)
        self._captures: Dict[tuple, object] = {}   # capture_train_step / capture_eval_step results by (input buffer, exchange, carve-out, ...)
        self._capture_graphs: list = []            # their _Capture records; parked in _LIVE_GRAPHS when the engine goes (see there)
        self._launches = 0                         # kernel launches issued through call() so far (_capture: launches per captured graph)
        weakref.finalize(self, _park_graphs, self._capture_graphs)
        self._carved = False   # a CU carve-out for RCCL is in force (_backbone_backward sets it, _uncarve lifts it)

        # ---- flat f32 arenas: parameters, gradients, Adam moments
        # Fused stem weight gradient (csrc/conv_wgrad_stem.hip: no full-resolution dz tensor, bit-identical to the two-kernel form).
        # Round 2's register-gather version was slower than the two kernels and opt-in; the LDS-DMA rebuild of round 3 is faster in
        # the step (4 667 against 4 617 clips/s at cfg2) and the default; DPC_STEM_FUSED=0 / stem_fused=False run the two kernels.
        self._want_stem_fused = bool(int(os.environ.get("DPC_STEM_FUSED", "1"))) if stem_fused is None else bool(stem_fused)
        # backward pieces fused into input-gradient epilogues (dz never written, BatchNorm-backward reductions in the producing
        # launch): on by default, DPC_FOLD=0 / fold=False runs the separate kernels (A/B, and the reference for the fused form)
        self.fold = bool(int(os.environ.get("DPC_FOLD", "1"))) if fold is None else bool(fold)
        # CUs left to RCCL's channel kernels while the gradient tail is being all-reduced under layer1 + stem backward: the
        # persistent one-workgroup-per-CU kernels of that phase shrink their grids (dpc_set_reserved_cus).  Only consulted when a
        # two-bucket exchange is running; data-parallel callers pass parallel.default_reserve_cus(world) (= the RCCL channel count:
        # measured with a co-tenant on one GPU, profiles/r04_cotenant.txt), single-GPU runs 0.
        self.reserve_cus = int(os.environ.get("DPC_RESERVE_CUS", "0")) if reserve_cus is None else int(reserve_cus)
        # arithmetic of the f32 kernels' contractions (include/dpc_hip.h: dpc_set_f32_matmul): "exact" = f32 MFMA chains (default),
        # "bf16x6" = operands split three ways onto the bf16 matrix pipe -- f32-grade results (the reference goldens hold at 1e-3:
        # tests/test_engine_gpu.py), up to 2.7x the f32 matrix rate.  Only meaningful with compute_dtype=float32.
        mm = (f32_matmul or os.environ.get("DPC_F32_MATMUL", "exact")).lower()
        if mm not in ("exact", "bf16x6"):
            raise ValueError("f32_matmul must be 'exact' or 'bf16x6'")
        self.f32_matmul = mm
        self._x6 = 1 if (mm == "bf16x6" and compute_dtype == torch.float32) else 0
        self._pack_table = None
        # weight gradients on a second stream beside the next unit's BatchNorm backward (side() below); DPC_WGRAD_STREAM=0: one stream.
        # What goes there: conv2 / downsample weight gradients, conv1's, the head's parameter gradients, the per-step weight repacks;
        # the main stream waits for the side stream before every input-gradient (side()).  Rounds 3-4 had switches for both choices
        # (DPC_SIDE_MASK, DPC_SIDE_QUIET); every other setting measured slower and the switches are gone (round 5).
        self._side = (torch.cuda.Stream(self.device) if self.device.type == "cuda" and int(os.environ.get("DPC_WGRAD_STREAM", "1")) else None)
        self._on_side = False
        self.side_off = frozenset(x for x in os.environ.get("DPC_SIDE_OFF", "").split(",") if x)   # probe knob (scripts/probes/side_sites.py)
        self._busy = []   # [(event recorded on the side stream, scratch buffers its launches read)], oldest first
        self.bn_running = bool(bn_running)  # BatchNorm3d with running statistics (the LC classifier's backbone)
        self.train_mode = True       # only matters when bn_running: eval uses the running buffers
        self.BUF: Dict[str, torch.Tensor] = {}
        self.shapes = shapes
        self.offsets: Dict[str, Tuple[int, int]] = {}
        off = 0
        for k, shp in self.shapes.items():
            n = int(math.prod(shp))
            self.offsets[k] = (off, n)
            off += (n + 3) // 4 * 4  # keep every tensor 16-byte aligned
        self.numel = off
        self.flat_p = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.flat_g = torch.zeros_like(self.flat_p)
        self.flat_m = torch.zeros_like(self.flat_p)
        self.flat_v = torch.zeros_like(self.flat_p)
        self.PRM = {k: self.flat_p[o:o + n].view(self.shapes[k]) for k, (o, n) in self.offsets.items()}
        ENGINES[self.flat_p.data_ptr()] = self   # dpc_amd.optim.Adam finds the engine behind a module's parameters (views of flat_p)
        self.G = {k: self.flat_g[o:o + n].view(self.shapes[k]) for k, (o, n) in self.offsets.items()}

        # ---- backbone plan
        BN, H = batch * num_seq, sample_size
        dt = self.cdtype
        self.x_s2d = self.empty((BN, seq_len, H // 2, H // 2, 16), dt)
        # synthetic-input draw counter (fill_synthetic): advanced in front of every draw, read by dpc_synthetic_input on the device
        self.dev_input = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._resident_ws = None   # load_resident's jitter workspaces (u8 image, per-frame L sums): allocated by its first call
        self.stem =_ConvBN(self, "backbone.conv1.weight", "backbone.bn1", 16, widths[0], (1, 4, 4), (1, 1, 1), (0, 2, 2),
                            (BN, seq_len, H // 2, H // 2), stem=True)
        hp = (H // 2 - 1) // 2 + 1
        self.pool_shape = (BN, seq_len, hp, hp)
        self.pooled = self.empty(self.pool_shape + (widths[0],), dt)
        self.pool_arg = torch.empty(self.pool_shape + (widths[0],), dtype=torch.uint8, device=self.device)
        self.blocks: List[_Block] = []
        shape = self.pool_shape
        for pre, cin, planes, is3d, stride, has_ds, last in walk_blocks(network, widths):
            blk = _Block(self, "backbone." + pre, cin, planes, is3d, stride, shape, has_ds, final_relu=not last)
            self.blocks.append(blk)
            shape = blk.out_shape
        for i, blk in enumerate(self.blocks):
            blk.plan_backward(self.blocks[i - 1] if i > 0 else None)
        # gradient-arena split for the overlapped all-reduce: the head = stem + layer1 (finished last by the backward)
        self.n_head_blocks = LAYER_PLAN[network][0]
        self.grad_split = self.offsets["backbone.layer2.0.conv1.weight"][0]
        self.feat_shape = shape
        if shape[1] != self.last_duration or shape[2] != self.last_size or shape[3] != self.last_size:
            raise ValueError(f"backbone output {shape} does not match last_duration/last_size "
                             f"({self.last_duration},{self.last_size}); see dpc/model_3d.py:24-25,53-55")
        self.units: List[_ConvBN] = [self.stem] + [u for b in self.blocks for u in b.units()]

        # optimizer-step counter and Adam bias corrections in device memory: a captured hipGraph advances them on replay
        self.dev_step = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.dev_bc = torch.ones(2, dtype=torch.float32, device=self.device)
        # dropout draw counter: every train-mode forward advances it, the recurrence keys its Philox masks on it.  Not the optimizer
        # step: the nn.Module boundary with an external torch optimizer never runs adam_step() and would redraw one mask forever
        self.dev_draw = torch.zeros(1, dtype=torch.int32, device=self.device)

    # ---- ConvGRU host wiring (backbone/convrnn.py:24-34,62-88), one copy for both heads: buffers, sizing, the descriptor's common
    # fields here; the pack in pack_weights; the parameter gradients in _gru_param_grads
    def _build_gru(self, n_agg: int, n_steps: int, P: int):
        """the recurrence over n_steps steps, the first n_agg of them aggregation (rows M = (b, s)); the head adds its own
        descriptor fields to self.gru_desc"""
        N, D, SQ, dt, f32 = self.N, self.D, self.SQ, self.cdtype, torch.float32
        # the recurrence runs as two launches (dpc_gru_chain_fwd / _bwd, csrc/gru_chain.hip): fragment-major packed weights,
        # f32 scratch of the backward kernel, and the descriptor with every (static) buffer address
        if D % 32 or D > 256:
            raise ValueError("feature size must be a multiple of 32, at most 256 (fused ConvGRU recurrence)")
        M = self.B * SQ
        ns = n_steps
        self.M, self.n_agg, self.n_steps = M, n_agg, ns
        self.feat_relu = self.empty((N, M, D), dt)    # [n][(b,s)][d]; slots [0,n_steps) double as the GRU inputs
        self.X_all = self.feat_relu[:ns]              # GRU inputs x_t (agg: feat_relu[t]; predict: relu(p_t) overwrites
                                                      # the slots of the last P blocks, whose ReLU'd features are unused)
        self.H_all = torch.zeros((ns + 1, M, D), dtype=dt, device=self.device)   # h_0 = 0 (never written), h_t after dropout
        self.HR_all = self.empty((ns, M, D), dt)
        self.G_all = self.empty((ns, M, 3 * D), dt)   # [dpu | dpr | dpo] per step
        self.U_all, self.R_all, self.O_all = (self.empty((ns, M, D), f32) for _ in range(3))
        self.drop_all: Optional[torch.Tensor] = None
        self.d_featrelu = self.empty((n_agg, M, D), f32)
        self.d_feat = self.empty(self.feat_shape + (D,), dt)
        self.gru_packed = self.empty((16 * D * D,), dt)
        self.gru_ws = self.empty((2, M, D), f32)
        self.dWx = self.empty((3 * D, D), f32)
        self.dWh = self.empty((2 * D, D), f32)
        self.dWo = self.empty((D, D), f32)
        self.db = self.empty((3 * D,), f32)
        for (co, kk) in ((3 * D, D), (2 * D, D), (D, D)):
            self._need_wgrad(ns * M, co, kk)
        self.need_part(64 * 3 * D)  # dpc_colsum workspace
        self._gate_table = None
        gd, Pm = L.GruChainDesc(), self.PRM
        gd.dtype, gd.M, gd.D, gd.SQ, gd.P, gd.n_agg, gd.n_steps = L.dtype_code(dt), M, D, SQ, P, n_agg, ns
        gd.p_drop, gd.seed = float(self.p_drop), self.seed
        for name, t in (("packed", self.gru_packed), ("bias_u", Pm["agg.ConvGRUCell_00.update_gate.bias"]),
                        ("bias_r", Pm["agg.ConvGRUCell_00.reset_gate.bias"]), ("bias_o", Pm["agg.ConvGRUCell_00.out_gate.bias"]),
                        ("X_all", self.X_all), ("H_all", self.H_all), ("HR_all", self.HR_all), ("U_all", self.U_all),
                        ("R_all", self.R_all), ("O_all", self.O_all), ("G_all", self.G_all), ("d_x", self.d_featrelu),
                        ("ws", self.gru_ws)):
            setattr(gd, name, t.data_ptr())
        self.gru_desc = gd

    def _gru_param_grads(self, dc):
        """weight / bias gradients of the ConvGRU, batched over all steps, into the gradient arena (on whichever stream the head
        issues them)"""
        D, M, ns, Gm = self.D, self.M, self.n_steps, self.G
        self.gemm_tn(self.G_all, 3 * D, self.X_all, D, self.dWx, ns * M, 3 * D, D)
        self.gemm_tn(self.G_all, 3 * D, self.H_all, D, self.dWh, ns * M, 2 * D, D)
        self.gemm_tn(self.G_all[:, :, 2 * D:], 3 * D, self.HR_all, D, self.dWo, ns * M, D, D)
        self.call("dpc_colsum", self.G_all, dc, 3 * D, ns * M, 3 * D, self.db, 0, self.part, self.part.numel())
        if self._gate_table is None:   # the nine gate slices in one launch (static table: addresses never change)
            ents = []
            for i, (g, n) in enumerate((("u", "update_gate"), ("r", "reset_gate"), ("o", "out_gate"))):
                w = Gm[f"agg.ConvGRUCell_00.{n}.weight"].view(D, 2 * D)   # [D][x half | h half]
                ents += [(self.dWx[i * D:(i + 1) * D], D, w, 2 * D, D, D),
                         (self.dWh[i * D:(i + 1) * D] if g != "o" else self.dWo, D, w[:, D:], 2 * D, D, D),
                         (self.db[i * D:(i + 1) * D], D, Gm[f"agg.ConvGRUCell_00.{n}.bias"], D, 1, D)]
            tab = (L.Copy2dEntry * len(ents))()
            blk = 0
            for i, (src, sld, dst, dld, r, c) in enumerate(ents):
                tab[i] = L.Copy2dEntry(src.data_ptr(), dst.data_ptr(), sld, dld, r, c, blk, 0)
                blk += max(1, min(64, (r * c + 1023) // 1024))
            raw = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).clone()
            self._gate_table = (raw.to(self.device), len(ents), blk)
        self.call("dpc_copy2d_multi", *self._gate_table)

    def dropout_masks_of_step(self) -> torch.Tensor:
        """[n_steps, M, D] pre-scaled keep masks the recurrence kernels generated in the LAST train-mode forward (same Philox
        stream at the current draw counter, materialised by dpc_dropout_mask): diagnostics and tests."""
        buf = self.empty((self.n_steps, self.M, self.D), torch.float32)
        self.call("dpc_dropout_mask", buf, buf.numel(), float(self.p_drop), self.seed, self.dev_draw)
        return buf

    def _finish_buffers(self):
        widths, dt, f32 = self.widths, self.cdtype, torch.float32
        prs = C.c_int32(0)  # stem backward: partial rows of the pooled reduction (sized by query, not by coincidence)
        ps_ = self.pool_shape
        self.lib.call("dpc_pooled_bn_bwd_reduce", None, None, None, L.dtype_code(dt), ps_[0] * ps_[1] * ps_[2] * ps_[3], widths[0],
                      None, None, None, C.byref(prs), self.lib.stream())
        self.need_stats(prs.value * 2 * widths[0])
        self.coef = self.empty((2, max(widths)), f32)
        self.stats = self.empty((max(self._stats_need, 1),), f32)
        self.part = self.empty((max(self._part_need, 1),), f32)
        # stem backward: fused weight gradient when asked for and the kernel serves the shape (bf16, image >= 96 px wide), else dz + generic path
        ns = C.c_int32(0)
        self._stem_fused = False
        if dt == torch.bfloat16 and self._want_stem_fused:
            try:
                self._stem_fused = self.lib.call("dpc_stem_wgrad_fused", C.byref(self.stem.desc_w), None, None, None, None, None, None, None,
                                                 None, None, C.byref(ns), self.lib.stream()) == 0
            except L.DpcError:
                self._stem_fused = False
        if self._stem_fused:
            self.need_part(ns.value * widths[0] * 256)
            self.part = self.empty((max(self._part_need, 1),), f32)
            self.stem_dz = None
        else:
            self.stem_dz = self.empty(tuple(self.stem.raw.shape), dt)
        self.packed_for_step = -1

    # ------------------------------------------------------------------ plumbing
    # split-K slab workspace: one buffer per stream.  Launches issued inside side() get the side stream's own slabs, so a
    # main-stream user (dpc_gemm_*_splitk, dpc_colsum, a weight gradient that stays on the main stream with need_dx=False) can never overwrite slabs a side-stream weight gradient is still reducing.
    @property
    def part(self) -> torch.Tensor:
        return self._part_side if self._on_side else self._part_main

    @part.setter
    def part(self, t: torch.Tensor):
        self._part_main = t
        self._part_side = torch.empty_like(t) if self._side is not None else t

    def empty(self, shape, dtype):
        return torch.empty(tuple(shape), dtype=dtype, device=self.device)

    def need_stats(self, n):
        self._stats_need = max(self._stats_need, int(n))

    def need_part(self, n):
        self._part_need = max(self._part_need, int(n))

    def _need_wgrad(self, M, Co, K):
        d = self._gemm_desc(M, Co, K, K, K, Co, out_f32=True)
        ns = C.c_int32(0)
        self.lib.call("dpc_conv_wgrad", C.byref(d), None, None, (Co + 7) // 8 * 8, None, C.byref(ns), self.lib.stream())
        self.need_part(ns.value * Co * K)

    def call(self, name, *args):
        self._launches += 1
        if getattr(self.lib, "_f32_mode", 0) != self._x6:   # process-wide library state, read when a launch is planned: keep it ours
            self.lib.call("dpc_set_f32_matmul", self._x6)
            self.lib._f32_mode = self._x6
        tm = self.timer
        if tm is not None and name in tm.names:
            return tm.timed(self, name, args)
        return self.lib.call(name, *args, self.lib.stream())

    @contextlib.contextmanager
    def tag(self, name: str):
        """labels the launches made inside the block for KernelTimer (bench.py: score-GEMM roofline)"""
        prev, self._tag = self._tag, name
        try:
            yield
        finally:
            self._tag = prev

    def scratch(self, shape, exclude):
        """gradient scratch of a given activation shape; a handful live per shape by construction.  Buffers a side-stream launch
        may still be reading (side()) are passed over; when the pool has nothing else the oldest side generation is retired first
        (the main stream waits for its event -- long complete by then)."""
        pool = self._scratch.setdefault(tuple(shape), [])

        def free():
            for t in pool:
                if all(t is not x for x in exclude if x is not None) and all(t is not b for _, bufs in self._busy for b in bufs):
                    return t
            return None
        t = free()
        while t is None and self._busy:
            ev, _ = self._busy.pop(0)
            torch.cuda.current_stream(self.device).wait_event(ev)
            t = free()
        if t is None:
            t = self.empty(shape, self.cdtype)
            pool.append(t)
        return t

    # ---- weight gradients on a second stream.  A weight gradient and the input-gradient of the same unit both read the unit's
    # output gradient and nothing depends on the weight gradient until the optimizer.  Launches inside side() go to the side
    # stream, ordered after everything issued on the main stream so far; `reads` are the scratch buffers they read, kept out of
    # scratch() until the main stream has waited for the event recorded behind them.  Captured into the step's hipGraph as a
    # fork / join.  Two rules came out of the measurements (profiles/r03_two_stream.txt):
    #   * a weight gradient runs beside the NEXT unit's BatchNorm backward (HBM-bound, no LDS), not beside an input-gradient
    #     (LDS-bound like itself): the main stream waits for the side stream before every input-gradient (_ConvBN.dgrad).  Pairs in
    #     isolation (scripts/probes/overlap_probe.py): layer2 531 -> 430 us, layer1 736 -> 705, layer3 509 -> 482; the step: cfg2
    #     27.48 -> 26.5 ms (+3.6 %), cfg4 +3.9 %, cfg5 +3.2 %; without the wait only +1.6 %.
    #   * without that wait the schedule is NOT bit-reproducible: scripts/stream_stress.py (two engines, one per schedule, compared
    #     bit for bit after every step) then finds, about once per 300-500 steps, a step whose gradients differ from the output of
    #     a layer2 / layer3 input-gradient upwards.  scripts/probes/corun_probe.py found the pair that does it: igemm_ws_kernel with
    #     reduce_unpack_t (8 KB of LDS: the one kernel whose workgroups fit on a CU beside igemm_ws's 144 KB) on the same CU --
    #     one compute wave's block of a tile wrong in 38 of 15 000 launches; the persistent kernels now claim all 160 KB of LDS
    #     and the probe is clean (conv_igemm_ws.hip).  The wait in _ConvBN.dgrad stays for the throughput.  With it, 9 600 steps (three configurations, graph
    #     replay and kernel-by-kernel) were bit-identical to the one-stream schedule.
    @contextlib.contextmanager
    def side(self, reads=(), site: str = ""):
        # instrumented pass (bench.py): one stream, clean per-kernel times.  side_off: sites whose launches stay on the main stream
        if self._side is None or self.timer is not None or site in self.side_off:
            yield
            return
        main = torch.cuda.current_stream(self.device)
        ev = torch.cuda.Event()
        ev.record(main)
        self._side.wait_event(ev)
        with torch.cuda.stream(self._side):
            self._on_side = True
            try:
                yield
            finally:
                self._on_side = False
            done = torch.cuda.Event()
            done.record(self._side)
        self._busy.append((done, [t for t in reads if t is not None]))
        if self._capture_events is not None:   # recorded into a hipGraph being captured: see capture_train_step
            self._capture_events += [ev, done]

    def side_wait(self):
        """the main stream waits for the side stream's work so far; its buffers stay tracked"""
        if self._busy:
            torch.cuda.current_stream(self.device).wait_event(self._busy[-1][0])

    def side_join(self):
        """the main stream waits for everything issued on the side stream; its buffers are free again"""
        if self._busy:
            torch.cuda.current_stream(self.device).wait_event(self._busy[-1][0])   # the side stream runs in order
            self._busy.clear()

    def _gemm_desc(self, M, N, K, lda, ldb, ldo, out_f32=True):
        dc = L.dtype_code(self.cdtype)
        return L.ConvDesc(dc, L.F32 if out_f32 else dc, 0, M, 1, 1, 1, 1, 1, 1, K, lda, N, ldb, ldo, 1, 1, 1, 1, 1, 1, 0, 0, 0)

    def gemm(self, A, Bm, out, M, N, K, lda=None, ldb=None, ldo=None, addend=None, out_f32=True):
        """out[M][N] = A[M][K] @ Bm[N][K]^T (+ addend) on the matrix cores"""
        d = self._gemm_desc(M, N, K, lda or K, ldb or K, ldo or N, out_f32)
        self.call("dpc_conv_igemm", C.byref(d), A, Bm, out, addend, None)

    def gemm_splitk(self, A, Bm, out, M, N, K, lda, ldb):
        """out[M][N] (f32) = A[M][K] @ Bm[N][K]^T with the reduction split over workgroups (small output, long K)"""
        ns = C.c_int32(0)
        self.call("dpc_gemm_nt_splitk", L.dtype_code(self.cdtype), M, N, K, A, lda, Bm, ldb, self.part, C.byref(ns))
        self.call("dpc_reduce_unpack", self.part, ns.value, out, M, 1, N, N, 0, 1, 0)

    def gemm_tn(self, dy, dy_ld, X, x_ld, out, M, Co, K):
        """out[Co][K] = dy[M][Co]^T @ X[M][K] (f32), split-K + deterministic reduce"""
        d = self._gemm_desc(M, Co, K, x_ld, K, Co)
        ns = C.c_int32(0)
        self.call("dpc_conv_wgrad", C.byref(d), X, dy, dy_ld, self.part, C.byref(ns))
        self.call("dpc_reduce_unpack", self.part, ns.value, out, Co, 1, K, K, 0, 1, 0)

    # ------------------------------------------------------------------ parameters
    def load_params(self, params: Dict[str, torch.Tensor]):
        """copy a reference-layout state_dict (alias / module. prefixes tolerated) into the flat arena"""
        self._not_swapped("load_params")
        for k, v in params.items():
            k = k[7:] if k.startswith("module.") else k
            if k.startswith("agg.cell_list.0."):
                continue  # alias of agg.ConvGRUCell_00 (backbone/convrnn.py:55-58)
            dst, shp = self.PRM.get(k), self.shapes.get(k)
            if dst is None or shp is None:   # (a bare KeyError(k) here was seen once in a full GPU-tier run and never again: say more)
                raise KeyError(f"{k}: not a parameter of this {self.network} engine ({len(self.PRM)} parameters, {len(self.shapes)} shapes, "
                               f"in PRM: {k in self.PRM}, in shapes: {k in self.shapes})")
            dst.copy_(v.to(torch.float32).reshape(shp))
        self.packed_for_step = -1
        if self._ema is not None:   # an external write of the parameters restarts their average
            self.flat_ema.copy_(self.flat_p)

    def adopt_optimizer_state(self, old: "BackboneEngine"):
        """continue `old`'s optimisation in this engine (same network, any batch / compute dtype / device): Adam moments, the
        optimizer-step counter with its device-side bias corrections, the dropout draw counter, lr / weight decay.  The module
        boundary rebuilds its engine when the batch size, model.bfloat16() / .float() or the device change (model._ensure_engine);
        torch.optim.Adam over the same Parameters would keep its state through all three."""
        if old.numel != self.numel or list(old.offsets) != list(self.offsets):
            raise ValueError("adopt_optimizer_state: the engines hold different parameter sets")
        self.flat_m.copy_(old.flat_m)
        self.flat_v.copy_(old.flat_v)
        self.dev_step.copy_(old.dev_step)
        self.dev_bc.copy_(old.dev_bc)
        self.dev_draw.copy_(old.dev_draw)
        self._step_count, self._steps_unsure = old._step_count, old._steps_unsure
        self.lr, self.wd = old.lr, old.wd
        if old.param_groups:
            self.set_param_groups(old.param_groups)
        if old._guard_state is not None:   # the guard's settings and its counters
            self._guard_alloc()
            self._guard_state.copy_(old._guard_state)
            self._guard = old._guard
        if old.flat_ema is not None:   # the average and its setting
            old._not_swapped("adopt_optimizer_state")
            self._ema_alloc()
            self.flat_ema.copy_(old.flat_ema)
            self._ema = old._ema
        if old._lr_desc is not None:   # the schedule and the record of its last step
            self._lr_alloc()
            self._lr_state.copy_(old._lr_state)
            self._lr_sched, self._lr_desc = old._lr_sched, old._lr_desc
        if old._opt_kind != "adam":   # the update rule, its tables and (LAMB) the records of its last step
            self.set_optimizer(old._opt_kind, old._opt_x1d)
            if old._lamb is not None and self._lamb is not None:
                self._lamb["records"].copy_(old._lamb["records"])
        if old.flat_acc is not None:   # the accumulation: its setting, the sum so far and the position in the cycle
            self._accum_alloc()
            self.flat_acc.copy_(old.flat_acc)
            self._accum_n, self._accum_pos = old._accum_n, old._accum_pos
        self.packed_for_step = -1

    def state_dict(self) -> Dict[str, torch.Tensor]:
        self._not_swapped("state_dict")
        self._not_mid_cycle("state_dict")
        sd = {k: v.detach().clone() for k, v in self.PRM.items()}
        for k in list(sd):
            if k.startswith("agg.ConvGRUCell_00."):
                sd[k.replace("agg.ConvGRUCell_00.", "agg.cell_list.0.")] = sd[k]
        return sd

    def pack_weights(self):
        if self.packed_for_step == self._step_count:
            return
        dc = L.dtype_code(self.cdtype)
        if self._pack_table is None:  # static: built once (addresses and shapes never change)
            ents = [e for u in self.units if not u.stem for e in u.pack_entries()]
            tab = (L.PackEntry * len(ents))()
            blk = 0
            for i, (src, dst, d0, d1, d2, s0, s1, s2) in enumerate(ents):
                tab[i] = L.PackEntry(src.data_ptr(), dst.data_ptr(), d0, d1, d2, blk, s0, s1, s2)
                blk += max(1, min(1024, (d0 * d1 * d2 + 511) // 512))   # (an eighth of the workgroups: measured neutral, round 4)
            raw = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).clone()
            self._pack_table = (raw.to(self.device), len(ents), blk)
        tab_dev, n_ent, n_blk = self._pack_table
        self.call("dpc_pack_stem_weight", self.PRM[self.stem.wname], self.stem.wp, dc, self.stem.Co)
        self.call("dpc_pack3d_multi", tab_dev, n_ent, n_blk, dc)
        Pm = self.PRM
        self.call("dpc_gru_pack", Pm["agg.ConvGRUCell_00.update_gate.weight"], Pm["agg.ConvGRUCell_00.reset_gate.weight"],
                  Pm["agg.ConvGRUCell_00.out_gate.weight"], Pm.get("network_pred.0.weight"), Pm.get("network_pred.2.weight"), self.D, dc,
                  self.gru_packed)
        self.packed_for_step = self._step_count

    # ------------------------------------------------------------------ forward
    def load_frames(self, frames: torch.Tensor, aug: torch.Tensor, gray: Optional[torch.Tensor], ds: int = 3):
        """GPU-side input pipeline (dpc_amd/data.py): decoded uint8 frames [B,F,H0,W0,3] + the loader's per-clip draws ->
        the stem's operand, without an f32 video in between.  Follow with forward(None, ...) / train_step(None, ...)."""
        from .data import frames_to_input
        frames_to_input(self.lib, frames, aug, gray, self.N, self.SL, ds, self.size, None, self.x_s2d)

    def load_recipe(self, frames: torch.Tensor, starts, clips, ds: int = 3):
        """the reference's full training transform (dpc/main.py:114-132: crop / resized crop, flip, RandomGray, ColorJitter, ToTensor,
        Normalize) on the GPU: decoded uint8 frames [B,F,H0,W0,3] + one data.draw_k400 / data.draw_ucf101 result per clip -> the
        stem's operand.  Follow with forward(None, ...) / train_step(None, ...)."""
        from .data import recipe_to_input
        recipe_to_input(self.lib, frames, starts, clips, self.N, self.SL, ds, self.size, None, self.x_s2d)

    def resident_reserve(self) -> int:
        """bytes this engine still allocates once frames are resident: load_resident's two jitter workspaces, and an allowance
        of 1 GiB for the gradient scratch and graph pools that the first steps and a capture fill lazily"""
        n = self.B * self.N * self.SL
        return n * self.size * self.size * 3 + n * 8 + (1 << 30)

    def load_resident(self, source):
        """one batch from frames resident in HBM (data.ResidentFrameSource): advance the source's cursor and draw counter, draw the
        recipe on the device (dpc_draw_recipe), gather from the store into the stem's operand (dpc_store_to_input).  Six launches
        (two counters, the draw, the gather's three; its one without ColorJitter); no host synchronisation, no host-to-device copy, no allocation after the
        first call, no address that changes: graph-safe as the `refill` of capture_train_step / capture_eval_step, and one capture
        serves every epoch.  A source with labels (data.ResidentLabelledSource) has them gathered into ``self.target`` by the draw's
        launch (dpc_draw_recipe_ex): no set_labels, no further launch.  Follow with forward(None, ...) / train_step(None, ...)."""
        from .data import store_to_input
        if source.batch != self.B or source.N != self.N or source.SL != self.SL or source.size != self.size or source.device != self.device:
            raise ValueError("the source was built for another batch / clip shape / device than this engine")
        if source.has_jitter and self._resident_ws is None:   # allocated once, shared by every source of this engine
            n = self.B * self.N * self.SL
            self._resident_ws = (torch.empty(n * self.size * self.size * 3, dtype=torch.uint8, device=self.device),
                                 torch.empty(n, dtype=torch.int64, device=self.device))
        u8, ls = self._resident_ws if source.has_jitter else (None, None)
        self.call("dpc_counter_advance", source.cursor)
        self.call("dpc_counter_advance", source.draw)
        target = None
        if source.labels_dev is not None:   # data.ResidentLabelledSource: the draw's launch gathers the batch's labels as well
            target = getattr(self, "target", None)
            if target is None:
                raise ValueError("the source carries labels but this engine has no `target` to receive them (LCEngine has)")
        source.draw_recipe(self.lib, call=self.call, target=target)
        store_to_input(self.lib, source.store.dev, source.aug, source.clip_first, source.gray, source.rs,
                       source.jitter if source.has_jitter else None, self.N, self.SL, source.ds, self.size, None, self.x_s2d, u8, ls,
                       call=self.call)

    def fill_synthetic(self, seed: int, block: Optional[torch.Tensor] = None):
        """a new synthetic N(0,1) batch drawn on the device (csrc/synthetic.hip): advances dev_input, then writes the stem's operand
        (and `block` [B,N,3,SL,H,W] f32 with the same values when given).  Follow with forward(None, ...) / train_step(None, ...).
        Graph-safe: captured in front of a step (capture_train_step / capture_eval_step refill=) it draws a new batch per replay."""
        if block is not None and (tuple(block.shape) != (self.B, self.N, 3, self.SL, self.size, self.size) or block.dtype != torch.float32
                                  or not block.is_contiguous() or block.device != self.device):
            raise ValueError(f"block must be a contiguous float32 {(self.B, self.N, 3, self.SL, self.size, self.size)} on {self.device}")
        self.call("dpc_counter_advance", self.dev_input)
        self.call("dpc_synthetic_input", block, self.x_s2d, L.dtype_code(self.cdtype), self.B * self.N, self.SL, self.size, self.size,
                  int(seed) & 0xFFFFFFFFFFFFFFFF, self.dev_input)

    def _backbone_forward(self, block: Optional[torch.Tensor]) -> torch.Tensor:
        """2d3d-ResNet (backbone/resnet_2d3d.py:259-270) on block [B,N,3,SL,H,W] (None: the stem operand was filled by
        load_frames): returns the last block's output [B*N, T, ls, ls, D] (channels-last, no final ReLU)"""
        B, N = self.B, self.N
        dc = L.dtype_code(self.cdtype)
        with self.side(site="pack"):   # the per-step weight repacks (0.2 ms of small launches) beside the input pack
            self.pack_weights()
        if block is not None:
            self.call("dpc_pack_input_s2d", block.contiguous(), self.x_s2d, dc, B * N, self.SL, self.size, self.size)
        self.side_join()
        self.stem.forward(self.x_s2d)
        st = self.stem.out_shape
        self.call("dpc_bn_relu_maxpool_fwd", self.stem.raw, dc, st[0] * st[1], st[2], st[3], self.widths[0], self.stem.scale,
                  self.stem.shift, self.pooled, self.pool_arg)
        x = self.pooled
        for blk in self.blocks:
            x = blk.forward(x)
        return x

    def _backbone_backward(self, d: torch.Tensor, on_tail_ready=None):
        """backward of _backbone_forward from d = d loss / d (last block output); fills the backbone's gradients"""
        carved = False
        for bi in reversed(range(len(self.blocks))):
            if on_tail_ready is not None and bi == self.n_head_blocks - 1:
                self.side_join()   # the tail's weight gradients are complete before its all-reduce starts
                on_tail_ready(self.flat_g[self.grad_split:])
                if self.reserve_cus:  # the all-reduce of the tail is in flight from here to the end of the backward pass
                    self.lib.call("dpc_set_reserved_cus", self.reserve_cus)
                    carved = True
            d = self.blocks[bi].backward(d, need_dx=True)
        if carved:
            self._carved = True
        self._stem_backward(d)

    def _stem_backward(self, d: torch.Tensor):
        """backward of the stem from d = d loss / d (pooled output): fills the gradients of conv1 and bn1"""
        dc = L.dtype_code(self.cdtype)
        # stem: max-pool routing (ReLU mask folded into the saved argmax) -> BN -> weight grad; the video has no grad
        st = self.stem.out_shape
        u, C0 = self.stem, self.widths[0]
        pr = C.c_int32(0)
        ps = self.pool_shape
        self.call("dpc_pooled_bn_bwd_reduce", d, self.pool_arg, self.pooled, dc, ps[0] * ps[1] * ps[2] * ps[3], C0,
                  self.PRM[u.bnname + ".weight"], self.PRM[u.bnname + ".bias"], self.stats, C.byref(pr))
        self.call("dpc_bn_bwd_finalize", self.stats, pr.value, C0, float(u.rows), self.G[u.bnname + ".weight"],
                  self.G[u.bnname + ".bias"], self.coef)
        self.side_join()   # the stem's weight gradient uses the same split-K slab buffer; everything is on one stream again
        if self._stem_fused:  # BN backward + pool routing inside the weight-gradient kernel: no 2.7 GB dz tensor (csrc/conv_wgrad_stem.hip)
            ns = C.c_int32(0)
            self.call("dpc_stem_wgrad_fused", C.byref(u.desc_w), self.x_s2d, u.raw, d, self.pool_arg, u.mean, u.invstd,
                      self.PRM[u.bnname + ".weight"], self.coef, self.part, C.byref(ns))
            self.call("dpc_unpack_stem_wgrad", self.part, ns.value, self.G[u.wname], C0)
            self._uncarve()
            return
        self.call("dpc_pool_bn_bwd_apply", d, self.pool_arg, u.raw, dc, st[0] * st[1], st[2], st[3], C0, u.mean, u.invstd,
                  self.PRM[u.bnname + ".weight"], self.coef, self.stem_dz)
        self.stem.wgrad(self.x_s2d, self.stem_dz)
        self._uncarve()

    def _uncarve(self):
        if self._carved:
            self.lib.call("dpc_set_reserved_cus", 0)
            self._carved = False

    @property
    def step_count(self) -> int:
        """completed optimizer steps (host mirror of dev_step).  The gradient guard drops a non-finite step on the device, so while
        it may have done so the mirror is refreshed from dev_step here -- one read-back where somebody asks (a checkpoint, a probe),
        none in the step."""
        if self._steps_unsure:
            t = int(self.dev_step.item())
            if t != self._step_count:
                self._step_count = t
                self.packed_for_step = -1   # (the re-pack cache is keyed on the mirror: do not let the new value match an old key)
            self._steps_unsure = False
        return self._step_count

    @step_count.setter
    def step_count(self, t: int):  # checkpoint resume: host value -> device counter
        self._step_count, self._steps_unsure = int(t), False
        self.dev_step.fill_(int(t))
        # one draw per forward in the engine-owned loop, set_grad_accum(N) forwards per optimizer step: a resumed run continues the
        # same mask stream
        self.dev_draw.fill_(int(t) * self._accum_n)

    def set_param_groups(self, groups=None):
        """Parameter groups of the fused Adam (torch.optim.Adam over several groups: eval/test.py:76-84 gives every parameter its own).
        groups: an iterable of dicts {'params': [parameter names], 'lr': float, 'weight_decay': float, 'frozen': bool (default False)};
        a parameter named by no group is frozen, as is every parameter of a 'frozen' group: the update neither reads nor writes its
        slices of the four arenas (torch skips a parameter without a gradient the same way).  None / () returns to the one-group
        update (``self.lr`` / ``self.wd`` over the whole arena, dpc_adam_dev).

        The segment table (csrc/loss.hip: dpc_adam_groups_dev) is built from ``self.offsets``, adjacent parameters with equal
        values merged into one segment, and uploaded here -- only when a host value differs from what the device holds, so an lr
        schedule that calls this once per epoch costs one small copy per change and a caller that passes the same values every
        step costs none.  Never call it while a graph is being captured (the upload is a host-to-device copy).  The table lives in
        one device buffer whose address never changes; a captured step (capture_train_step) counts the table among the
        values baked into it, so a replay after the groups changed raises instead of stepping with another table.

        ONE step counter serves all groups: a parameter that is frozen for the first k steps and trained afterwards is updated
        with the shared bias corrections 1 - beta^t of the run, where torch, which counts steps per parameter, would restart it at
        t = 1.  (Its moments do start from zero either way.)"""
        if not groups:
            self._groups, self._groups_key, self._seg_host, self._seg_n = None, None, None, 0   # (the device buffer stays: a captured step may hold its address)
            return
        key = tuple((tuple(g["params"]), float(g["lr"]), float(g.get("weight_decay", 0.0)), bool(g.get("frozen", False))) for g in groups)
        if key == self._groups_key:   # the values of the last call (an optimizer that passes its groups at every step): nothing to rebuild
            return
        names = list(self.offsets)
        per_param: Dict[str, Tuple[float, float, bool]] = {}
        norm = []
        for g in groups:
            lr, wd, frozen = float(g["lr"]), float(g.get("weight_decay", 0.0)), bool(g.get("frozen", False))
            if not (lr >= 0.0) or not (wd >= 0.0):   # (NaN fails both)
                raise ValueError(f"set_param_groups: lr and weight_decay must be non-negative numbers, got lr={lr}, weight_decay={wd}")
            ks = list(g["params"])
            for k in ks:
                if k not in self.offsets:
                    raise KeyError(f"set_param_groups: {k} is not a parameter of this engine")
                if k in per_param:
                    raise ValueError(f"set_param_groups: {k} appears in more than one parameter group")
                per_param[k] = (lr, wd, not frozen)
            norm.append({"params": ks, "lr": lr, "weight_decay": wd, "frozen": frozen})
        segs = []   # [begin, end, lr, wd, active] in arena order; a parameter's slice is rounded up to its 16-byte slot
        for k in names:
            o, n = self.offsets[k]
            lr, wd, active = per_param.get(k, (0.0, 0.0, False))
            if not active:
                lr = wd = 0.0
            e = o + (n + 3) // 4 * 4
            if segs and segs[-1][1] == o and tuple(segs[-1][2:]) == (lr, wd, active):
                segs[-1][1] = e
            else:
                segs.append([o, e, lr, wd, active])
        prev = 0
        for b, e, _, _, _ in segs:   # the table is validated where it is built: sorted, 16-byte aligned, inside the arena
            if b % 4 or e % 4 or b < prev or e <= b or e > self.numel:
                raise ValueError(f"set_param_groups: bad segment [{b}, {e}) in an arena of {self.numel} floats")
            prev = e
        if len(segs) > L.ADAM_MAX_SEGMENTS:
            raise ValueError(f"set_param_groups: {len(segs)} segments, the kernel's table holds {L.ADAM_MAX_SEGMENTS}")
        tab = (L.AdamSegment * len(segs))()
        for i, (b, e, lr, wd, active) in enumerate(segs):
            tab[i] = L.AdamSegment(b, e, lr, wd, int(active), 0)
        host = bytes(tab)
        self._groups, self._groups_key = norm, key
        if host != self._seg_host:
            if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise L.DpcError("set_param_groups: the segment table changed while a graph is being captured")
            if self._seg_dev is None:   # ONE device buffer of the kernel's capacity for the engine's life: its address never changes
                self._seg_dev = torch.zeros(L.ADAM_MAX_SEGMENTS * C.sizeof(L.AdamSegment), dtype=torch.uint8, device=self.device)
            raw = torch.frombuffer(bytearray(host), dtype=torch.uint8)
            self._seg_dev[:raw.numel()].copy_(raw)
            self._seg_host, self._seg_n = host, len(segs)
            self.seg_uploads += 1

    @property
    def param_groups(self):
        """what set_param_groups was given last (normalised), or None: the one-group update"""
        return self._groups

    def frozen_params(self):
        """names of the parameters the grouped update leaves alone (empty without groups)"""
        if not self.param_groups:
            return []
        live = {k for g in self._groups if not g["frozen"] for k in g["params"]}
        return [k for k in self.offsets if k not in live]

    def set_grad_guard(self, max_norm: Optional[float] = None, skip_nonfinite: bool = False):
        """Gradient guard of the fused Adam (csrc/grad_guard.hip), decided on the device between the gradient exchange and the update:
        max_norm: clip the gradient's global 2-norm over the live parameters (those the grouped update would touch) to it, by torch's
        clip_grad_norm_ formula, the factor folded into the update -- flat_g itself is not rewritten; skip_nonfinite: an Inf or NaN
        anywhere in the live gradient suppresses the whole step -- flat_p / flat_m / flat_v, dev_step and the bias corrections keep
        their bits, and the step does not count as an optimizer step.  The defaults turn the guard off: adam_step() then launches
        exactly what it launched without it.

        The partial sums and the 32-byte verdict record (zeroed) are allocated at the first enabling -- do that before a step is
        captured, a captured step allocates nothing.  The settings are among the scalars a captured step bakes in: a replay after they
        changed raises.  grad_stats() reads the record."""
        if max_norm is not None:
            max_norm = float(max_norm)
            if not (math.isfinite(max_norm) and max_norm > 0.0):
                raise ValueError(f"set_grad_guard: max_norm must be None or a finite positive number, got {max_norm}")
        guard = (max_norm, bool(skip_nonfinite)) if (max_norm is not None or skip_nonfinite) else None
        if guard is not None:
            self._guard_alloc()
        self._guard = guard

    def _guard_alloc(self):
        if self._guard_state is None:
            if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise L.DpcError("set_grad_guard: enable the guard before a step is captured (it allocates its device record)")
            self._guard_partials = torch.zeros(L.GRAD_PARTIALS, dtype=torch.float64, device=self.device)
            self._guard_state = torch.zeros(C.sizeof(L.GradState), dtype=torch.uint8, device=self.device)

    @property
    def grad_guard(self):
        """(max_norm or None, skip_nonfinite), or None while the guard is off"""
        return self._guard

    def grad_stats(self) -> dict:
        """the guard's verdict on the last guarded step and its running counts: norm, coef, skip, n_skipped, n_clipped, sumsq.
        One 32-byte device-to-host copy; the step itself never calls it."""
        if self._guard_state is None:
            raise RuntimeError("grad_stats: the gradient guard was never enabled (set_grad_guard)")
        st = L.GradState.from_buffer_copy(self._guard_state.cpu().numpy().tobytes())
        return {"norm": st.norm, "coef": st.coef, "skip": st.skip, "n_skipped": st.n_skipped, "n_clipped": st.n_clipped, "sumsq": st.sumsq}

    # ------------------------------------------------------------------ EMA of the parameters (csrc/loss.hip, the _ema entries)
    def set_ema(self, decay: Optional[float] = None):
        """Exponential moving average of the parameters, kept by the fused Adam itself: the thread that has just updated a 16-byte unit
        of flat_p does ``e += (1 - d) (p_new - e)`` on the same unit of ``flat_ema``, d = min(decay, (1 + t) / (10 + t)) with t the
        optimizer-step count after this step (the usual warm-up, always on).  No launch, no graph node and no collective of its own:
        every rank updates the same bits.  A step the gradient guard skips and a frozen parameter leave the average untouched.
        decay=None (the default) turns it off: adam_step() then launches exactly what it launched without it, and flat_ema -- once
        allocated -- keeps its values until the average is turned on again.

        ``flat_ema`` is allocated and seeded with a copy of flat_p at the first enabling -- before a step is captured, a captured step
        allocates nothing.  load_params() re-seeds it while the average is on.  The decay is among the scalars a captured step bakes
        in: a replay after it changed raises.  Only parameters are averaged: the running buffers of the LC classifier's BatchNorm
        (``BUF``) are shared between the raw and the averaged model.  Read the average with ema_state_dict(), evaluate with it inside
        ``with eng.ema_weights():``."""
        if decay is not None:
            decay = float(decay)
            if not 0.0 < decay < 1.0:
                raise ValueError(f"set_ema: decay must be None or lie in (0, 1), got {decay}")
            self._not_swapped("set_ema")
            self._ema_alloc()
        self._ema = decay

    def _ema_alloc(self):
        if self.flat_ema is None:
            if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise L.DpcError("set_ema: enable the average before a step is captured (it allocates its arena)")
            self.flat_ema = self.flat_p.detach().clone()

    @property
    def ema_decay(self) -> Optional[float]:
        """the decay, or None while the average is off"""
        return self._ema

    def _not_swapped(self, what: str):
        if self._ema_swapped:
            raise RuntimeError(f"{what}: flat_p holds the averaged weights (swap_ema / ema_weights); swap back first")

    def swap_ema(self):
        """exchange flat_p and flat_ema in place (dpc_arena_swap: one launch, a bit copy).  ``PRM``, the pack tables and every captured
        graph keep their addresses and now see the averaged weights; a second call puts everything back, bit for bit.  While the arenas
        are exchanged only evaluation is allowed: adam_step, train_step, a train-step replay, state_dict(), ema_state_dict() and the
        checkpoint writers raise.  An eval-step replay repacks inside the graph, so it evaluates whatever is in flat_p."""
        if self.flat_ema is None:
            raise RuntimeError("swap_ema: the parameter average was never enabled (set_ema)")
        self._not_mid_cycle("swap_ema")
        self.call("dpc_arena_swap", self.flat_p, self.flat_ema, self.numel)
        self._ema_swapped = not self._ema_swapped
        self.packed_for_step = -1

    @contextlib.contextmanager
    def ema_weights(self):
        """``with eng.ema_weights():`` -- forward / evaluate with the averaged parameters (and, for LC, the shared running buffers)"""
        self._not_swapped("ema_weights")
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """state_dict() over flat_ema (alias keys included; running buffers, which are not averaged, as state_dict() gives them).
        No swap."""
        if self.flat_ema is None:
            raise RuntimeError("ema_state_dict: the parameter average was never enabled (set_ema)")
        sd = self.state_dict()
        for k, (o, n) in self.offsets.items():
            sd[k] = self.flat_ema[o:o + n].detach().clone().view(self.shapes[k])
        for k in sd:
            if k.startswith("agg.cell_list.0."):
                sd[k] = sd[k.replace("agg.cell_list.0.", "agg.ConvGRUCell_00.")]
        return sd

    # ------------------------------------------------------------------ per-step learning-rate schedule (csrc/loss.hip, the _sched entries)
    def set_lr_schedule(self, schedule=None):
        """Learning-rate multiplier evaluated on the device, once per optimizer step, by the thread that advances the step counter
        (dpc_step_advance_sched) and read by the update of the same step: every parameter group steps with ``lr_group * mult(k)``,
        k = completed optimizer steps (dev_step before the advance).  schedule: a dpc_amd.optim.LRSchedule (warm-up, then constant /
        cosine / linear / multistep; optim.lr_multiplier is the same function on the host), or None (the default) to turn it off:
        adam_step() then launches exactly what it launched without it.  ``self.lr`` and the groups' lrs stay the BASE values.

        No launch, graph node, collective or host work per step is added, so it works in a replayed step; every rank evaluates the
        same function of the same count.  A step the gradient guard skips does not advance the schedule; a resumed run continues it
        from the checkpoint's step count.  The 16-byte record {mult, k} is allocated at the first enabling -- before a step is
        captured, a captured step allocates nothing.  The descriptor travels by value in the kernel arguments, so it is among the
        scalars a captured step bakes in: a replay after it changed raises.  lr_now() reads the record."""
        if schedule is None:
            self._lr_sched, self._lr_desc = None, None
            return
        desc = schedule.descriptor()
        if not isinstance(desc, L.LrSchedule):
            raise TypeError("set_lr_schedule: schedule.descriptor() must give a dpc_amd._lib.LrSchedule")
        self._lr_alloc()
        self._lr_sched, self._lr_desc = schedule, desc

    def _lr_alloc(self):
        if self._lr_state is None:
            if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise L.DpcError("set_lr_schedule: enable the schedule before a step is captured (it allocates its device record)")
            host = torch.frombuffer(bytearray(bytes(L.LrState(mult=1.0, k=-1))), dtype=torch.uint8)   # (no step taken yet)
            self._lr_state = host.to(self.device)

    @property
    def lr_schedule(self):
        """the schedule set_lr_schedule was given, or None while it is off"""
        return self._lr_sched

    def lr_now(self) -> dict:
        """the multiplier the last scheduled step used: {'mult', 'k', 'lr'} with lr = float32(self.lr) * mult as the one-group update
        forms it (with parameter groups: the base lr of each group times mult).  k = -1 before the first scheduled step.  One
        16-byte device-to-host copy; the step itself never calls it."""
        if self._lr_state is None:
            raise RuntimeError("lr_now: the learning-rate schedule was never enabled (set_lr_schedule)")
        st = L.LrState.from_buffer_copy(self._lr_state.cpu().numpy().tobytes())
        lr = float(torch.tensor(self.lr, dtype=torch.float32) * torch.tensor(st.mult, dtype=torch.float32))
        return {"mult": st.mult, "k": st.k, "lr": lr}

    def _adam_step_sched(self, grad_scale: float):
        """adam_step() with the schedule on: the eight arms (guard x EMA x groups) through dpc_step_advance_sched and the _sched
        entries, which take the guard's record and the average as nullable arguments -- the launches of the unscheduled arms, one
        for one"""
        st = None
        seg, nseg = (self._seg_dev, self._seg_n) if self._groups else (None, 0)
        if self._guard is not None:
            max_norm, skip_nonfinite = self._guard
            st = self._guard_state
            self.call("dpc_grad_sumsq", self.flat_g, self.numel, seg, nseg, self._guard_partials)
            self.call("dpc_grad_verdict", self._guard_partials, L.GRAD_PARTIALS, max_norm or 0.0, int(skip_nonfinite), st)
        self.call("dpc_step_advance_sched", self.dev_step, self.dev_bc, 0.9, 0.999, st, C.byref(self._lr_desc), self._lr_state)
        ema, step, decay = (self.flat_ema, self.dev_step, self._ema) if self._ema is not None else (None, None, 0.0)
        if self._groups:
            self.call("dpc_adam_groups_dev_sched", self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.numel, seg, nseg,
                      0.9, 0.999, 1e-8, self.dev_bc, grad_scale, st, ema, step, decay, self._lr_state)
        else:
            self.call("dpc_adam_dev_sched", self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.numel, self.lr, 0.9, 0.999, 1e-8,
                      self.wd, self.dev_bc, grad_scale, st, ema, step, decay, self._lr_state)

    # ------------------------------------------------------------------ update rule of the fused step (csrc/optim_kinds.hip)
    def set_optimizer(self, kind: str = "adam", exclude_1d: bool = False):
        """Update rule of the fused step: "adam" (the default: torch.optim.Adam, weight decay folded into the gradient -- adam_step()
        then runs exactly what it ran before this method existed), "adamw" (torch.optim.AdamW: the decay decoupled, one launch as
        Adam) or "lamb" (You et al. 2020, bias-corrected: per parameter tensor the step is scaled by the trust ratio |p| / |u|; three
        launches where Adam has one -- moments and per-chunk norms, per-tensor ratios, apply -- with nothing crossing the host, so it
        works in a replayed step and every rank reaches the same bits without a collective).  The step counter, the gradient guard,
        the parameter average and the learning-rate schedule work under all three.

        exclude_1d (adamw / lamb only): no weight decay on parameters with at most one dimension (biases, BatchNorm), and under lamb
        no trust ratio either (r = 1).  Learning rate, weight decay and frozen parameters come from the parameter groups when there
        are groups, else from ``self.lr`` / ``self.wd``; the tables are rebuilt, and uploaded, when one of those changes -- here or at
        the next adam_step(), never while a graph is being captured (that raises).  The device buffers are allocated once and keep
        their addresses.  Kind, flag and table contents are among the values a captured step bakes in, while the kind is not adam.
        lamb_stats() reads the last step's norms and ratios."""
        if kind not in ("adam", "adamw", "lamb"):
            raise ValueError(f"set_optimizer: kind must be 'adam', 'adamw' or 'lamb', got {kind!r}")
        if exclude_1d and kind == "adam":
            raise ValueError("set_optimizer: exclude_1d needs kind 'adamw' or 'lamb'")
        if (kind, bool(exclude_1d)) == (self._opt_kind, self._opt_x1d):   # (a caller that passes its settings at every step)
            if kind != "adam":
                self._opt_sync()
            return
        self._opt_kind, self._opt_x1d, self._opt_key, self._opt_host = kind, bool(exclude_1d), None, b""
        if kind != "adam":
            self._opt_sync()

    @property
    def optimizer_kind(self) -> str:
        return self._opt_kind

    @property
    def optimizer_exclude_1d(self) -> bool:
        return self._opt_x1d

    def _per_param_hyper(self):
        """[(name, begin, end, lr, weight_decay, active)] in arena order: what the update does with every parameter slot"""
        per = None
        if self._groups:
            per = {k: (g["lr"], g["weight_decay"], not g["frozen"]) for g in self._groups for k in g["params"]}
        rows = []
        for k, (o, n) in self.offsets.items():
            lr, wd, active = per.get(k, (0.0, 0.0, False)) if per is not None else (float(self.lr), float(self.wd), True)
            if not active:
                lr = wd = 0.0
            if self._opt_x1d and len(self.shapes[k]) <= 1:
                wd = 0.0
            rows.append((k, o, o + (n + 3) // 4 * 4, lr, wd, active))
        return rows

    def _opt_upload(self, dst: torch.Tensor, host: bytes):
        raw = torch.frombuffer(bytearray(host), dtype=torch.uint8)
        dst[:raw.numel()].copy_(raw)

    def _opt_sync(self):
        """(re)build the tables of the adamw / lamb step when what they are made from changed; upload what differs"""
        key = (self._opt_kind, self._opt_x1d, float(self.lr), float(self.wd), self._groups_key)
        if key == self._opt_key:
            return
        capturing = self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()
        if self._opt_kind == "adamw" and not self._opt_x1d:   # the one-group update or the groups' own table: nothing of its own
            self._opt_key, self._opt_host = key, b""
            return
        rows = self._per_param_hyper()
        if self._opt_kind == "adamw":
            segs = []
            for _, b, e, lr, wd, active in rows:
                if segs and segs[-1][1] == b and tuple(segs[-1][2:]) == (lr, wd, active):
                    segs[-1][1] = e
                else:
                    segs.append([b, e, lr, wd, active])
            if len(segs) > L.ADAM_MAX_SEGMENTS:
                raise ValueError(f"set_optimizer: {len(segs)} segments, the kernel's table holds {L.ADAM_MAX_SEGMENTS}")
            tab = (L.AdamSegment * len(segs))()
            for i, (b, e, lr, wd, active) in enumerate(segs):
                tab[i] = L.AdamSegment(b, e, lr, wd, int(active), 0)
            host = bytes(tab)
            if host != self._opt_host:
                if capturing:
                    raise L.DpcError("set_optimizer: the optimizer's table changed while a graph is being captured")
                if self._aw_seg_dev is None:
                    self._aw_seg_dev = torch.zeros(L.ADAM_MAX_SEGMENTS * C.sizeof(L.AdamSegment), dtype=torch.uint8, device=self.device)
                self._opt_upload(self._aw_seg_dev, host)
                self._aw_seg_n = len(segs)
            self._opt_key, self._opt_host = key, host
            return
        # lamb: one table entry per parameter slot, and the chunk table that is the work split of its launches
        if len(rows) > L.ADAM_MAX_SEGMENTS:
            raise ValueError(f"set_optimizer: {len(rows)} parameters, the kernel's table holds {L.ADAM_MAX_SEGMENTS}")
        cap = self.numel // L.LAMB_CHUNK + len(rows) + 1
        tab = (L.LambSegment * len(rows))()
        for i, (k, b, e, lr, wd, active) in enumerate(rows):
            adapt = int(active and not (self._opt_x1d and len(self.shapes[k]) <= 1))
            tab[i] = L.LambSegment(b, e, lr, wd, int(active), adapt, 0, 0)
        chunks = (L.LambChunk * cap)()
        nc = self.lib.call("dpc_lamb_build_chunks", tab, len(rows), self.numel, chunks, cap)
        if nc <= 0:
            raise ValueError("set_optimizer: no parameter is trained (every parameter is frozen)")
        seg_host, chunk_host = bytes(tab), bytes(chunks)[:nc * C.sizeof(L.LambChunk)]
        host = seg_host + chunk_host
        if host != self._opt_host:
            if capturing:
                raise L.DpcError("set_optimizer: the optimizer's tables changed while a graph is being captured")
            if self._lamb is None:   # allocated once, for the engine's life: a captured step holds these addresses
                u8 = dict(dtype=torch.uint8, device=self.device)
                self._lamb = {"seg": torch.zeros(L.ADAM_MAX_SEGMENTS * C.sizeof(L.LambSegment), **u8),
                              "chunks": torch.zeros(cap * C.sizeof(L.LambChunk), **u8),
                              "partials": torch.zeros(2 * cap, dtype=torch.float64, device=self.device),
                              "records": torch.zeros(L.ADAM_MAX_SEGMENTS * C.sizeof(L.LambRecord), **u8)}
            self._opt_upload(self._lamb["seg"], seg_host)
            self._opt_upload(self._lamb["chunks"], chunk_host)
        self._lamb.update(n_seg=len(rows), n_chunks=nc, names=[r[0] for r in rows],
                          active=[bool(r[5]) for r in rows], adapt=[bool(t.adapt) for t in tab])
        self._opt_key, self._opt_host = key, host

    def lamb_stats(self, adaptive_only: bool = False) -> Dict[str, Tuple[float, float, float]]:
        """{parameter name: (|p|, |u|, trust ratio)} of the last LAMB step over the trained parameters (adaptive_only: those that step
        with a trust ratio).  One device-to-host copy; the step itself never calls it."""
        if self._lamb is None:
            raise RuntimeError("lamb_stats: LAMB was never enabled (set_optimizer('lamb'))")
        lm = self._lamb
        recs = (L.LambRecord * lm["n_seg"]).from_buffer_copy(lm["records"][:lm["n_seg"] * C.sizeof(L.LambRecord)].cpu().numpy().tobytes())
        return {k: (r.pnorm, r.unorm, r.ratio) for k, r, a, ad in zip(lm["names"], recs, lm["active"], lm["adapt"])
                if a and (ad or not adaptive_only)}

    def _opt_step(self, grad_scale: float):
        """adam_step() under adamw / lamb: the guard and the step advance as in the Adam arms, then the kind's own update.  The
        entries take the guard's record, the average and the schedule's record as nullable arguments, so one path serves every arm."""
        self._opt_sync()
        st = None
        seg, nseg = (self._seg_dev, self._seg_n) if self._groups else (None, 0)
        if self._guard is not None:
            max_norm, skip_nonfinite = self._guard
            st = self._guard_state
            self.call("dpc_grad_sumsq", self.flat_g, self.numel, seg, nseg, self._guard_partials)
            self.call("dpc_grad_verdict", self._guard_partials, L.GRAD_PARTIALS, max_norm or 0.0, int(skip_nonfinite), st)
        lrs = None
        if self._lr_desc is not None:
            lrs = self._lr_state
            self.call("dpc_step_advance_sched", self.dev_step, self.dev_bc, 0.9, 0.999, st, C.byref(self._lr_desc), lrs)
        elif st is not None:
            self.call("dpc_step_advance_gated", self.dev_step, self.dev_bc, 0.9, 0.999, st)
        else:
            self.call("dpc_step_advance", self.dev_step, self.dev_bc, 0.9, 0.999)
        ema, step, decay = (self.flat_ema, self.dev_step, self._ema) if self._ema is not None else (None, None, 0.0)
        if self._opt_kind == "adamw":
            if self._opt_x1d:
                seg, nseg = self._aw_seg_dev, self._aw_seg_n
            if seg is not None:
                self.call("dpc_adamw_groups_dev", self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.numel, seg, nseg,
                          0.9, 0.999, 1e-8, self.dev_bc, grad_scale, st, ema, step, decay, lrs)
            else:
                self.call("dpc_adamw_dev", self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.numel, self.lr, 0.9, 0.999, 1e-8,
                          self.wd, self.dev_bc, grad_scale, st, ema, step, decay, lrs)
            return
        lm = self._lamb
        self.call("dpc_lamb_moments", self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.numel, lm["seg"], lm["n_seg"], lm["chunks"],
                  lm["n_chunks"], 0.9, 0.999, 1e-8, self.dev_bc, grad_scale, st, lm["partials"])
        self.call("dpc_lamb_ratios", lm["seg"], lm["n_seg"], lm["partials"], lm["n_chunks"], st, lm["records"])
        self.call("dpc_lamb_apply", self.flat_p, self.flat_m, self.flat_v, self.numel, lm["seg"], lm["n_seg"], lm["chunks"], lm["n_chunks"],
                  1e-8, self.dev_bc, st, lm["records"], ema, step, decay, lrs)

    def _count_step(self):
        """one more attempted optimizer step on the host mirror; with skip_nonfinite the device may have counted none"""
        self._step_count += 1
        if self._guard is not None and self._guard[1]:
            self._steps_unsure = True

    def _adam_step_ema(self, grad_scale: float):
        """adam_step() with the parameter average on: the four arms of adam_step (guard on / off x groups yes / no) through the _ema
        entries, which take the guard's record as a nullable argument"""
        st = None
        seg, nseg = (self._seg_dev, self._seg_n) if self._groups else (None, 0)
        if self._guard is not None:
            max_norm, skip_nonfinite = self._guard
            st = self._guard_state
            self.call("dpc_grad_sumsq", self.flat_g, self.numel, seg, nseg, self._guard_partials)
            self.call("dpc_grad_verdict", self._guard_partials, L.GRAD_PARTIALS, max_norm or 0.0, int(skip_nonfinite), st)
            self.call("dpc_step_advance_gated", self.dev_step, self.dev_bc, 0.9, 0.999, st)
        else:
            self.call("dpc_step_advance", self.dev_step, self.dev_bc, 0.9, 0.999)
        if self._groups:
            self.call("dpc_adam_groups_dev_ema", self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.numel, seg, nseg,
                      0.9, 0.999, 1e-8, self.dev_bc, grad_scale, st, self.flat_ema, self.dev_step, self._ema)
        else:
            self.call("dpc_adam_dev_ema", self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.numel, self.lr, 0.9, 0.999, 1e-8,
                      self.wd, self.dev_bc, grad_scale, st, self.flat_ema, self.dev_step, self._ema)

    def adam_step(self, grad_scale: float = 1.0):
        self._adam_step(grad_scale)
        # a step (or cycle) the guard skips empties the negative queue: one one-thread launch behind the verdict, only while both are on
        if self._negq and self._guard is not None and self._guard[1]:
            self.call("dpc_negq_clear", self._negq_state, self._guard_state)

    def _adam_step(self, grad_scale: float):
        self._not_swapped("adam_step")
        self._count_step()
        if self._opt_kind != "adam":
            return self._opt_step(grad_scale)
        if self._lr_desc is not None:
            return self._adam_step_sched(grad_scale)
        if self._ema is not None:
            return self._adam_step_ema(grad_scale)
        if self._guard is not None:
            # Runs after the gradient exchange: every rank reduces the same all-reduced arena with the same work split and the same
            # summation order, so all ranks reach the same verdict bit for bit -- no collective, no host.
            max_norm, skip_nonfinite = self._guard
            seg, nseg = (self._seg_dev, self._seg_n) if self._groups else (None, 0)
            st = self._guard_state
            self.call("dpc_grad_sumsq", self.flat_g, self.numel, seg, nseg, self._guard_partials)
            self.call("dpc_grad_verdict", self._guard_partials, L.GRAD_PARTIALS, max_norm or 0.0, int(skip_nonfinite), st)
            self.call("dpc_step_advance_gated", self.dev_step, self.dev_bc, 0.9, 0.999, st)
            if self._groups:
                self.call("dpc_adam_groups_dev_ex", self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.numel, seg, nseg,
                          0.9, 0.999, 1e-8, self.dev_bc, grad_scale, st)
            else:
                self.call("dpc_adam_dev_ex", self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.numel, self.lr, 0.9, 0.999, 1e-8,
                          self.wd, self.dev_bc, grad_scale, st)
            return
        self.call("dpc_step_advance", self.dev_step, self.dev_bc, 0.9, 0.999)
        if self._groups:
            self.call("dpc_adam_groups_dev", self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.numel, self._seg_dev, self._seg_n,
                      0.9, 0.999, 1e-8, self.dev_bc, grad_scale)
            return
        self.call("dpc_adam_dev", self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.numel, self.lr, 0.9, 0.999, 1e-8,
                  self.wd, self.dev_bc, grad_scale)

    # ------------------------------------------------------------------ gradient accumulation (csrc/grad_accum.hip)
    def set_grad_accum(self, n: int = 1):
        """Gradient accumulation in front of the fused step: with n > 1, train_step() -- eager or replayed -- is one MICRO-BATCH, and
        n of them make one optimizer step.  Micro-batches 0 .. n-2 of a cycle run forward and backward and add flat_g into a second
        f32 arena, ``flat_acc`` (dpc_grad_accumulate, DPC_ACCUM_ADD): no gradient exchange, no adam_step().  The last one runs
        forward and backward, turns flat_g into the MEAN gradient of the cycle -- (flat_acc + flat_g) * float32(1 / n), which also
        returns flat_acc to +0 (DPC_ACCUM_FINISH) -- in front of the gradient exchange, and then adam_step() as it stands: the
        guard's norm and verdict, the clip, AdamW, LAMB's ratios, the parameter average and the schedule see the mean gradient and
        count optimizer steps, not micro-batches.  ``self.result`` is every micro-batch's own.  n = 1 (the default) turns it off:
        train_step(), adam_step() and the captures then run what they ran without it.

        A non-finite value in any micro-gradient reaches the sum, so with skip_nonfinite the whole cycle is dropped (flat_acc is
        +0 again all the same).  Dropout is keyed on dev_draw, which advances per forward: every micro-batch draws new masks.
        BatchNorm uses each micro-batch's own statistics (LC's running buffers move once per micro-batch, as in torch), and the
        contrastive negatives stay those of one micro-batch: accumulation enlarges the optimizer's batch, not the number of negatives
        (DPCEngine.set_neg_queue does that: under it every micro-batch also competes against the keys of the K batches before it).

        With parameter groups only the units of active segments are accumulated (the live-unit rule of the gradient guard): the slices
        of a frozen parameter are neither read nor written in either arena.

        ``flat_acc`` is allocated zero-filled at the first n > 1 -- before a step is captured, a captured step allocates nothing -- and
        never otherwise.  Refused inside a capture and while a cycle is open (accum_pending != 0; reset_accum() closes one after an
        exception).  n is among the scalars a captured step bakes in: a replay after it changed raises."""
        n = int(n)
        if n < 1:
            raise ValueError(f"set_grad_accum: n must be at least 1, got {n}")
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise L.DpcError("set_grad_accum: not while a graph is being captured")
        self._not_mid_cycle("set_grad_accum")
        if n > 1:
            self._accum_alloc()
        self._accum_n = n

    def _accum_alloc(self):
        if self.flat_acc is None:
            if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise L.DpcError("set_grad_accum: enable the accumulation before a step is captured (it allocates its arena)")
            self.flat_acc = torch.zeros_like(self.flat_g)

    @property
    def accum_steps(self) -> int:
        """micro-batches per optimizer step (1: no accumulation)"""
        return self._accum_n

    @property
    def accum_pending(self) -> int:
        """micro-batches of the open cycle already summed into flat_acc (0: at a cycle boundary)"""
        return self._accum_pos

    def _not_mid_cycle(self, what: str):
        if self._accum_pos:
            raise RuntimeError(f"{what}: an accumulation cycle is open ({self._accum_pos} of {self._accum_n} micro-batches are in "
                               "flat_acc); finish the cycle, or drop it with reset_accum()")

    def reset_accum(self):
        """drop the open cycle (after an exception): flat_acc back to zero, the position to 0"""
        if self.flat_acc is not None:
            self.flat_acc.zero_()
        self._accum_pos = 0

    def _accum_launch(self, mode: int, begin: int, end: int):
        """dpc_grad_accumulate over the floats [begin, end) of the two arenas, under the groups' segment table when there is one"""
        seg, nseg = (self._seg_dev, self._seg_n) if self._groups else (None, 0)
        self.call("dpc_grad_accumulate", self.flat_acc, self.flat_g, self.numel, begin, end, seg, nseg, mode, 1.0 / self._accum_n)

    def _accum_finish_and_exchange(self, allreduce=None, cut=None):
        """the last micro-batch's backward, DPC_ACCUM_FINISH in front of each exchange point, the exchange: two FINISH launches with
        the two-bucket exchange (the tail's inside on_tail_ready, in front of ``allreduce.start``; the first bucket's after the
        backward, in front of ``allreduce.finish`` -- left out when the backward did not reach the backbone: that bucket is empty),
        else one over the whole arena.  cut: a captured step's cut (capture_train_step) in place of the exchange's calls"""
        if allreduce is not None and hasattr(allreduce, "start"):
            def tail_ready(tail):
                self._accum_launch(L.ACCUM_FINISH, self.grad_split, self.numel)
                if cut is None:
                    allreduce.start(tail)
                elif self._backward_reaches_backbone():   # (else one cut serves both exchange points, as without accumulation)
                    cut()

            self.backward(on_tail_ready=tail_ready)
            head = self._first_bucket()
            if head.numel():
                self._accum_launch(L.ACCUM_FINISH, 0, self.grad_split)
            if cut is None:
                allreduce.finish(head)
            else:
                cut()
            return
        self.backward()
        self._accum_launch(L.ACCUM_FINISH, 0, self.numel)
        if allreduce is not None:
            if cut is None:
                allreduce(self.flat_g)
            else:
                cut()

    def _accum_micro_step(self, allreduce=None):
        """what train_step() runs behind the forward while set_grad_accum(n > 1) is on: one micro-batch of the cycle"""
        if self._accum_pos < self._accum_n - 1:
            self.backward()
            self._accum_launch(L.ACCUM_ADD, 0, self.numel)
            self._accum_pos += 1
            return
        self._accum_finish_and_exchange(allreduce)
        self._accum_pos = 0
        self.adam_step()

    def _first_bucket(self) -> torch.Tensor:
        """the gradients finished last (stem + layer1): the second bucket of the two-bucket exchange"""
        return self.flat_g[:self.grad_split]

    def _backward_and_exchange(self, allreduce=None):
        """the head's backward(), then the gradient exchange: two buckets (``allreduce.start`` on the tail while layer1 + stem
        are still running, ``allreduce.finish`` on the rest) or one call on the whole arena"""
        if allreduce is not None and hasattr(allreduce, "start"):
            self.backward(on_tail_ready=allreduce.start)
            allreduce.finish(self._first_bucket())
        else:
            self.backward()
            if allreduce is not None:
                allreduce(self.flat_g)

    # ------------------------------------------------------------------ captured steps of both heads
    def _baked_scalars(self) -> tuple:
        """host scalars a captured step carries as kernel arguments (a replay keeps the values of its capture)"""
        gd = self.gru_desc
        base = (float(self.lr), float(self.wd), float(gd.p_drop), int(gd.seed))
        # with parameter groups the captured update reads the segment table: its contents belong to what a replay must still find
        if self._groups:
            base = base + ((self._seg_n, self._seg_host),)
        # ... and with the gradient guard its two settings (only then: the keys of unguarded runs stay what they were)
        if self._guard is not None:
            base = base + (("grad_guard",) + self._guard,)
        # ... and with the parameter average its decay (again only then)
        if self._ema is not None:
            base = base + (("ema", self._ema),)
        # ... and with another update rule than Adam its kind, its flag and its tables (only then)
        if self._opt_kind != "adam":
            base = base + (("optimizer", self._opt_kind, self._opt_x1d, self._opt_host),)
        # ... and with gradient accumulation the micro-batches per optimizer step (only then)
        if self._accum_n > 1:
            base = base + (("accum", self._accum_n),)
        # ... and with the negative queue its slot count (only then)
        if self._negq:
            base = base + (("negq", self._negq),)
            if self._negq_gen > 1:   # ... and which allocation of the ring: a step captured on an earlier one must not replay on this one
                base = base + (("negq_ring", self._negq_gen),)
        # ... and with the cosine score its form and temperature (only then)
        if getattr(self, "_snorm", None) is not None:
            base = base + (("score_norm", "cosine", self._snorm[0]),)
        # ... and with the negative classes their weights and the report flag (only then)
        if getattr(self, "_ncls", None) is not None:
            base = base + (("neg_cls",) + self._ncls,)
        # ... and with the symmetric loss the weight of its column direction (only then)
        if getattr(self, "_sym", 0.0) > 0:
            base = base + (("loss_sym", self._sym),)
        # ... and with the learning-rate schedule its descriptor, which a captured step carries by value (only then, once more)
        return base + (("lr_schedule", bytes(self._lr_desc)),) if self._lr_desc is not None else base

    def check_graph_capture(self):
        """raises the DpcError every capture raises when this engine cannot capture a step (it does not run on the HIP device)"""
        if self.device.type != "cuda":
            raise L.DpcError("hipGraph capture needs the HIP device")

    def _capture(self, key: tuple, what: str, again: str, warm, body, run, refill=None, **attrs):
        """what capture_train_step and capture_eval_step share: the cache by `key`, the eager `warm()` and the capture of
        `body(cut)` on a side stream -- `cut()` ends one graph and begins the next where a replay has host work to do between
        them --, the fork / join events, and ``replay()``, which checks the baked scalars and returns ``run(engine, graphs)``.
        `attrs` are hung on the replay closure beside .graphs / .events / .refill / .kernels (kernel launches captured into each
        graph: a capture that would leave an empty graph raises)."""
        self.check_graph_capture()
        hit = self._captures.get(key)
        if hit is not None:   # the same static buffer, the same exchange: the capture that exists (see _LIVE_GRAPHS)
            return hit
        cur = torch.cuda.current_stream(self.device)
        side = torch.cuda.Stream(self.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):  # eager warm-up: lazy buffers, RCCL communicator
            warm()
        cur.wait_stream(side)
        torch.cuda.synchronize(self.device)
        pool = torch.cuda.graph_pool_handle()
        graphs: List[torch.cuda.CUDAGraph] = []
        kernels: List[int] = []
        state = {}

        def begin():
            state["g"] = torch.cuda.CUDAGraph()
            state["g"].capture_begin(pool=pool)
            state["n0"] = self._launches

        def end():
            state["g"].capture_end()
            graphs.append(state["g"])
            kernels.append(self._launches - state["n0"])

        def cut(*_):
            end()
            begin()

        side.wait_stream(cur)
        # The fork / join events side() records while the step is being captured live as long as the graphs do (they hang off the
        # replay closure): a captured event that is destroyed before its graph is the one candidate mechanism found for the host-memory
        # corruption that used to follow graph destruction (see _LIVE_GRAPHS; DPC_KEEP_CAPTURE_EVENTS=0 lets them go when side()
        # returns, as rounds 3-4 did -- the A/B of scripts/gpu_r5_graph_destroy.sh).
        keep_events = os.environ.get("DPC_KEEP_CAPTURE_EVENTS", "1") != "0"
        self._capture_events = [] if keep_events else None
        try:
            with torch.cuda.stream(side):
                begin()
                self.packed_for_step = -1
                if refill is not None:
                    refill()
                body(cut)
                end()
        finally:
            events, self._capture_events = self._capture_events, None
        self.packed_for_step = -1   # the capture executed nothing: the packed weights are not those of this step yet
        cur.wait_stream(side)
        me = weakref.ref(self)   # the cached closure must not keep its engine (tens of GB of buffers) alive through a cycle
        baked = self._baked_scalars()

        def replay():
            eng = me()
            if eng is None:
                raise RuntimeError(f"replay of a captured {what} step whose engine is gone")
            if eng._baked_scalars() != baked:   # loud, not stale: the graph would go on stepping with the values of its capture
                raise RuntimeError(f"lr / wd / dropout / gradient guard / EMA decay / lr schedule changed since this step was captured ({baked} -> {eng._baked_scalars()}): "
                                   f"call {again}")
            return run(eng, graphs)

        replay.graphs = graphs
        replay.kernels = kernels
        replay.events = events   # destroyed after the graphs, not before
        replay.refill = refill
        for k, v in attrs.items():
            setattr(replay, k, v)
        self._capture_graphs.append(_Capture(graphs, events))
        if not all(kernels):   # (parked like every other capture; never cached, never replayed)
            raise L.DpcError(f"the captured {what} step was cut into an empty hipGraph (kernel launches per graph: {kernels})")
        self._captures[key] = replay
        return replay

    def _forward_loss(self, block: Optional[torch.Tensor], train: bool):
        """the head's forward of an engine-owned step on `block` (None: the stem's operand as it stands): leaves the metrics in
        ``self.result`` and, when `train`, the loss gradient where ``backward()`` expects it"""
        raise NotImplementedError

    def _backward_reaches_backbone(self) -> bool:
        """whether the engine-owned step's backward runs the backbone's backward.  A head whose backward can stop in front of it
        answers from its optimizer's state; a captured step asks when it is captured, and the answer is part of its key."""
        return True

    def capture_train_step(self, block: Optional[torch.Tensor], allreduce=None, warmup: int = 2, refill=None):
        """Captures the head's whole train step -- forward + loss on `block` (a static device buffer: refill it in place between
        replays), backward, Adam -- into hipGraphs and returns ``replay() -> self.result`` (device f32: DPC loss, top1, top3, top5;
        LC loss, top-1).  Dropout masks and Adam's bias corrections are keyed on device-side counters, so every replay is a new
        optimizer step.
        block=None: the step starts from the stem's operand as it stands (train_step(None)) -- and, for LC, the labels as they
        stand in ``self.target``: filled in the graph by ``refill=lambda: eng.fill_synthetic(seed)``, or eagerly before each replay
        (load_recipe, set_labels).
        refill: optional callable captured in FRONT of the step (e.g. ``lambda: block.normal_()``: a fresh synthetic batch per replay
        from torch's graph-safe default generator -- SURVEY section 8d "generated ON DEVICE").

        Cached by (static input buffer, exchange, carve-out, side_off, refill identity, no_grad_params, baked host scalars): asking
        again returns the replay that exists.  Every host scalar the capture bakes into kernel arguments (_baked_scalars: lr, wd,
        dropouts and seeds, the Adam segment table) is part of the key, and a replay raises once one of them changed: after
        eng.lr = ... (LR schedule, checkpoint.resume, --reset_lr) asking again captures a step with the new values instead of
        handing back the stale replay.  The graphs are parked, never destroyed (_LIVE_GRAPHS).

        One graph without data parallelism.  With the two-bucket gradient exchange the capture is cut where the backward hands the
        gradient tail to RCCL: graph A (forward, loss, backward down to layer2) -> allreduce.start(tail) asynchronously -> graph B
        (layer1 + stem backward) -> allreduce.finish(head) + join -> graph C (Adam).  With a backward that stops in front of the
        backbone (_backward_reaches_backbone) there is nothing between the two exchange points, so the capture is cut ONCE: graph A
        (forward, head backward) -> allreduce.start(tail) -> allreduce.finish(empty first bucket), as the eager step does -> graph
        B (Adam).  No empty hipGraph is created or replayed.

        Under set_grad_accum(n > 1) the replay is one MICRO-BATCH per call and holds two such captures (_capture_accum_step)."""
        buf = self.x_s2d if block is None else block   # the static buffer the step reads its input from
        need_backbone = self._backward_reaches_backbone()
        key = (buf.data_ptr(), tuple(buf.shape), id(allreduce) if allreduce is not None else None, self.reserve_cus, tuple(sorted(self.side_off)),
               id(refill) if refill is not None else None, tuple(sorted(self.no_grad_params))) + self._baked_scalars()
        two_bucket = allreduce is not None and hasattr(allreduce, "start")
        split = self.grad_split if need_backbone else 0   # the first bucket of the exchange: empty when the backward was truncated
        tail, head, whole, result = self.flat_g[self.grad_split:], self.flat_g[:split], self.flat_g, self.result

        def warm():
            for _ in range(warmup):
                self.train_step(block, allreduce=allreduce)

        def body(cut):
            self._forward_loss(block, True)
            if two_bucket and not need_backbone:   # backward() hands the tail over and returns: one cut serves both exchange points
                self.backward(on_tail_ready=lambda _tail: None)
                cut()
            else:
                self.backward(on_tail_ready=cut if two_bucket else None)
                if allreduce is not None:
                    cut()
            host_steps, unsure = self._step_count, self._steps_unsure
            self.adam_step()
            self._step_count, self._steps_unsure = host_steps, unsure  # capture executes nothing

        def run(eng, graphs):
            eng._not_swapped("replay of a captured train step")
            graphs[0].replay()
            if two_bucket:
                allreduce.start(tail)
                if need_backbone:
                    graphs[1].replay()
                allreduce.finish(head)
                graphs[-1].replay()
            elif allreduce is not None:
                allreduce(whole)
                graphs[1].replay()
            eng._count_step()
            eng.packed_for_step = -1
            return result

        if self._accum_n > 1:   # one micro-batch per replay: two captures, picked by the position in the cycle
            return self._capture_accum_step(key, block, buf, allreduce, warmup, refill, run)
        # block=buf: the static input buffer stays alive (and its address un-reused) as long as the capture does
        return self._capture(key, "train", "capture_train_step() again (it captures a new step for the new values)", warm, body, run,
                             refill, block=buf)

    def _capture_accum_step(self, key: tuple, block, buf, allreduce, warmup: int, refill, run_last):
        """capture_train_step() under set_grad_accum(n > 1).  The replay is still one micro-batch per call, refill included, and holds
        two captures taken at the same time: ``replay.micro``, one graph -- refill, forward, backward, DPC_ACCUM_ADD --, and
        ``replay.last``, the cut protocol of capture_train_step with the DPC_ACCUM_FINISH launches in front of each exchange point
        (_accum_finish_and_exchange).  It picks by the engine's position in the cycle and advances it, so eager micro-batches and
        replays may alternate.  The warm-up runs whole cycles and needs a cycle boundary."""
        hit = self._captures.get(key)
        if hit is not None:
            return hit
        n, result = self._accum_n, self.result
        again = "capture_train_step() again (it captures a new step for the new values)"
        if warmup and self._accum_pos:
            raise RuntimeError("capture_train_step: a warm-up under gradient accumulation runs whole cycles and must start at a cycle "
                               f"boundary ({self._accum_pos} of {n} micro-batches are pending)")

        def warm():
            for _ in range(warmup * n):
                self.train_step(block, allreduce=allreduce)

        def body_micro(cut):
            self._forward_loss(block, True)
            self.backward()
            self._accum_launch(L.ACCUM_ADD, 0, self.numel)

        def run_micro(eng, graphs):
            eng._not_swapped("replay of a captured train step")
            graphs[0].replay()
            return result

        def body_last(cut):
            self._forward_loss(block, True)
            self._accum_finish_and_exchange(allreduce, cut)
            host_steps, unsure = self._step_count, self._steps_unsure
            self.adam_step()
            self._step_count, self._steps_unsure = host_steps, unsure  # capture executes nothing

        micro = self._capture(key + ("micro",), "train", again, warm, body_micro, run_micro, refill, block=buf)
        last = self._capture(key + ("last",), "train", again, lambda: None, body_last, run_last, refill, block=buf)
        me = weakref.ref(self)

        def replay():
            eng = me()
            if eng is None:
                raise RuntimeError("replay of a captured train step whose engine is gone")
            if eng._accum_pos < n - 1:
                res = micro()
                eng._accum_pos += 1
            else:
                res = last()
                eng._accum_pos = 0
            return res

        replay.micro, replay.last = micro, last
        replay.graphs, replay.kernels = micro.graphs + last.graphs, micro.kernels + last.kernels
        replay.events, replay.refill, replay.block = (micro.events or []) + (last.events or []), refill, buf
        self._captures[key] = replay
        return replay

    def capture_eval_step(self, refill=None):
        """Captures one evaluation step on the stem's operand (and LC's labels) as they stand -- `refill` (e.g. ``lambda:
        eng.fill_synthetic(seed)``), then the head's eval-mode forward + loss -- into one hipGraph and returns ``replay() ->
        self.result``.  The weight repack is inside the graph unconditionally, so a replay after more training evaluates the weights
        (and running buffers) of now, not those of the capture.  Same rules as capture_train_step.  No eager warm-up: run one eager
        evaluation step first (the forward allocates its ReLU masks on first use)."""
        key = ("eval", self.x_s2d.data_ptr(), tuple(sorted(self.side_off)), id(refill) if refill is not None else None) + self._baked_scalars()
        result = self.result

        def warm():
            if self._pack_table is None:
                self.pack_weights()   # builds the static repack table: its host-to-device copy cannot be captured

        def body(cut):
            self._forward_loss(None, False)

        def run(eng, graphs):
            graphs[0].replay()
            return result

        return self._capture(key, "evaluation", "capture_eval_step() again", warm, body, run, refill)

    def release_captures(self):
        """forget this engine's captured train steps (the next capture_train_step captures again).  The hipGraphs are parked until the
        interpreter exits, not destroyed -- see _LIVE_GRAPHS for why and for what that costs; DPC_KEEP_GRAPHS=0 destroys them here,
        after the device has gone idle."""
        torch.cuda.synchronize(self.device)
        self._captures.clear()
        _park_graphs(list(self._capture_graphs))
        self._capture_graphs.clear()


class DPCEngine(BackboneEngine):
    """the DPC-RNN step: backbone + ConvGRU aggregate / predict, contrastive score, loss"""

    def __init__(self, network: str = "resnet18", sample_size: int = 128, num_seq: int = 8, seq_len: int = 5,
                 pred_step: int = 3, batch: int = 4, device="cuda", compute_dtype=torch.float32,
                 widths: Sequence[int] = LAYER_WIDTH, lib: Optional[L.Lib] = None,
                 lr: float = 1e-3, wd: float = 1e-5, dropout: float = 0.1, seed: int = 233, score_path: str = "auto", stem_fused: bool | None = None,
                 fold: bool | None = None, reserve_cus: int | None = None, f32_matmul: str | None = None):
        self.P = pred_step
        self.score_mode = "materialised"  # what the last train step ran ("fused": no [R][R] tensor in HBM)
        super().__init__(param_shapes(network, widths), network, sample_size, num_seq, seq_len, batch, device, compute_dtype, widths, lib,
                         lr, wd, dropout, seed, stem_fused, fold, reserve_cus, f32_matmul)
        self._build_head(score_path)
        self._finish_buffers()

    # ---- head of DPC_RNN: ConvGRU aggregate/predict, contrastive score, loss
    def _build_head(self, score_path: str):
        dt, f32 = self.cdtype, torch.float32
        B, P, SQ, D, N = self.B, self.P, self.SQ, self.D, self.N
        if score_path not in ("auto", "fused", "materialised"):
            raise ValueError("score_path must be auto, fused or materialised")
        # ---- ConvGRU / predictor / score buffers.  rows M = (b, s); N - P aggregation steps (dpc/model_3d.py:62), and the GRU step
        # after the last prediction is dead code (model_3d.py:70-72)
        self._build_gru(n_agg=N - P, n_steps=(N - P) + P - 1, P=P)
        M = self.M
        self.feat_inf = self.empty((B, P, SQ, D), dt)
        self.pred = self.empty((B, P, SQ, D), dt)
        self.P1_all = self.empty((P, M, D), dt)       # relu(W1 h + b1)
        self.dP1 = self.empty((P, M, D), dt)          # grads at the pre-activations of network_pred
        self.dP2 = self.empty((P, M, D), dt)
        self.Hpred = self.H_all[self.n_agg:]          # hidden state each prediction was made from
        R = B * P * SQ
        self.R = R
        self.score = self.empty((R, R), f32)
        E = 8 if dt == torch.bfloat16 else 4
        self.ld_d = (R + E - 1) // E * E
        self.dscore = self.empty((R, self.ld_d), dt)
        self.row_ws = self.empty((R, 2), f32)
        self.result = self.empty((4,), f32)
        self.predT = torch.zeros((D, self.ld_d), dtype=dt, device=self.device)   # transposed operands of the score backward
        self.finfT = torch.zeros((D, self.ld_d), dtype=dt, device=self.device)   # (columns >= R stay zero)
        # The score + loss of a bf16 train step, two ways (csrc/score_fused.hip):
        #   "materialised": score GEMM -> [R][R] f32 in HBM -> CE / top-k / dS (bf16) -> two split-K GEMMs;
        #   "fused": LSE, target logit and rank inside the forward contraction, dS recomputed inside the two backward contractions -- no
        #            [R][R] tensor in HBM (151 MB + 75 MB at cfg2, 983 MB + 492 MB at cfg5).
        # Measured on MI355X: at R = 6 144 the materialised step wins clearly (fused backward 2 x 140 us against 2 x 37 us: exp() is
        # quarter rate and K = 256 gives the matrix cores too little to hide it behind); at R = 15 680 it wins by 1.5 % of the step
        # (813 against 801 clips/s at cfg5, round 4).  288 GB of HBM make the 1.5 GB a non-issue, so "auto" = materialised at every
        # size since round 5 (round 2-4: fused from R = 8 192); "fused" keeps the other path selectable (bench.py --score-path fused).
        fusable = dt == torch.bfloat16 and D in (256, 32)
        self.score_fusable = fusable and score_path == "fused"
        self._score_fused = False
        if self.score_fusable:
            nf, nb = C.c_int64(0), C.c_int64(0)
            self.lib.call("dpc_score_ws_floats", R, D, C.byref(nf), C.byref(nb))
            self.score_ws = self.empty((max(nf.value, nb.value),), f32)
            self.score_diag, self.score_lse2 = self.empty((R,), f32), self.empty((R,), f32)
        # bf16 LOGITS for the step that does not return its score (train_step / capture_train_step / validate: forward(materialise=False)):
        # the score GEMM writes, and the loss kernel reads, [R][R] in the compute dtype -- 75 MB instead of 151 MB each way at cfg2,
        # 492 instead of 983 MB at cfg5.  forward(materialise=True) -- the module boundary, everything that looks at the score -- keeps
        # f32.  Needs whole 128-byte rows (R a multiple of 64: cfg2 6 144, cfg5 15 680; cfg4's 6 468 keeps f32); DPC_SCORE_BF16=0: off.
        self.score16 = None
        if dt == torch.bfloat16 and R % 64 == 0 and R <= 16384 and D in (256, 32) and not self.score_fusable and int(os.environ.get("DPC_SCORE_BF16", "1")):
            self.score16 = self.empty((R, R), dt)
        self._score16_live = False
        self.d_pred = self.empty((B, P, SQ, D), f32)
        self.d_finf = self.empty((B, P, SQ, D), f32)
        self.mask: Optional[torch.Tensor] = None
        self._score_path = score_path
        self._negq_live = False   # the last forward read the negative queue (set_neg_queue): its backward adds the queue part and pushes
        self._negq_state = self._negq_ring = self._negq_ringT = self._negq_stats = self._negq_lse = self._negq_ws = None
        self._negq_retired = []   # buffers of an earlier ring that a captured step may still address (set_neg_queue)
        self._snorm = None        # the cosine score (set_score_norm): None, or (temperature, float32(1 / temperature))
        self.pred_n = self.finf_n = self.rnorm = None   # ... its normalised operands [R][D] and the rows' 1 / norm, f32 [2R]
        self._snorm_retired = []
        self._ncls = None         # negative classes in the loss (set_neg_classes): None, or (w_S, w_T, w_E, report)
        self._ncls_live = False   # the last forward was the training step's: loss_topk runs the _cls entry
        self._ncls_desc = self._ncls_rows = self._ncls_report = None
        self._ncls_retired = []
        self._sym = 0.0           # symmetric loss (set_loss_sym): the weight W of the key-to-prediction direction, 0 = off
        self._sym_live = False    # the last forward was the training step's: loss_topk runs the _sym entry
        self._sym_col_lse = self._sym_col_ws = self._sym_ws = self._sym_result = None
        self._sym_retired = []
        self._need_wgrad(R, R, D)
        nsk = C.c_int32(0)  # d_pred = dS @ feature_inf: f32 slabs of the split reduction
        self.lib.call("dpc_gemm_nt_splitk", L.dtype_code(dt), R, D, self.ld_d, None, self.ld_d, None, self.ld_d, None, C.byref(nsk), self.lib.stream())
        self.need_part(nsk.value * R * D)
        # d_feature_inf = dS^T @ pred on the loader / compute kernel with dS read K-major (csrc/gemm_ws.hip); None: weight-gradient kernel
        self._tn_splits = None
        if dt == torch.bfloat16:
            rc = self.lib._fn("dpc_gemm_tn_splitk")(L.dtype_code(dt), R, D, R, None, self.ld_d, None, self.ld_d, None, C.byref(nsk), self.lib.stream())
            if rc == 0:
                self._tn_splits = nsk.value
                self.need_part(nsk.value * R * D)
        gd, Pm = self.gru_desc, self.PRM
        for name, t in (("bias_1", Pm["network_pred.0.bias"]), ("bias_2", Pm["network_pred.2.bias"]), ("P1_all", self.P1_all),
                        ("pred", self.pred), ("d_pred", self.d_pred), ("dP1", self.dP1), ("dP2", self.dP2)):
            setattr(gd, name, t.data_ptr())

    def forward(self, block: torch.Tensor, train: bool = False, dropout_masks: Optional[torch.Tensor] = None,
                materialise: bool = True, new_draw: bool = True, use_neg_queue: bool = False):
        """block [B,N,3,SL,H,W] f32 on the device.  Returns the score tensor [B,P,SQ,B,P,SQ] (f32, engine-owned).
        dropout_masks: optional [n_steps,M,D] pre-scaled keep masks (tests); train=True draws them on the device.
        new_draw=False repeats the previous forward's Philox masks (tests comparing two paths on one step).
        materialise=False (bf16 mode): the score is consumed tile by tile by the fused loss (csrc/score_fused.hip) and
        never written; the return value is None and loss_topk() / backward() use the fused path.
        use_neg_queue: the engine-owned training step's forward (_forward_loss(train=True)) -- with set_neg_queue(K > 0) the rows also
        compete against the bank's keys, and this forward's backward pushes feat_inf; everything else leaves the bank alone.  The same
        flag marks the forward whose loss carries the class weights and the report of set_neg_classes: both belong to the engine-owned
        training loss and to nothing else."""
        B, N, P, SQ, D, M = self.B, self.N, self.P, self.SQ, self.D, self.M
        if block is not None:
            if tuple(block.shape) != (B, N, 3, self.SL, self.size, self.size) or block.dtype != torch.float32:
                raise ValueError(f"block must be float32 [B,N,3,SL,H,W] = {(B, N, 3, self.SL, self.size, self.size)}, got {tuple(block.shape)}")
            if block.device != self.device:
                raise ValueError("block is on the wrong device")
        x = self._backbone_forward(block)
        dc = L.dtype_code(self.cdtype)
        fs = self.feat_shape
        self.call("dpc_tpool_split_fwd", x, dc, B, N, fs[1], SQ, D, P, self.feat_relu, self.feat_inf)
        # dropout masks on the carried hidden state (backbone/convrnn.py:78)
        if dropout_masks is not None:
            self.drop_all = dropout_masks.to(self.device, torch.float32).contiguous()
            if tuple(self.drop_all.shape) != (self.n_steps, M, D):
                raise ValueError(f"dropout_masks must be [n_steps, M, D] = {(self.n_steps, M, D)}")
        else:  # train: Philox masks are generated inside the recurrence kernel, keyed on (seed, draw counter)
            self.drop_all = None
        # aggregate + predict (dpc/model_3d.py:62-72): the whole recurrence in one launch
        gd = self.gru_desc
        gd.drop_masks = self.drop_all.data_ptr() if dropout_masks is not None else None
        draw = dropout_masks is None and train and self.p_drop > 0
        if draw and new_draw:  # a new draw per train-mode forward (the backward of THIS forward regenerates the same bits)
            self.call("dpc_counter_advance", self.dev_draw)
        gd.step_dev = self.dev_draw.data_ptr() if draw else None
        self.call("dpc_gru_chain_fwd", C.byref(gd))
        # score (dpc/model_3d.py:79-84): pred [R][D] x feat_inf [R][D]^T
        R = self.R
        sp, sf = self.pred, self.feat_inf
        if self._snorm is not None:   # the cosine score: pred / (|pred| T) against feat_inf / |feat_inf|, train and eval alike
            sp, sf = self.pred_n, self.finf_n
            with self.tag("score"):
                self.call("dpc_rownorm_fwd", self.pred, self.feat_inf, sp, sf, self.rnorm, R, D, dc, self._snorm[1], 1.0, SCORE_NORM_EPS)
        self._score_fused = bool(self.score_fusable and not materialise)
        if self._score_fused:
            with self.tag("score"):
                self.call("dpc_score_fwd", sp, sf, R, D, self.score_diag, self.score_lse2, self.row_ws, None,
                          self.score_ws)
            self.score_mode = "fused"
            return None
        self._score16_live = bool(self.score16 is not None and not materialise)
        # the negative queue: only the engine-owned training step (_forward_loss(train=True)) reads it
        self._negq_live = bool(self._negq and use_neg_queue)
        self._ncls_live = bool(self._ncls is not None and use_neg_queue)   # (the engine-owned training forward: see the docstring)
        self._sym_live = bool(self._sym > 0 and use_neg_queue)             # (the same rule for the symmetric loss: set_loss_sym)
        if self._score16_live:   # nobody reads the score but the loss: logits in the compute dtype
            self.score_mode = "materialised (bf16 logits)"
            with self.tag("score"):
                self.gemm(sp, sf, self.score16, R, R, D, out_f32=False)
                if self._negq_live:
                    self._negq_forward(self.score16, L.BF16)
            return None
        self.score_mode = "materialised"
        with self.tag("score"):
            self.gemm(sp, sf, self.score, R, R, D)
            if self._negq_live:
                self._negq_forward(self.score, L.F32)
        return self.score.view(B, P, SQ, B, P, SQ)

    def _negq_forward(self, score: torch.Tensor, dtype_code: int):
        """per-row (max, sum-exp, rank) of pred against the live keys; the target logit is the diagonal of the in-batch logits"""
        self.call("dpc_negq_fwd", self._score_operands()[0], self._negq_ring, self._negq_state, self.R, self.D, self._negq, score, self.R + 1, dtype_code,
                  self._negq_stats, self._negq_ws)

    def _score_operands(self):
        """(pred, feat_inf) as the score reads them: the normalised copies under the cosine score (set_score_norm)"""
        return (self.pred, self.feat_inf) if self._snorm is None else (self.pred_n, self.finf_n)

    def get_mask(self) -> torch.Tensor:
        if self.mask is None:
            B, P, SQ = self.B, self.P, self.SQ
            self.mask = torch.empty((B, P, SQ, B, P, SQ), dtype=torch.int8, device=self.device)
            self.call("dpc_mask_gen", self.mask, B, P, SQ)
        return self.mask

    # ------------------------------------------------------------------ loss
    def loss_topk(self, with_grad: bool = True) -> torch.Tensor:
        """[loss, top1, top3, top5] (device f32[4]); fills dscore when with_grad"""
        R = self.R
        if self._score_fused:  # per-row (loss term, rank) pairs are already there; d/dscore is recomputed inside the backward
            self.call("dpc_ce_finalize", self.row_ws, R, self.result)
            return self.result
        if self._sym_live:    # the column direction beside the row direction, with or without the bank (csrc/loss_sym.hip)
            qs, lse = (self._negq_stats, self._negq_lse) if self._negq_live else (None, None)
            tail = (qs, lse, self._sym, 0, self._sym_col_lse, self._sym_col_ws, self._sym_ws, self._sym_result)
            with self.tag("score"):
                if self._score16_live:
                    self.call("dpc_ce_topk_bf16_sym", self.score16, R, R, R, self.row_ws, self.result, self.dscore if with_grad else None,
                              self.ld_d, *tail)
                else:
                    self.call("dpc_ce_topk_sym", self.score, R, R, R, self.row_ws, self.result, self.dscore if with_grad else None,
                              L.dtype_code(self.cdtype), self.ld_d, *tail)
            return self.result
        if self._ncls_live:   # the same row kernels with a weight per negative class, with or without the bank (csrc/loss_cls.hip)
            qs, lse = (self._negq_stats, self._negq_lse) if self._negq_live else (None, None)
            rows, rep = (self._ncls_rows, self._ncls_report) if self._ncls[3] else (None, None)
            with self.tag("score"):
                if self._score16_live:
                    self.call("dpc_ce_topk_bf16_cls", self.score16, R, R, R, self.row_ws, self.result, self.dscore if with_grad else None,
                              self.ld_d, qs, lse, self._ncls_desc, rows, rep)
                else:
                    self.call("dpc_ce_topk_cls", self.score, R, R, R, self.row_ws, self.result, self.dscore if with_grad else None,
                              L.dtype_code(self.cdtype), self.ld_d, qs, lse, self._ncls_desc, rows, rep)
            return self.result
        if self._negq_live:   # the same row kernels with the queue's statistics folded in (csrc/loss.hip: the EXT arms)
            with self.tag("score"):
                if self._score16_live:
                    self.call("dpc_ce_topk_bf16_ext", self.score16, R, R, R, self.row_ws, self.result, self.dscore if with_grad else None,
                              self.ld_d, self._negq_stats, self._negq_lse)
                else:
                    self.call("dpc_ce_topk_ext", self.score, R, R, R, self.row_ws, self.result, self.dscore if with_grad else None,
                              L.dtype_code(self.cdtype), self.ld_d, self._negq_stats, self._negq_lse)
            return self.result
        if self._score16_live:
            self.call("dpc_ce_topk_bf16", self.score16, R, R, R, self.row_ws, self.result, self.dscore if with_grad else None, self.ld_d)
            return self.result
        self.call("dpc_ce_topk", self.score, R, R, R, self.row_ws, self.result, self.dscore if with_grad else None,
                  L.dtype_code(self.cdtype), self.ld_d)
        return self.result

    # ------------------------------------------------------------------ backward
    def backward(self, dscore_external: Optional[torch.Tensor] = None, on_tail_ready=None):
        """gradients of everything w.r.t. the loss whose d/dscore sits in self.dscore (or is given, [R][R] f32).
        on_tail_ready(flat_g[split:]) is called once every gradient except the stem's and layer1's is final
        (data-parallel runs start their all-reduce there, dpc_amd/parallel.py)."""
        self._backbone_backward(self._head_backward(dscore_external), on_tail_ready)

    def _head_backward(self, dscore_external: Optional[torch.Tensor] = None) -> torch.Tensor:
        """backward of the head from d/dscore: score backward -> recurrence -> temporal pool / split, and the ConvGRU / predictor
        parameter gradients forked onto the side stream.  Returns d_feat, d loss / d (last block output)"""
        B, N, P, SQ, D, M, R = self.B, self.N, self.P, self.SQ, self.D, self.M, self.R
        dc = L.dtype_code(self.cdtype)
        if dscore_external is not None:
            src = dscore_external.reshape(R, R).to(torch.float32).contiguous()
            if self.ld_d != R:
                self.dscore.zero_()
            self.dscore[:, :R].copy_(src)  # module-boundary path only (torch hands over an arbitrary d/dscore)
        # score = pred @ finf^T  ->  d_pred = dS @ finf ; d_finf = dS^T @ pred  (under the cosine score: of the normalised operands)
        sp, sf = self._score_operands()
        both = self.cdtype == torch.bfloat16 and ((self._score_fused and dscore_external is None) or bool(self._tn_splits))
        if both:   # feature_inf^T and pred^T, one launch
            self.call("dpc_transpose2d_bf16x2", sf, sp, D, self.finfT, self.predT, self.ld_d, R, D)
        else:
            self.call("dpc_transpose2d", sf, dc, D, self.finfT, dc, self.ld_d, R, D)
        if self._score_fused and dscore_external is None:
            if not both:
                self.call("dpc_transpose2d", sp, dc, D, self.predT, dc, self.ld_d, R, D)
            with self.tag("score"):
                for own, oth, othT, by_owner, out in ((sp, sf, self.finfT, 1, self.d_pred), (sf, sp, self.predT, 0, self.d_finf)):
                    n = self.call("dpc_score_bwd", own, oth, othT, self.ld_d, R, D, self.score_lse2, by_owner, self.score_ws)
                    self.call("dpc_reduce_unpack", self.score_ws, n, out, R, 1, D, D, 0, 1, 0)
        else:
            if self._score_fused:
                raise L.DpcError("backward(dscore_external=...) needs a materialised score: call forward(materialise=True)")
            with self.tag("score"):
                self.gemm_splitk(self.dscore, self.finfT, self.d_pred, R, D, self.ld_d, self.ld_d, self.ld_d)
                if self._tn_splits:
                    ns = C.c_int32(0)
                    self.call("dpc_gemm_tn_splitk", dc, R, D, R, self.dscore, self.ld_d, self.predT, self.ld_d, self.part, C.byref(ns))
                    self.call("dpc_reduce_unpack", self.part, ns.value, self.d_finf, R, 1, D, D, 0, 1, 0)
                else:
                    self.gemm_tn(self.dscore, self.ld_d, sp, D, self.d_finf, R, R, D)
                if self._negq_live and dscore_external is None:
                    # the queue's share of d_pred, summed behind the in-batch product; d_finf gets nothing (the bank is detached)
                    n = self.call("dpc_negq_bwd", sp, self._negq_ring, self._negq_ringT, self._negq_state, R, D, self._negq,
                                  self._negq_lse, self._negq_ws)
                    self.call("dpc_reduce_unpack", self._negq_ws, n, self.d_pred, R, 1, D, D, 0, 1, 1)
            if self._negq_live and dscore_external is None:
                # this batch's keys replace the oldest slot -- behind its own backward, so a batch never competes against itself
                self.call("dpc_negq_push", sf, self.finfT, self.ld_d, self._negq_ring, self._negq_ringT, self._negq_state, R, D,
                          self._negq)
                self._negq_live = False
        if self._snorm is not None:   # d_pred / d_finf are final: through the normalisation, in place, back to the raw operands
            with self.tag("score"):
                self.call("dpc_rownorm_bwd", self.pred, self.feat_inf, self.rnorm, self.d_pred, self.d_finf, R, D, dc, self._snorm[1], 1.0,
                          SCORE_NORM_EPS)
        # ---- predict loop + aggregation, reversed: one launch (G_all, dP1, dP2, d_featrelu come back)
        self.call("dpc_gru_chain_bwd", C.byref(self.gru_desc))
        # ---- temporal pool / split: the backbone's incoming gradient (the main stream's critical path goes on into the backbone)
        fs = self.feat_shape
        self.call("dpc_tpool_split_bwd", self.blocks[-1].out, self.d_featrelu, self.d_finf, dc, B, N, fs[1], SQ, D, P, self.d_feat)
        # ---- weight / bias grads of the ConvGRU and predictor, batched over all steps: ~20 small launches nothing waits for until
        # the optimizer -- on the side stream, beside layer4's backward (they share the split-K slab buffer with the backbone's
        # weight gradients, which queue behind them on the same stream)
        with self.side(site="head"):
            self._head_param_grads(dc)
        return self.d_feat

    def _head_param_grads(self, dc):
        D, M, P, Gm = self.D, self.M, self.P, self.G
        self._gru_param_grads(dc)
        self.gemm_tn(self.dP1, D, self.Hpred, D, Gm["network_pred.0.weight"].view(D, D), P * M, D, D)
        self.gemm_tn(self.dP2, D, self.P1_all, D, Gm["network_pred.2.weight"].view(D, D), P * M, D, D)
        self.call("dpc_colsum", self.dP1, dc, D, P * M, D, Gm["network_pred.0.bias"], 0, self.part, self.part.numel())
        self.call("dpc_colsum", self.dP2, dc, D, P * M, D, Gm["network_pred.2.bias"], 0, self.part, self.part.numel())

    def _forward_loss(self, block: Optional[torch.Tensor], train: bool, dropout_masks: Optional[torch.Tensor] = None):
        """forward without a score to return (consumed by the loss: bf16 logits, or never written) + CE / top-k.
        dropout_masks: train_step's explicit masks (tests)"""
        self.forward(block, train=train, dropout_masks=dropout_masks, materialise=False, use_neg_queue=train)
        self.loss_topk(with_grad=train)

    # ------------------------------------------------------------------ negative queue (csrc/neg_queue.hip)
    def set_neg_queue(self, k: int = 0):
        """Keep the keys (``feat_inf``, the encoded future blocks) of the last `k` training batches on the device and use them, detached,
        as extra negatives of every row of the engine-owned training step (train_step, its accumulation micro-batches, the captured
        steps): a row then competes against its R in-batch columns and the Q = filled * R keys of the bank.  The loss is the mean of
        logsumexp(R + Q logits) - target, the printed top-1/3/5 are accuracies among R + Q candidates, d_pred gets both parts, d_finf
        the in-batch part only, and after its backward the batch's own keys replace the oldest slot.  The in-batch logits are read
        rounded as before; the queue logits are the f32 accumulators, never materialised (per-row statistics, flash-style).

        A memory bank, not a momentum encoder: the keys are up to `k` updates old.  Evaluation (forward(train=False), validate,
        capture_eval_step) and the module boundary neither read nor write it.  load_params, checkpoint.resume and reset_neg_queue()
        empty it; so does a step or cycle the gradient guard skips (skip_nonfinite), so a batch with Inf / NaN features cannot poison
        the next `k` losses.  The bank is not checkpointed: it refills in `k` batches.  Each rank keeps its own.

        k = 0 turns it off and frees the ring: the step runs the lines it ran.  The current k again only empties the bank; another k
        allocates a new ring (buffers a captured step may still address are kept alive, and that step's replay raises).  Refused: another compute dtype than bf16, D not 256 or
        32, score_path="fused", inside a capture, in the middle of an accumulation cycle, k outside 0 .. 64.  k is among the scalars
        a captured step bakes in."""
        k = int(k)
        if k < 0 or k > L.NEGQ_MAX_SLOTS:
            raise ValueError(f"set_neg_queue: k must be 0 (off) or 1 .. {L.NEGQ_MAX_SLOTS}, got {k}")
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise L.DpcError("set_neg_queue: not while a graph is being captured")
        self._not_mid_cycle("set_neg_queue")
        if k == self._negq:   # nothing to allocate: the bank starts empty all the same
            self.reset_neg_queue()
            return
        if self._negq_ring is not None and self._capture_graphs:
            # a captured step holds these addresses; its replay raises (the baked scalars changed), but a parked graph must never
            # point at memory that went back to the allocator
            self._negq_retired.append((self._negq_state, self._negq_ring, self._negq_ringT, self._negq_stats, self._negq_lse, self._negq_ws))
        if k == 0:
            self._negq, self._negq_live = 0, False
            self._negq_state = self._negq_ring = self._negq_ringT = self._negq_stats = self._negq_lse = self._negq_ws = None
            return
        if self.cdtype != torch.bfloat16:
            raise L.DpcError("set_neg_queue: the negative queue needs the bf16 compute dtype (f32 is the parity mode against a reference "
                             "that has no bank)")
        if self.D not in (256, 32):
            raise L.DpcError(f"set_neg_queue: the feature size must be 256 or 32, not {self.D}")
        if self._score_path == "fused":
            raise L.DpcError('set_neg_queue: not with score_path="fused" (the benchmark arm of the in-batch score)')
        if self._ncls is not None and self._ncls[2] == 0.0:
            raise L.DpcError("set_neg_queue: the bank's keys are easy negatives, and set_neg_classes gave the easy class the weight 0")
        R, D = self.R, self.D
        pitch = L.negq_pitch(R)
        nf, nb = C.c_int64(0), C.c_int64(0)
        self.lib.call("dpc_negq_ws_floats", R, D, k, C.byref(nf), C.byref(nb))
        self._negq_state = torch.zeros((4,), dtype=torch.int32, device=self.device)
        self._negq_ring = torch.zeros((k, pitch, D), dtype=self.cdtype, device=self.device)
        self._negq_ringT = torch.zeros((k, D, pitch), dtype=self.cdtype, device=self.device)
        self._negq_stats = self.empty((R, 4), torch.float32)
        self._negq_lse = self.empty((R,), torch.float32)
        self._negq_ws = self.empty((max(nf.value, nb.value),), torch.float32)
        self._negq, self._negq_live = k, False
        self._negq_gen += 1

    @property
    def neg_queue(self) -> int:
        """slots of the negative queue (0: off)"""
        return self._negq

    def neg_queue_filled(self) -> int:
        """live slots of the bank, read back from the device record (a host synchronisation)"""
        return int(self._negq_state[1].item()) if self._negq else 0

    def reset_neg_queue(self):
        """empty the bank: the record back to zero (the ring's contents are dead from then on and never read)"""
        if self._negq:
            self._negq_state.zero_()
        self._negq_live = False

    # ------------------------------------------------------------------ negative classes in the loss (csrc/loss_cls.hip)
    def set_neg_classes(self, weights=(1, 1, 1), report: bool = False):
        """A weight per class of negatives inside the training loss's softmax, and a per-class report of where its mass sits.  The
        classes are those of the reference's mask (dpc/model_3d.py:86-96, dpc_mask_gen) for row (b, p, s) and column (b2, n, s2):
        spatial (same video, another position), temporal (same video and position, another predicted step), easy (another video; the
        negative queue's keys are easy).  With ``weights = (w_S, w_T, w_E)`` a row's term is log Z - target with
        Z = e^target + sum w_class e^logit, and d score = (w e^logit / Z - onehot) / R: a class of weight 0 is out of the loss and
        gets a gradient of exactly 0.  Top-1/3/5 stay the unweighted ranks, so accuracies compare across weights.

        ``report=True`` keeps, per training step, the means over the rows of the four shares of Z (positive, spatial, temporal, easy)
        and the fraction of rows with at least one column of a class strictly above the target: neg_class_stats().

        Only the engine-owned training forward (train_step, its micro-batches, the captured steps) runs the weighted entry;
        forward(train=False), validate, capture_eval_step, forward(materialise=True) and the module boundary run what they ran.
        Weights (1, 1, 1) without the report turn it off: the step runs the lines and launches it ran.  Refused: weights that are not
        three finite numbers in [0, 65536], w_E = 0 with a negative queue, score_path="fused", inside a capture, in the middle of an
        accumulation cycle.  The weights and the flag are among the scalars a captured step bakes in."""
        w = L.neg_class_weights(weights)
        report = bool(report)
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise L.DpcError("set_neg_classes: not while a graph is being captured")
        self._not_mid_cycle("set_neg_classes")
        on = report or w != (1.0, 1.0, 1.0)
        if on and self._sym > 0:
            raise L.DpcError("set_neg_classes: not with the symmetric loss (set_loss_sym): the column direction of the class weights is not built")
        if on and self._score_path == "fused":
            raise L.DpcError('set_neg_classes: not with score_path="fused" (its loss is formed inside the contraction)')
        if on and self._negq and w[2] == 0.0:
            raise L.DpcError("set_neg_classes: the easy class cannot have the weight 0 while a negative queue is on (its keys are easy)")
        if report and self._ncls_rows is None:
            self._ncls_rows = torch.zeros((self.R, 8), dtype=torch.float32, device=self.device)
            self._ncls_report = torch.zeros((8,), dtype=torch.float32, device=self.device)
        if not report and self._ncls_rows is not None:   # the report's buffers go; a parked graph never points at freed memory
            if self._capture_graphs:
                self._ncls_retired.append((self._ncls_rows, self._ncls_report))
            self._ncls_rows = self._ncls_report = None
        self._ncls = (w[0], w[1], w[2], report) if on else None
        self._ncls_desc = L.NegClasses(self.B, self.P, self.SQ, 0, w[0], w[1], w[2], 0.0) if on else None
        self._ncls_live = False

    @property
    def neg_classes(self):
        """((w_S, w_T, w_E), report) of the training loss: ((1.0, 1.0, 1.0), False) while off"""
        return ((1.0, 1.0, 1.0), False) if self._ncls is None else (self._ncls[:3], self._ncls[3])

    NEG_CLASS_KEYS = ("mass_pos", "mass_S", "mass_T", "mass_E", "above_S", "above_T", "above_E")

    def neg_class_stats(self) -> Dict[str, float]:
        """the report of the last training step (micro-batch): one 32-byte read-back, a host synchronisation"""
        if self._ncls is None or not self._ncls[3]:
            raise L.DpcError("neg_class_stats: the report is off (set_neg_classes(..., report=True))")
        v = self._ncls_report.cpu().tolist()
        return dict(zip(self.NEG_CLASS_KEYS, v[:7]))

    # ------------------------------------------------------------------ symmetric loss (csrc/loss_sym.hip)
    def set_loss_sym(self, w: float = 0.0):
        """The symmetric InfoNCE: over the same [R][R] logits each key (a column) also picks its prediction among the rows, the second
        half of the loss CLIP, NT-Xent and MoCo v3 train with.  With ``w`` in (0, 1]

            loss = (1 - w) mean_i Lr_i + w mean_j Lc_j,   Lc_j = logsumexp(S[:, j]) - S[j, j]

        Lr_i the row direction as it was (the negative queue in its denominator; the bank has keys but no predictions and takes no part
        in the column direction), and d score = ((1 - w)(pr - I) + w (pc - I)) / R, rounded once.  w = 0.5 is the symmetric loss.
        ``result`` keeps the row top-1/3/5, so accuracies compare across runs; loss_sym_stats() reads the two means and the column
        accuracies.  Everything behind ``dscore`` is what it was.

        Only the engine-owned training forward (train_step, its micro-batches, the captured steps) runs the symmetric entry;
        forward(train=False), validate, capture_eval_step, forward(materialise=True) and the module boundary run what they ran.
        w = 0 turns it off and frees the buffers: the step runs the lines and launches it ran.  Refused: w outside [0, 1] or not
        finite, score_path="fused", together with set_neg_classes (in either order), inside a capture, in the middle of an accumulation
        cycle.  w is among the scalars a captured step bakes in."""
        try:
            w = float(w)
        except (TypeError, ValueError):
            raise ValueError(f"set_loss_sym: the weight must be a number in [0, 1], got {w!r}") from None
        if not (math.isfinite(w) and 0.0 <= w <= 1.0):
            raise ValueError(f"set_loss_sym: the weight must be a number in [0, 1], got {w!r}")
        w = C.c_float(w).value   # the float32 the launcher sees
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise L.DpcError("set_loss_sym: not while a graph is being captured")
        self._not_mid_cycle("set_loss_sym")
        if w > 0 and self._score_path == "fused":
            raise L.DpcError('set_loss_sym: not with score_path="fused" (its loss is formed inside the contraction)')
        if w > 0 and self._ncls is not None:
            raise L.DpcError("set_loss_sym: not with set_neg_classes: the column direction of the class weights is not built")
        if w > 0 and self._sym_col_lse is None:
            nf = C.c_int64(0)
            self.lib.call("dpc_ce_sym_ws_floats", self.R, 0, C.byref(nf))
            self._sym_col_lse = self.empty((self.R,), torch.float32)
            self._sym_col_ws = self.empty((self.R, 2), torch.float32)
            self._sym_ws = self.empty((nf.value,), torch.float32)
            self._sym_result = torch.zeros((8,), dtype=torch.float32, device=self.device)
        if w == 0 and self._sym_col_lse is not None:   # the buffers go; a parked graph never points at freed memory
            if self._capture_graphs:
                self._sym_retired.append((self._sym_col_lse, self._sym_col_ws, self._sym_ws, self._sym_result))
            self._sym_col_lse = self._sym_col_ws = self._sym_ws = self._sym_result = None
        self._sym, self._sym_live = w, False

    @property
    def loss_sym(self) -> float:
        """the weight of the key-to-prediction direction of the training loss (0.0: off)"""
        return self._sym

    LOSS_SYM_KEYS = ("loss_row", "loss_col", "col_top1", "col_top3", "col_top5")

    def loss_sym_stats(self) -> Dict[str, float]:
        """the two directions of the last training step (micro-batch): one 32-byte read-back, a host synchronisation"""
        if not self._sym > 0:
            raise L.DpcError("loss_sym_stats: the symmetric loss is off (set_loss_sym(w > 0))")
        return dict(zip(self.LOSS_SYM_KEYS, self._sym_result.cpu().tolist()[:5]))

    # ------------------------------------------------------------------ cosine score (csrc/score_norm.hip)
    def set_score_norm(self, kind: str = "dot", temperature: float = 1.0):
        """The form of the contrastive score.  ``"dot"`` (temperature 1) is the reference's pred . feat_inf.  ``"cosine"`` scores
        L2-normalised operands over a temperature: s = (pred / |pred|) . (feat_inf / |feat_inf|) / T, F.normalize's semantics
        (eps 1e-12), so every logit lies in [-1/T, 1/T] and keys of different feature scale -- a memory bank's old and new ones --
        compete on equal terms.  dpc_rownorm_fwd runs behind the recurrence in every forward, train and eval alike (it defines the
        model's score), writes ``pred_n`` (scaled by float32(1 / T)) and ``finf_n`` and keeps the rows' 1 / norm in ``rnorm``; every
        consumer of the score operands -- the score contraction of all three routes, the negative queue and what it pushes, the
        transposes and products of the backward -- reads those; ``pred`` / ``feat_inf`` keep the raw values.  dpc_rownorm_bwd takes
        d_pred / d_finf back through the normalisation, in place, once both are final and before the recurrence's backward -- on the
        module boundary's backward(dscore_external) too.  Two launches per training step, one per evaluation step.

        "dot" frees the buffers: the step runs the lines it ran.  Every call empties the negative queue (keys of another geometry are
        not negatives of this one).  Refused: an unknown kind, "dot" with another temperature than 1, a temperature (or its f32
        reciprocal) that is not finite and positive, D not 256 or 32, inside a capture, in the middle of an accumulation cycle.  The
        form and T are among the scalars a captured step bakes in."""
        if kind not in ("dot", "cosine"):
            raise ValueError(f"set_score_norm: kind must be 'dot' or 'cosine', got {kind!r}")
        t = float(temperature)
        if not (math.isfinite(t) and t > 0):
            raise ValueError(f"set_score_norm: the temperature must be finite and positive, got {temperature}")
        if kind == "dot" and t != 1.0:
            raise ValueError("set_score_norm: a temperature other than 1 needs kind='cosine' (the dot-product score is the reference's)")
        scale = C.c_float(1.0 / t).value   # float32(1 / T), rounded once, here
        if not (math.isfinite(scale) and scale > 0):
            raise ValueError(f"set_score_norm: 1 / temperature is not a finite positive float32 (temperature {temperature})")
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise L.DpcError("set_score_norm: not while a graph is being captured")
        self._not_mid_cycle("set_score_norm")
        if kind == "cosine" and self.D not in (256, 32):
            raise L.DpcError(f"set_score_norm: the feature size must be 256 or 32, not {self.D}")
        if self.pred_n is not None and self._capture_graphs and kind == "dot":
            self._snorm_retired.append((self.pred_n, self.finf_n, self.rnorm))   # a parked graph never points at freed memory
        self.reset_neg_queue()
        if kind == "dot":
            self._snorm = None
            self.pred_n = self.finf_n = self.rnorm = None
            return
        if self.pred_n is None:
            self.pred_n, self.finf_n = self.empty((self.R, self.D), self.cdtype), self.empty((self.R, self.D), self.cdtype)
            self.rnorm = self.empty((2 * self.R,), torch.float32)
        self._snorm = (t, scale)

    @property
    def score_norm(self):
        """(kind, temperature) of the score: ("dot", 1.0) or ("cosine", T)"""
        return ("dot", 1.0) if self._snorm is None else ("cosine", self._snorm[0])

    def release_captures(self):
        super().release_captures()
        self._negq_retired.clear()   # no capture of this engine is left to replay on an earlier ring
        self._snorm_retired.clear()
        self._ncls_retired.clear()
        self._sym_retired.clear()

    def load_params(self, params: Dict[str, torch.Tensor]):
        super().load_params(params)
        self.reset_neg_queue()   # keys encoded with other weights are not negatives of these

    def train_step(self, block: torch.Tensor, dropout_masks: Optional[torch.Tensor] = None, allreduce=None) -> torch.Tensor:
        """forward + CE/top-k + backward (+ gradient all-reduce) + Adam.  Returns device f32[4] = loss, top1, top3, top5."""
        self._not_swapped("train_step")
        self._forward_loss(block, True, dropout_masks=dropout_masks)
        if self._accum_n > 1:   # one micro-batch of the cycle (set_grad_accum)
            self._accum_micro_step(allreduce)
            return self.result
        self._backward_and_exchange(allreduce)
        self.adam_step()
        return self.result
