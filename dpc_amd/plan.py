"""Which gfx950 kernel serves which convolution of the 2d3d-ResNet -- the static schedule's kernel plan, queryable
without a GPU (``dpc_conv_plan`` runs the library's own dispatch code with the launch skipped, include/dpc_hip.h).

``walk_blocks`` is the one walk over the reference's layer plan (backbone/resnet_2d3d.py:205-284), ``block_geometry`` the one
statement of a block's conv geometry and ``fold_decision`` the one decision which backward pieces ride in input-gradient
epilogues; ``unit_descs`` builds the three descriptors of a Conv3d + BatchNorm3d unit (forward, input-gradient,
weight-gradient).  The engine builds itself from the same functions, so the table printed here is what a train step launches.  tests/test_plan.py pins the table
for BASELINE.json's configurations; ``python -m dpc_amd.plan cfg2`` prints it.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import torch

from . import _lib as L

LAYER_PLAN = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}  # backbone/resnet_2d3d.py:274-284
LAYER_WIDTH = (64, 128, 256, 256)                                    # resnet_2d3d.py:217-223


def out_shape_of(in_shape, k, s, p, stem=False):
    N, T, H, W = in_shape
    if stem:
        return (N, T, H, W)  # space-to-depth grid == output grid
    return (N, (T + 2 * p[0] - k[0]) // s[0] + 1, (H + 2 * p[1] - k[1]) // s[1] + 1, (W + 2 * p[2] - k[2]) // s[2] + 1)


def unit_descs(Ci: int, Co: int, k, s, p, in_shape, dtype: torch.dtype, stem: bool = False):
    """(forward, input-gradient, weight-gradient) descriptors of one conv unit on a channels-last [N,T,H,W,Ci] input"""
    N, T, H, W = in_shape
    No, To, Ho, Wo = out_shape_of(in_shape, k, s, p, stem)
    taps = k[0] * k[1] * k[2]
    dc = L.dtype_code(dtype)
    Kp = taps * Ci
    desc_f = L.ConvDesc(dc, dc, 0, N, To, Ho, Wo, T, H, W, Ci, Ci, Co, Kp, Co, *k, *s, *p)
    # input-gradient: rows enumerate the forward input grid, source is dy on the output grid
    desc_d = L.ConvDesc(dc, dc, 1, N, T, H, W, To, Ho, Wo, Co, Co, Ci, taps * Co, Ci, *k, *s, *p)
    desc_w = L.ConvDesc(dc, L.F32, 0, N, To, Ho, Wo, T, H, W, Ci, Ci, Co, Kp, Co, *k, *s, *p)
    return desc_f, desc_d, desc_w


def walk_blocks(network: str, widths: Sequence[int] = LAYER_WIDTH):
    """the BasicBlocks of the backbone in forward order (backbone/resnet_2d3d.py:205-257):
    yields (prefix "layerL.B.", cin, planes, is3d, stride, has_ds, last)"""
    if network not in LAYER_PLAN:
        raise IOError("model type is wrong")  # backbone/select_backbone.py:19
    plan = LAYER_PLAN[network]
    inplanes = widths[0]
    for li in range(4):
        planes = widths[li]
        for bi in range(plan[li]):
            stride = 2 if (li > 0 and bi == 0) else 1
            has_ds = bi == 0 and (stride != 1 or inplanes != planes)
            yield f"layer{li + 1}.{bi}.", inplanes if bi == 0 else planes, planes, li >= 2, stride, has_ds, li == 3 and bi == plan[li] - 1
        inplanes = planes


def block_geometry(is3d: bool, stride: int):
    """(k, s, p) of a block's conv1; conv2 is the same at stride 1, the downsample a 1x1x1 conv at s without padding"""
    k = (3, 3, 3) if is3d else (1, 3, 3)
    p = (1, 1, 1) if is3d else (0, 1, 1)
    s = (stride,) * 3 if is3d else (1, stride, stride)
    return k, s, p


def backbone_units(network: str, size: int, batch: int, num_seq: int = 8, seq_len: int = 5,
                   widths: Sequence[int] = LAYER_WIDTH) -> "List[Dict]":
    """every conv unit of the backbone in forward order: name, geometry and how the backward uses its input-gradient"""
    BN, H = batch * num_seq, size
    units = [dict(name="conv1", Ci=16, Co=widths[0], k=(1, 4, 4), s=(1, 1, 1), p=(0, 2, 2), in_shape=(BN, seq_len, H // 2, H // 2),
                  stem=True, dgrad=None)]
    hp = (H // 2 - 1) // 2 + 1
    shape = (BN, seq_len, hp, hp)
    for pre, cin, planes, is3d, stride, has_ds, _ in walk_blocks(network, widths):
        k, s, p = block_geometry(is3d, stride)
        mid = out_shape_of(shape, k, s, p)
        # c1's input-gradient carries the residual branch as its addend unless a downsample accumulates in place afterwards
        units.append(dict(name=pre + "conv1", Ci=cin, Co=planes, k=k, s=s, p=p, in_shape=shape, stem=False,
                          dgrad="plain" if has_ds else "addend"))
        units.append(dict(name=pre + "conv2", Ci=planes, Co=planes, k=k, s=(1, 1, 1), p=p, in_shape=mid, stem=False, dgrad="plain"))
        if has_ds:
            units.append(dict(name=pre + "downsample.0", Ci=cin, Co=planes, k=(1, 1, 1), s=s, p=(0, 0, 0), in_shape=shape,
                              stem=False, dgrad="inplace"))
        shape = mid
    return units


def ex_supported(lib: L.Lib, desc_d, addend: bool, gate: bool, bnred: bool) -> bool:
    """dpc_conv_igemm_ex serves this input-gradient with the given fused pieces WITHOUT demoting it from a specialised kernel
    to the generic implicit GEMM (the query runs the library's own dispatch code)"""
    ex = L.conv_plan(lib, desc_d, L.PLAN_IGEMM, addend=addend, addend_mask=gate, bnred=bnred)
    plain = L.conv_plan(lib, desc_d, L.PLAN_IGEMM, addend=addend)
    return bool(ex) and (not ex.startswith("igemm_kernel") or plain.startswith("igemm_kernel"))


def fold_decision(lib: L.Lib, d1, d2, has_ds: bool, final_relu: bool, has_prev: bool) -> "Tuple[bool, bool, bool]":
    """which backward pieces of a BasicBlock ride in input-gradient epilogues, from the input-gradient descriptors of its conv1
    (d1) and conv2 (d2) (dpc_conv_igemm_ex + the plan query):
    fold_c1   conv2's input-gradient takes bn1's backward reduction;
    gate      conv1's input-gradient adds the block's incoming gradient gated by the output ReLU mask (no dz tensor);
    fold_prev ... and takes the backward reduction of the PREVIOUS block's bn2, whose output gradient it writes."""
    fold_c1 = ex_supported(lib, d2, False, False, True)
    gate = (not has_ds) and ex_supported(lib, d1, True, final_relu, False)
    fold_prev = bool(has_prev and gate and ex_supported(lib, d1, True, final_relu, True))
    return fold_c1, gate, fold_prev


def fold_table(lib: L.Lib, network: str, size: int, batch: int, dtype: torch.dtype, **kw) -> "List[Tuple[str, bool, bool, bool]]":
    """per BasicBlock: (block, fold_c1, gate, fold_prev) -- fold_decision on the descriptors the engine builds (its own switches,
    fold=False / DPC_FOLD_RED, come on top there: engine._Block.plan_backward)"""
    units = {u["name"]: u for u in backbone_units(network, size, batch, **kw)}
    rows = []
    for pre, _, _, _, _, has_ds, last in walk_blocks(network, kw.get("widths", LAYER_WIDTH)):
        d1, d2 = (unit_descs(u["Ci"], u["Co"], u["k"], u["s"], u["p"], u["in_shape"], dtype)[1]
                  for u in (units[pre + "conv1"], units[pre + "conv2"]))
        rows.append((pre[:-1],) + fold_decision(lib, d1, d2, has_ds, not last, bool(rows)))
    return rows


def plan_table(lib: L.Lib, network: str, size: int, batch: int, dtype: torch.dtype, **kw) -> "List[Tuple[str, str, str]]":
    """(unit, op, kernel) for every conv launch of one train step's backbone"""
    rows = []
    for u in backbone_units(network, size, batch, **kw):
        f, d, w = unit_descs(u["Ci"], u["Co"], u["k"], u["s"], u["p"], u["in_shape"], dtype, u["stem"])
        rows.append((u["name"], "fwd", L.conv_plan(lib, f, L.PLAN_IGEMM, stats=True)))
        if u["dgrad"] is not None:
            rows.append((u["name"], "dgrad" + ("" if u["dgrad"] == "plain" else "+" + u["dgrad"]),
                         L.conv_plan(lib, d, L.PLAN_IGEMM, addend=u["dgrad"] != "plain")))
        rows.append((u["name"], "wgrad", L.conv_plan(lib, w, L.PLAN_WGRAD, dy_ld=u["Co"])))
    return rows


CONFIGS = {"cfg2": ("resnet18", 128, 128), "cfg4": ("resnet34", 224, 44), "cfg5": ("resnet34", 224, 64)}


if __name__ == "__main__":
    import sys
    lib = L.Lib(L.HIP_LIB_PATH, "probe")  # dlopen only: the query launches nothing and needs no GPU
    for cfg in sys.argv[1:] or ["cfg2"]:
        net, size, batch = CONFIGS[cfg]
        for dt in (torch.bfloat16, torch.float32):
            print(f"# {cfg}: {net} {size}^2 batch {batch} {dt}")
            for name, op, kern in plan_table(lib, net, size, batch, dt):
                print(f"{name:24s} {op:14s} {kern}")
            for name, a, b, c in fold_table(lib, net, size, batch, dt):
                print(f"{name:24s} fused epilogues: bn1 reduction in conv2's input-gradient {int(a)}, gated residual {int(b)}, "
                      f"previous bn2 reduction {int(c)}")
