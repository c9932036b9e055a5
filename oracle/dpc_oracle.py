"""CPU oracle for the DPC-RNN training step.  TEST INFRASTRUCTURE ONLY.

This file is a functional (module-free) torch-CPU fp32/fp64 restatement of the
reference algorithm.  Only ``tests/``, ``__graft_entry__.smoke()`` and the
``cpu_baseline`` leg of ``bench.py`` may import it; the product path
(``dpc_amd``) never does and fails loudly when its HIP library is missing.

Parity pinning: the reference ships no tests or golden vectors,
so this oracle is pinned against outputs of the reference itself, imported on
CPU in the build container by ``tests/golden/make_golden.py`` (fixtures under
``tests/golden/*.npz``; ``tests/test_oracle_golden.py`` checks them).

Every function cites the reference lines (relative to /root/reference) whose
arithmetic it restates.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

Params = Dict[str, torch.Tensor]

BN_EPS = 1e-5  # torch.nn.BatchNorm3d default, backbone/resnet_2d3d.py:55,93,212

# backbone/resnet_2d3d.py:274-284 -- BasicBlock plans (2d,2d,3d,3d)
LAYER_PLAN = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}
LAYER_WIDTH = (64, 128, 256, 256)  # backbone/resnet_2d3d.py:217-222 (layer4 stays 256)
FEATURE_SIZE = 256  # backbone/select_backbone.py:7,10


# --------------------------------------------------------------------------
# configuration-derived sizes (dpc/model_3d.py:24-25)
# --------------------------------------------------------------------------
def derived_sizes(sample_size: int, seq_len: int = 5) -> Tuple[int, int]:
    last_duration = int(math.ceil(seq_len / 4))
    last_size = int(math.ceil(sample_size / 32))
    return last_duration, last_size


# --------------------------------------------------------------------------
# parameter inventory: names and shapes of the reference state_dict
# (dpc/model_3d.py:28-40, backbone/resnet_2d3d.py:205-257, backbone/convrnn.py:13-15,55-58)
# --------------------------------------------------------------------------
def param_shapes(network: str = "resnet18", widths: Sequence[int] = LAYER_WIDTH,
                 feature: Optional[int] = None, with_alias: bool = True) -> "Dict[str, Tuple[int, ...]]":
    """Ordered {state_dict key: shape}.  ``widths``/``feature`` default to the
    reference's; narrower values give the width-parametric test nets (the
    reference block classes are width-parametric, resnet_2d3d.py:50,86)."""
    plan = LAYER_PLAN[network]
    feature = widths[3] if feature is None else feature
    out: Dict[str, Tuple[int, ...]] = {}
    out["backbone.conv1.weight"] = (widths[0], 3, 1, 7, 7)
    out["backbone.bn1.weight"] = (widths[0],)
    out["backbone.bn1.bias"] = (widths[0],)
    inplanes = widths[0]
    for li in range(4):
        planes = widths[li]
        is3d = li >= 2
        k = (3, 3, 3) if is3d else (1, 3, 3)
        stride = 1 if li == 0 else 2
        for bi in range(plan[li]):
            pre = f"backbone.layer{li + 1}.{bi}."
            cin = inplanes if bi == 0 else planes
            out[pre + "conv1.weight"] = (planes, cin) + k
            out[pre + "bn1.weight"] = (planes,)
            out[pre + "bn1.bias"] = (planes,)
            out[pre + "conv2.weight"] = (planes, planes) + k
            out[pre + "bn2.weight"] = (planes,)
            out[pre + "bn2.bias"] = (planes,)
            if bi == 0 and (stride != 1 or inplanes != planes):
                out[pre + "downsample.0.weight"] = (planes, inplanes, 1, 1, 1)
                out[pre + "downsample.1.weight"] = (planes,)
                out[pre + "downsample.1.bias"] = (planes,)
        inplanes = planes
    cells = ["agg.ConvGRUCell_00."] + (["agg.cell_list.0."] if with_alias else [])
    for pre in cells:
        for gate in ("reset_gate", "update_gate", "out_gate"):
            out[pre + gate + ".weight"] = (feature, 2 * feature, 1, 1)
            out[pre + gate + ".bias"] = (feature,)
    for idx in (0, 2):
        out[f"network_pred.{idx}.weight"] = (feature, feature, 1, 1)
        out[f"network_pred.{idx}.bias"] = (feature,)
    return out


def make_params_pcg(network: str = "resnet18", widths: Sequence[int] = LAYER_WIDTH,
                    dtype=torch.float32) -> Params:
    """Portable weight recipe used on both sides of every parity test
    (SURVEY.md §8c G3): key i -> PCG64(1000+i) normals; convs scaled
    1/sqrt(fan_in); BN gamma 1+0.1n, beta 0.1n; biases 0.05n; the ConvGRU
    alias keys (backbone/convrnn.py:55-58) share the first cell's tensors."""
    shapes = param_shapes(network, widths)
    params: Params = {}
    for i, (k, shp) in enumerate(shapes.items()):
        if k.startswith("agg.cell_list.0."):
            params[k] = params[k.replace("agg.cell_list.0.", "agg.ConvGRUCell_00.")]
            continue
        n = np.random.Generator(np.random.PCG64(1000 + i)).standard_normal(shp, dtype=np.float32)
        if len(shp) >= 4:
            fan_in = int(np.prod(shp[1:]))
            v = n / np.float32(math.sqrt(fan_in))
        elif ".bn" in k or "downsample.1" in k:
            v = (1.0 + 0.1 * n) if k.endswith("weight") else 0.1 * n
        else:
            v = 0.05 * n
        params[k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dtype)
    return params


def make_input_pcg(B: int, num_seq: int, seq_len: int, size: int, seed: int = 7) -> torch.Tensor:
    x = np.random.Generator(np.random.PCG64(seed)).standard_normal(
        (B, num_seq, 3, seq_len, size, size), dtype=np.float32)
    return torch.from_numpy(x)


# --------------------------------------------------------------------------
# backbone (backbone/resnet_2d3d.py)
# --------------------------------------------------------------------------
def bn_batch(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = BN_EPS) -> torch.Tensor:
    """BatchNorm3d with track_running_stats=False (dpc/model_3d.py:28): batch
    statistics (biased variance) in train AND eval (torch functional/batch_norm)."""
    dims = (0, 2, 3, 4)
    mean = x.mean(dims, keepdim=True)
    var = x.var(dims, unbiased=False, keepdim=True)
    shp = (1, -1, 1, 1, 1)
    return (x - mean) / torch.sqrt(var + eps) * gamma.view(shp) + beta.view(shp)


def basic_block(x: torch.Tensor, p: Params, pre: str, is3d: bool, stride: int,
                final_relu: bool = True) -> torch.Tensor:
    """BasicBlock2d (resnet_2d3d.py:83-116) / BasicBlock3d (:47-80)."""
    if is3d:
        s1, pad = (stride,) * 3, (1, 1, 1)
    else:
        s1, pad = (1, stride, stride), (0, 1, 1)
    out = F.conv3d(x, p[pre + "conv1.weight"], None, s1, pad)
    out = F.relu(bn_batch(out, p[pre + "bn1.weight"], p[pre + "bn1.bias"]))
    out = F.conv3d(out, p[pre + "conv2.weight"], None, 1, pad)
    out = bn_batch(out, p[pre + "bn2.weight"], p[pre + "bn2.bias"])
    if (pre + "downsample.0.weight") in p:  # resnet_2d3d.py:232-245
        res = F.conv3d(x, p[pre + "downsample.0.weight"], None, s1, 0)
        res = bn_batch(res, p[pre + "downsample.1.weight"], p[pre + "downsample.1.bias"])
    else:
        res = x
    out = out + res
    return F.relu(out) if final_relu else out


def ste_round_bf16(x: torch.Tensor) -> torch.Tensor:
    """round to bf16 in the forward, identity in the backward: how a tensor the engine STORES in bf16 enters the next op while the
    gradient flows through unchanged (the engine's backward kernels differentiate the unrounded op at the stored values)"""
    return x + (x.to(torch.bfloat16).to(x.dtype) - x).detach()


def basic_block_rounded(x: torch.Tensor, p: Params, pre: str, is3d: bool, stride: int, final_relu: bool = True) -> torch.Tensor:
    """basic_block with the engine's throughput-mode storage points: weights, raw conv outputs and activations pass through
    ste_round_bf16; BatchNorm statistics are those of the STORED raw outputs, accumulation stays full precision.  The block-local
    gradient checks of the bf16 mode (tests/test_block_grads_gpu.py) differentiate this, not the fp32 block."""
    r = ste_round_bf16
    if is3d:
        s1, pad = (stride,) * 3, (1, 1, 1)
    else:
        s1, pad = (1, stride, stride), (0, 1, 1)
    raw1 = r(F.conv3d(x, r(p[pre + "conv1.weight"]), None, s1, pad))
    act1 = r(F.relu(bn_batch(raw1, p[pre + "bn1.weight"], p[pre + "bn1.bias"])))
    raw2 = r(F.conv3d(act1, r(p[pre + "conv2.weight"]), None, 1, pad))
    out = bn_batch(raw2, p[pre + "bn2.weight"], p[pre + "bn2.bias"])
    if (pre + "downsample.0.weight") in p:
        rawd = r(F.conv3d(x, r(p[pre + "downsample.0.weight"]), None, s1, 0))
        res = bn_batch(rawd, p[pre + "downsample.1.weight"], p[pre + "downsample.1.bias"])
    else:
        res = x
    out = out + res
    return r(F.relu(out) if final_relu else out)


# --------------------------------------------------------------------------
# the stem: conv1 (1,7,7)/(1,2,2) -> bn1 -> ReLU -> MaxPool3d (1,3,3)/(1,2,2)/(0,1,1) (resnet_2d3d.py:211-214,260-263)
# --------------------------------------------------------------------------
STEM_W = "backbone.conv1.weight"
STEM_G, STEM_B = "backbone.bn1.weight", "backbone.bn1.bias"


def pool_by_route(act: torch.Tensor, route: torch.Tensor) -> torch.Tensor:
    """MaxPool3d((1,3,3),(1,2,2),(0,1,1)) of act [N,C,T,H,W] with the window's tap given instead of searched: route [N,C,T,Ho,Wo]
    holds kh*3+kw of the chosen tap, 9 = the window passes nothing (the engine's argmax byte).  Differentiable: the gradient goes to
    the chosen tap only, as max-pool's does to its argmax."""
    N, Cc, T, H, W = act.shape
    a = act.permute(0, 2, 1, 3, 4).reshape(N * T, Cc, H, W)
    win = F.unfold(a, 3, padding=1, stride=2).view(N * T, Cc, 9, -1)
    win = torch.cat([win, torch.zeros_like(win[:, :, :1])], 2)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    r = route.permute(0, 2, 1, 3, 4).reshape(N * T, Cc, 1, Ho * Wo).long()
    out = win.gather(2, r).view(N, T, Cc, Ho, Wo)
    return out.permute(0, 2, 1, 3, 4)


def _stem(x: torch.Tensor, p: Params, r, route: Optional[torch.Tensor]):
    raw = r(F.conv3d(r(x), r(p[STEM_W]), None, (1, 2, 2), (0, 3, 3)))
    act = F.relu(bn_batch(raw, p[STEM_G], p[STEM_B]))
    pooled = F.max_pool3d(act, (1, 3, 3), (1, 2, 2), (0, 1, 1)) if route is None else pool_by_route(act, route)
    return r(pooled), raw


def stem_rounded(x: torch.Tensor, p: Params, route: Optional[torch.Tensor] = None):
    """the stem with the bf16 engine's storage points: the packed input, the weight, the stored raw conv output and the pooled output
    pass through ste_round_bf16; BatchNorm statistics are those of the STORED raw values; accumulation stays f32.  x [N,3,T,H,W].
    Returns (pooled, raw), NCTHW.  route: the pooling taps to use instead of max-pool's own argmax (pool_by_route)."""
    return _stem(x, p, ste_round_bf16, route)


def stem_unrounded(x: torch.Tensor, p: Params, route: Optional[torch.Tensor] = None):
    """the stem of the f32 engine: stem_rounded without the rounding"""
    return _stem(x, p, lambda t: t, route)


def _ulp(v: torch.Tensor, dtype) -> torch.Tensor:
    """one unit in the last place of |v| in `dtype` (bf16: 8 significant bits, f32: 24)"""
    bits = 8 if dtype == torch.bfloat16 else 24
    _, e = torch.frexp(v.abs().float())
    return torch.ldexp(torch.ones_like(v, dtype=torch.float32), e - bits)


def _taps(t: torch.Tensor, Ho: int, Wo: int):
    """the nine (kh, kw) views of a [F,C,H+2,W+2] padded tensor under the 3x3 / stride-2 pooling windows, scan order"""
    return [t[:, :, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2] for kh in range(3) for kw in range(3)]


def stem_pool_route(pre: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, dtype, floor: torch.Tensor, ulps: float = 1.0):
    """the max-pool routing of the engine (pool.hip: bn_relu_maxpool_fwd) from the pre-ReLU BatchNorm output pre [F,C,H,W] (frames
    first): the tap kh*3+kw of the FIRST maximum in scan order among the in-image taps, 9 when that maximum is <= 0 (the ReLU passes
    no gradient).  pre = raw * scale + shift ([1,C,1,1] each).  Also returns the pooled value, the NEAR-TIE mask -- windows whose two
    best candidates (the two largest taps, and 0 = no route) lie within `ulps` ulps of the STORED raw value (in `dtype`, mapped through
    the scale), or within `floor` [C] (the f32 cancellation scale of the channel), where another evaluation of the same stored values
    may choose the other one -- and each window's first in-image tap.  All [F,C,Ho,Wo]."""
    Fr, Cc, H, W = pre.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    taps = _taps(F.pad(pre.float(), (1, 1, 1, 1), value=float("-inf")), Ho, Wo)
    t1 = torch.full((Fr, Cc, Ho, Wo), float("-inf"))
    t2 = t1.clone()
    arg = torch.zeros(Fr, Cc, Ho, Wo, dtype=torch.uint8)
    for k, v in enumerate(taps):
        upd = v > t1                      # strictly greater: the first maximum stays
        t2 = torch.where(upd, t1, torch.maximum(t2, v))
        t1 = torch.where(upd, v, t1)
        arg.masked_fill_(upd, k)
    route = torch.where(t1 > 0, arg, torch.full_like(arg, 9))
    gap = (t1 - t2.clamp_min(0.0)).abs()
    rmax = torch.maximum(((t1 - shift) / scale).abs(), ((t2 - shift) / scale).abs())   # the stored values of the two best taps
    near = gap <= torch.maximum(ulps * _ulp(rmax, dtype) * scale.abs(), floor.view(1, Cc, 1, 1))
    oh = torch.arange(Ho).view(1, 1, Ho, 1)
    ow = torch.arange(Wo).view(1, 1, 1, Wo)
    first = ((oh < 1).to(torch.uint8) * 3 + (ow < 1).to(torch.uint8)).expand(Fr, Cc, Ho, Wo)
    return route, near, t1.clamp_min(0.0), first


def route_to_input(dy: torch.Tensor, route: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """the max-pool backward: dy [F,C,Ho,Wo] summed into the taps route [F,C,Ho,Wo] names (9: nowhere) -> [F,C,H,W]"""
    Fr, Cc, Ho, Wo = dy.shape
    out = torch.zeros(Fr, Cc, H + 2, W + 2, dtype=dy.dtype)
    for k, v in enumerate(_taps(out, Ho, Wo)):
        v += torch.where(route == k, dy, torch.zeros((), dtype=dy.dtype))
    return out[:, :, 1:H + 1, 1:W + 1]


def stem_backward_chunked(x: torch.Tensor, raw: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, dy: torch.Tensor, w_shape,
                          stored=torch.bfloat16, round_x: bool = True, chunk: int = 64, engine_route: Optional[torch.Tensor] = None,
                          drop_xhat_term: bool = False, route_first: bool = False, on_chunk=None,
                          tie_ulps: float = 1.0) -> Dict[str, object]:
    """closed-form backward of the stem for batches too large for autograd on the CPU, frame chunk by frame chunk, f64 sums.

    x [F,3,H,W] the input frames (frame = clip * T + t, the engine's order); raw [F,Hs,Ws,C] the STORED conv output (its stored dtype,
    widened one chunk at a time); gamma, beta [C]; dy [F,Ho,Wo,C] the gradient at the pooled output; w_shape the weight's
    (C,3,1,7,7).  round_x: the input enters the weight gradient bf16-rounded (the engine's packed operand).

    Routing is this function's own (stem_pool_route); engine_route [F,Ho,Wo,C], when given, replaces it on near-tie windows only,
    and the windows outside those where it disagrees are counted (tie_ulps: the width of a near tie, stem_pool_route).  Mean and invstd come from f64 sums of the stored raw values;
    dgamma = sum dz_bn * xhat, dbeta = sum dz_bn, and dz = gamma * invstd * (dz_bn - mean(dz_bn) - xhat * mean(dz_bn * xhat)), where
    dz_bn is dy routed through the pooling; dW = sum over chunks of the f32 weight gradient of the (1,7,7)/(1,2,2)/(0,3,3) conv.

    Mutations, for tests that must show they fail: drop_xhat_term leaves out the mean(dz_bn * xhat) term, route_first sends each
    routed window's gradient to its first in-image tap instead of its argmax.  on_chunk(f0, f1, d) sees, per chunk, the oracle's
    pooled output, dz (both [f,C,h,w], f32), its routing and near-tie mask.  Without on_chunk, chunks where dy is zero are not
    routed, and the near-tie fraction and routing mismatches cover the other chunks only."""
    Fr, Hs, Ws, Cc = raw.shape
    n = float(Fr * Hs * Ws)
    f64 = torch.float64
    s1 = torch.zeros(Cc, dtype=f64)
    s2 = torch.zeros(Cc, dtype=f64)
    for f0 in range(0, Fr, chunk):
        r = raw[f0:f0 + chunk].to(f64).reshape(-1, Cc)
        s1 += r.sum(0)
        s2 += (r * r).sum(0)
    mean = s1 / n
    var = (s2 / n - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    g64, b64 = gamma.to(f64), beta.to(f64)
    scale = (g64 * invstd).float().view(1, Cc, 1, 1)
    shift = (b64 - mean * g64 * invstd).float().view(1, Cc, 1, 1)
    floor = (1e-6 * (1.0 + b64.abs() + (mean * g64 * invstd).abs())).float()
    cv = lambda t: t.permute(0, 3, 1, 2)  # channels-last chunk -> [f,C,h,w]

    def routed(f0):
        rc = cv(raw[f0:f0 + chunk]).float()
        dyc = cv(dy[f0:f0 + chunk]).float()
        xhat = (rc.to(f64) - mean.view(1, Cc, 1, 1)) * invstd.view(1, Cc, 1, 1)
        if on_chunk is None and not bool(dyc.any()):   # no gradient in these frames: nothing to route (nor to count)
            return torch.zeros_like(rc), xhat, dict(near=torch.zeros((), dtype=torch.bool), mismatch=0)
        route, near, pooled, first = stem_pool_route(rc * scale + shift, scale, shift, stored, floor, tie_ulps)
        own = route
        if engine_route is not None:
            er = cv(engine_route[f0:f0 + chunk])
            route = torch.where(near, er, route)
            bad = int(((er != own) & ~near).sum())
        else:
            bad = 0
        if route_first:
            route = torch.where(route < 9, first, route)
        dzb = route_to_input(dyc, route, Hs, Ws)
        return dzb, xhat, dict(route=route, own_route=own, near=near, pooled=pooled, mismatch=bad)

    # pass 1: the BatchNorm-backward sums
    dbeta = torch.zeros(Cc, dtype=f64)
    dgamma = torch.zeros(Cc, dtype=f64)
    n_near = n_bad = 0
    for f0 in range(0, Fr, chunk):
        dzb, xhat, info = routed(f0)
        dbeta += dzb.to(f64).sum((0, 2, 3))
        dgamma += (dzb.to(f64) * xhat).sum((0, 2, 3))
        n_near += int(info["near"].sum())
        n_bad += info["mismatch"]
    c1 = (dbeta / n).view(1, Cc, 1, 1)
    c2 = (dgamma / n).view(1, Cc, 1, 1) if not drop_xhat_term else torch.zeros(1, Cc, 1, 1, dtype=f64)
    gi = (g64 * invstd).view(1, Cc, 1, 1)
    # pass 2: dz and the weight gradient
    dw = torch.zeros(w_shape[0], w_shape[1], w_shape[3], w_shape[4], dtype=f64)
    for f0 in range(0, Fr, chunk):
        dzb, xhat, info = routed(f0)
        dz = (gi * (dzb.to(f64) - c1 - xhat * c2)).float()
        xc = x[f0:f0 + chunk].float()
        if round_x:
            xc = xc.to(torch.bfloat16).float()
        dw += torch.nn.grad.conv2d_weight(xc, tuple(dw.shape), dz, stride=2, padding=3).to(f64)
        if on_chunk is not None:
            on_chunk(f0, min(f0 + chunk, Fr), dict(info, dz=dz))
    n_win = Fr * Cc * ((Hs - 1) // 2 + 1) * ((Ws - 1) // 2 + 1)
    return dict(mean=mean, invstd=invstd, dgamma=dgamma, dbeta=dbeta, dw=dw.view(w_shape), near_frac=n_near / n_win,
                route_mismatch=n_bad)


def backbone_forward(p: Params, x: torch.Tensor, network: str = "resnet18") -> torch.Tensor:
    """ResNet2d3d_full.forward (resnet_2d3d.py:259-270); x is [BN,3,T,H,W]."""
    plan = LAYER_PLAN[network]
    x = F.conv3d(x, p["backbone.conv1.weight"], None, (1, 2, 2), (0, 3, 3))
    x = F.relu(bn_batch(x, p["backbone.bn1.weight"], p["backbone.bn1.bias"]))
    x = F.max_pool3d(x, (1, 3, 3), (1, 2, 2), (0, 1, 1))
    for li in range(4):
        for bi in range(plan[li]):
            stride = 2 if (li > 0 and bi == 0) else 1
            last = li == 3 and bi == plan[li] - 1  # resnet_2d3d.py:249-252
            x = basic_block(x, p, f"backbone.layer{li + 1}.{bi}.", li >= 2, stride, final_relu=not last)
    return x


# --------------------------------------------------------------------------
# ConvGRU (backbone/convrnn.py)
# --------------------------------------------------------------------------
def convgru_cell(x: torch.Tensor, h: torch.Tensor, p: Params, pre: str = "agg.ConvGRUCell_00.") -> torch.Tensor:
    """ConvGRUCell.forward (convrnn.py:24-34), kernel_size 1."""
    comb = torch.cat([x, h], dim=1)
    upd = torch.sigmoid(F.conv2d(comb, p[pre + "update_gate.weight"], p[pre + "update_gate.bias"]))
    rst = torch.sigmoid(F.conv2d(comb, p[pre + "reset_gate.weight"], p[pre + "reset_gate.bias"]))
    out = torch.tanh(F.conv2d(torch.cat([x, h * rst], dim=1), p[pre + "out_gate.weight"], p[pre + "out_gate.bias"]))
    return h * (1 - upd) + out * upd


# --------------------------------------------------------------------------
# DPC_RNN.forward (dpc/model_3d.py:46-98)
# --------------------------------------------------------------------------
def dpc_forward(p: Params, block: torch.Tensor, network: str = "resnet18", pred_step: int = 3,
                dropout_masks: Optional[List[torch.Tensor]] = None,
                return_intermediates: bool = False):
    """Returns score [B,P,SQ,B,P,SQ].  ``dropout_masks``: None = eval mode
    (dropout off; BN still batch-stat, model_3d.py:28); else a list of
    (num_seq-pred_step)+pred_step pre-scaled masks [B,D,ls,ls] multiplied onto
    the carried hidden state after every GRU step (convrnn.py:78)."""
    B, N, C, SL, H, W = block.shape
    feat = backbone_forward(p, block.reshape(B * N, C, SL, H, W), network)
    assert tuple(feat.shape[2:]) == (derived_sizes(H, SL)[0],) + (derived_sizes(H, SL)[1],) * 2
    return dpc_head(p, feat, B, pred_step, dropout_masks, return_intermediates)


def dpc_head(p: Params, feat: torch.Tensor, B: int, pred_step: int = 3, dropout_masks: Optional[List[torch.Tensor]] = None,
             return_intermediates: bool = False):
    """the lines of DPC_RNN.forward after the backbone (dpc/model_3d.py:53-84): feat [B*N,D,T,ls,ls] (the last block's output)
    -> score [B,P,SQ,B,P,SQ]; dropout_masks as in dpc_forward"""
    N = feat.shape[0] // B
    last_duration, last_size = feat.shape[2], feat.shape[3]
    D = p["network_pred.0.weight"].shape[0]
    feat = F.avg_pool3d(feat, (last_duration, 1, 1), stride=(1, 1, 1))  # model_3d.py:53
    assert feat.shape[2] == 1 and feat.shape[3] == last_size
    feat_inf_all = feat.view(B, N, D, last_size, last_size)
    feature = F.relu(feat).view(B, N, D, last_size, last_size)
    feature_inf = feat_inf_all[:, N - pred_step:].contiguous()  # model_3d.py:58
    k = 0
    h = torch.zeros(B, D, last_size, last_size, dtype=feat.dtype)  # convrnn.py:25-27
    for t in range(N - pred_step):  # model_3d.py:62, convrnn.py:76-79
        h = convgru_cell(feature[:, t], h, p)
        if dropout_masks is not None:
            h = h * dropout_masks[k]
        k += 1
    preds = []
    for _ in range(pred_step):  # model_3d.py:66-71
        pt = F.conv2d(h, p["network_pred.0.weight"], p["network_pred.0.bias"])
        pt = F.conv2d(F.relu(pt), p["network_pred.2.weight"], p["network_pred.2.bias"])
        preds.append(pt)
        h = convgru_cell(F.relu(pt), h, p)
        if dropout_masks is not None:
            h = h * dropout_masks[k]
        k += 1
    pred = torch.stack(preds, 1)
    SQ = last_size ** 2
    pred2 = pred.permute(0, 1, 3, 4, 2).reshape(B * pred_step * SQ, D)  # model_3d.py:81
    feat2 = feature_inf.permute(0, 1, 3, 4, 2).reshape(B * pred_step * SQ, D)  # model_3d.py:82
    score = torch.matmul(pred2, feat2.t()).view(B, pred_step, SQ, B, pred_step, SQ)  # model_3d.py:83
    if return_intermediates:
        return score, {"pred": pred2, "feature_inf": feat2, "backbone": feat}
    return score


# --------------------------------------------------------------------------
# mask / target / loss / top-k (dpc/model_3d.py:86-96, dpc/main.py:178-185,213-218,
# utils/utils.py:38-55)
# --------------------------------------------------------------------------
def mask_closed_form(B: int, P: int, SQ: int) -> torch.Tensor:
    """int8 [B,P,SQ,B,P,SQ]: 1 pos (b=b',s=s',p=n); -1 temporal neg (b=b',s=s',p!=n);
    -3 spatial neg (b=b',s!=s'); 0 easy neg."""
    b = torch.arange(B)
    pp = torch.arange(P)
    s = torch.arange(SQ)
    same_b = (b.view(B, 1, 1, 1, 1, 1) == b.view(1, 1, 1, B, 1, 1))
    same_s = (s.view(1, 1, SQ, 1, 1, 1) == s.view(1, 1, 1, 1, 1, SQ))
    same_p = (pp.view(1, P, 1, 1, 1, 1) == pp.view(1, 1, 1, 1, P, 1))
    m = torch.zeros(B, P, SQ, B, P, SQ, dtype=torch.int8)
    m[(same_b & ~same_s).expand_as(m)] = -3
    m[(same_b & same_s & ~same_p).expand_as(m)] = -1
    m[(same_b & same_s & same_p).expand_as(m)] = 1
    return m


def mask_by_reference_steps(B: int, P: int, SQ: int) -> torch.Tensor:
    """Step-by-step restatement of model_3d.py:86-96 (note Q9: N==P there)."""
    N = P
    m = torch.zeros(B, P, SQ, B, N, SQ, dtype=torch.int8)
    for k in range(B):
        m[k, :, :, k, :, :] = -3
    for k in range(B):
        for s in range(SQ):
            m[k, :, s, k, :, s] = -1
    t = m.permute(0, 2, 1, 3, 5, 4).contiguous().view(B * SQ, P, B * SQ, N)
    for j in range(B * SQ):
        for q in range(P):
            t[j, q, j, N - P + q] = 1
    return t.view(B, SQ, P, B, SQ, N).permute(0, 2, 1, 3, 5, 4).contiguous()


def target_from_mask(mask: torch.Tensor) -> torch.Tensor:
    """process_output + argmax (main.py:178-185,213-215)."""
    B, P, SQ, B2, NS, _ = mask.shape
    return (mask == 1).reshape(B * P * SQ, B2 * NS * SQ).to(torch.int64).argmax(dim=1)


def loss_and_topk(score: torch.Tensor, target: Optional[torch.Tensor] = None):
    """CrossEntropyLoss(mean) + calc_topk_accuracy (main.py:217-218, utils.py:38-55)."""
    B, P, SQ = score.shape[:3]
    rows = B * P * SQ
    flat = score.reshape(rows, -1)
    if target is None:
        target = torch.arange(rows)
    loss = F.cross_entropy(flat, target)
    _, pred = flat.topk(5, 1, True, True)
    correct = pred.t().eq(target.view(1, -1))
    accs = [correct[:k].reshape(-1).float().sum() / rows for k in (1, 3, 5)]
    return loss, accs


# --------------------------------------------------------------------------
# the head with the engine's storage points, on rows m = (b, s) (DPCEngine._build_head / csrc/gru_chain.hip)
# --------------------------------------------------------------------------
class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return g.float().to(torch.bfloat16).to(g.dtype)


def ste_round_grad_bf16(x: torch.Tensor) -> torch.Tensor:
    """identity in the forward, rounds the GRADIENT to bf16 in the backward: where a bf16 kernel stores a gradient and its
    consumers read the stored value (the recurrence's gate pre-activation gradients G_all, dP1, dP2)"""
    return _RoundGrad.apply(x)


HEAD_PARAMS = tuple(f"agg.ConvGRUCell_00.{g}.{t}" for g in ("reset_gate", "update_gate", "out_gate") for t in ("weight", "bias")) + \
    tuple(f"network_pred.{i}.{t}" for i in (0, 2) for t in ("weight", "bias"))


def head_rounded(feat: torch.Tensor, params: Params, masks: Optional[torch.Tensor], P: int, rounded: bool = True,
                 num_seq: Optional[int] = None, pin: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """the head of DPC_RNN.forward (dpc/model_3d.py:53-84, backbone/convrnn.py:24-34) from the engine's saved layer4 output
    feat [B*N,T,ls,ls,D] (channels-last) to pred and feature_inf [R,D] (rows (b,p,s)), as the engine computes it: the temporal mean,
    the ReLU / inference split, the recurrence as matrix products on rows (b,s), network_pred.  masks: [n_steps,M,D] pre-scaled keep
    masks (None: no dropout); num_seq defaults to n_steps + 1 of the masks, else 8.

    rounded: the bf16 engine's storage points pass through ste_round_bf16 (feat_relu / the GRU inputs, feature_inf, the state after
    dropout, h*r, relu(W1 h + b1), pred, relu(pred) as the next input, the packed GRU / predictor weights), and the gradients the
    backward kernel stores in bf16 and reuses through ste_round_grad_bf16 (the gate pre-activation gradients, dP1, dP2).  Biases,
    gates and accumulation stay in the input's precision.  Returns pred, feat_inf, feat_relu [N,M,D], X_all, H_all (h_0 first),
    HR_all, P1_all: tensors of the graph (differentiable).

    pin: the engine's STORED values of those tensors (same names and layouts; any subset).  A pinned storage point takes the stored
    value in the forward and passes the gradient through unchanged: the backward is then differentiated at the engine's own saved
    operands, as its kernels are, and bf16 rounding flips of the forward (another accumulation order) no longer feed the backward."""
    r = ste_round_bf16 if rounded else (lambda t: t)
    rg = ste_round_grad_bf16 if rounded else (lambda t: t)
    BN, T, ls, ls2, D = feat.shape
    N = num_seq if num_seq is not None else (masks.shape[0] + 1 if masks is not None else 8)
    B, SQ = BN // N, ls * ls2
    M, n_agg = B * SQ, N - P
    pin = pin or {}

    def rs(t, name, idx=None):   # a storage point: rounded, or the engine's stored value
        if name not in pin:
            return r(t)
        v = pin[name] if idx is None else pin[name][idx]
        return t + (v.to(t.dtype).reshape(t.shape) - t).detach()

    pred_rows = lambda i: pin["pred"].reshape(B, P, SQ, D)[:, i] if "pred" in pin else None
    mean = feat.mean(1).reshape(B, N, SQ, D)                                      # model_3d.py:53
    feat_inf = rs(mean[:, N - P:], "feat_inf").reshape(B * P * SQ, D)             # model_3d.py:58, pre-ReLU
    feat_relu = r(F.relu(mean)).permute(1, 0, 2, 3).reshape(N, M, D)             # [n][(b,s)][d]
    pre = "agg.ConvGRUCell_00."
    W = {g: r(params[pre + g + "_gate.weight"].reshape(D, 2 * D)) for g in ("update", "reset", "out")}
    Bs = {g: params[pre + g + "_gate.bias"] for g in ("update", "reset", "out")}
    W1, W2 = r(params["network_pred.0.weight"].reshape(D, D)), r(params["network_pred.2.weight"].reshape(D, D))
    b1, b2 = params["network_pred.0.bias"], params["network_pred.2.bias"]

    def cell(x, h):   # convrnn.py:24-34 with kernel_size 1: the convolutions are products on rows
        c = torch.cat([x, h], 1)
        u = torch.sigmoid(rg(c @ W["update"].t() + Bs["update"]))
        rr = torch.sigmoid(rg(c @ W["reset"].t() + Bs["reset"]))
        hr = rs(h * rr, "HR_all", k)
        o = torch.tanh(rg(torch.cat([x, hr], 1) @ W["out"].t() + Bs["out"]))
        return h * (1 - u) + o * u, hr

    h = torch.zeros(M, D, dtype=feat.dtype)
    X, H, HR, P1, preds = [], [h], [], [], []
    k = 0

    def step(x, h):
        nonlocal k
        x = rs(x, "X_all", k) if "X_all" in pin else x
        hn, hr = cell(x, h)
        X.append(x)
        HR.append(hr)
        h = rs(hn * masks[k] if masks is not None else hn, "H_all", k + 1)
        k += 1
        H.append(h)
        return h

    for t in range(n_agg):                                                        # model_3d.py:62
        h = step(feat_relu[t], h)
    for i in range(P):                                                            # model_3d.py:66-71
        p1 = rs(F.relu(rg(h @ W1.t() + b1)), "P1_all", i)
        P1.append(p1)
        p2 = rg(p1 @ W2.t() + b2)
        preds.append(r(p2) if "pred" not in pin else p2 + (pred_rows(i).reshape(M, D).to(p2.dtype) - p2).detach())
        if i < P - 1:   # the state after the last prediction is never used
            h = step(r(F.relu(p2)), h)
    pred = torch.stack(preds, 0).reshape(P, B, SQ, D).permute(1, 0, 2, 3).reshape(B * P * SQ, D)
    return dict(pred=pred, feat_inf=feat_inf, feat_relu=feat_relu, X_all=torch.stack(X), H_all=torch.stack(H),
                HR_all=torch.stack(HR), P1_all=torch.stack(P1))


def _to_bf16(t: torch.Tensor) -> torch.Tensor:
    """t rounded the way an f32 kernel value is stored in bf16 (through f32: no double rounding against the engine)"""
    return t.float().to(torch.bfloat16).to(t.dtype)


def score_ce_backward_chunked(pred: torch.Tensor, finf: torch.Tensor, logits: str = "f32", round_ds: bool = True,
                              chunk: int = 1024) -> Dict[str, torch.Tensor]:
    """score = pred @ finf^T (dpc/model_3d.py:83), CrossEntropyLoss with target = arange (main.py:213-217) and its backward in closed
    form, in f64, row chunk by row chunk (the [R][R] score never exists at once: 1.9 GB of f64 at R = 15 680).  pred, finf [R,D].

    logits "bf16": the logits are rounded to bf16 before the softmax and the rank (the train step's score16); round_ds: d/dscore =
    (softmax - onehot) / R is rounded to bf16 before both products, as the bf16 engine stores (or, fused, recomputes) it.  Returns the
    loss, per-row loss terms, the per-row rank (logits STRICTLY greater than the target's: ties rank behind), the
    top-1/3/5 accuracies, d_pred = dS @ finf and d_finf = dS^T @ pred."""
    if logits not in ("f32", "bf16"):
        raise ValueError("logits must be 'f32' or 'bf16'")
    R, D = pred.shape
    p64, f64 = pred.double(), finf.double()
    terms = torch.empty(R, dtype=torch.float64)
    rank = torch.empty(R, dtype=torch.int64)
    d_pred = torch.empty(R, D, dtype=torch.float64)
    d_finf = torch.zeros(R, D, dtype=torch.float64)
    for i0 in range(0, R, chunk):
        i1 = min(i0 + chunk, R)
        rows = torch.arange(i1 - i0)
        S = p64[i0:i1] @ f64.t()
        if logits == "bf16":
            S = _to_bf16(S)
        tgt = S[rows, rows + i0]
        lse = torch.logsumexp(S, 1)
        terms[i0:i1] = lse - tgt
        rank[i0:i1] = (S > tgt[:, None]).sum(1)
        dS = torch.exp(S - lse[:, None])
        dS[rows, rows + i0] -= 1.0
        dS /= R
        if round_ds:
            dS = _to_bf16(dS)
        d_pred[i0:i1] = dS @ f64
        d_finf += dS.t() @ p64[i0:i1]
    accs = [(rank < kk).double().mean().item() for kk in (1, 3, 5)]
    return dict(loss=terms.mean(), terms=terms, rank=rank, accs=accs, d_pred=d_pred, d_finf=d_finf)


def adam_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int,
              lr: float = 1e-3, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, wd: float = 1e-5):
    """torch.optim.Adam with L2 weight decay folded into the gradient
    (main.py:80-81; torch/optim/adam.py single-tensor path). In place."""
    g = g + wd * p
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)


def unique_param_names(p: Params) -> List[str]:
    return [k for k in p if not k.startswith("agg.cell_list.0.")]


def train_step_reference(p: Params, block: torch.Tensor, network: str = "resnet18", pred_step: int = 3,
                         dropout_masks: Optional[List[torch.Tensor]] = None):
    """forward + CE + top-k + backward (main.py:198-231, without the optimizer).
    Returns loss, accs, {name: grad} (alias keys share the cell's grad)."""
    names = unique_param_names(p)
    leaves = {k: p[k].detach().clone().requires_grad_(True) for k in names}
    full = dict(leaves)
    for k in p:
        if k.startswith("agg.cell_list.0."):
            full[k] = leaves[k.replace("agg.cell_list.0.", "agg.ConvGRUCell_00.")]
    score = dpc_forward(full, block, network, pred_step, dropout_masks)
    loss, accs = loss_and_topk(score)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    return loss.detach(), [a.item() for a in accs], dict(zip(names, grads)), score.detach()


def init_params_reference_style(network: str = "resnet18", seed: int = 0,
                                widths: Sequence[int] = LAYER_WIDTH) -> Params:
    """Reference initialisation: kaiming_normal(fan_out) convs, BN 1/0
    (resnet_2d3d.py:224-230); orthogonal gain 1 / zero bias for agg and
    network_pred (model_3d.py:100-106)."""
    g = torch.Generator().manual_seed(seed)
    params: Params = {}
    for k, shp in param_shapes(network, widths).items():
        if k.startswith("agg.cell_list.0."):
            params[k] = params[k.replace("agg.cell_list.0.", "agg.ConvGRUCell_00.")]
        elif k.startswith("backbone") and len(shp) == 5:
            fan_out = shp[0] * int(np.prod(shp[2:]))
            params[k] = torch.randn(shp, generator=g) * math.sqrt(2.0 / fan_out)
        elif k.startswith("backbone"):
            params[k] = torch.ones(shp) if k.endswith("weight") else torch.zeros(shp)
        elif k.endswith("bias"):
            params[k] = torch.zeros(shp)
        else:
            w = torch.empty(shp)
            torch.nn.init.orthogonal_(w, 1, generator=g)
            params[k] = w
    return params


# --------------------------------------------------------------------------
# LC downstream classifier (eval/model_3d_lc.py:12-65, eval/test.py:244-255) -- SURVEY.md section 8 f3
# --------------------------------------------------------------------------
BN_MOMENTUM = 0.1  # torch.nn.BatchNorm default


def lc_state_dict_keys(network: str = "resnet18", num_class: int = 101, widths: Sequence[int] = LAYER_WIDTH) -> List[str]:
    """state_dict keys of the reference LC, in its order (BatchNorm buffers interleaved; backbone built with
    track_running_stats=True, model_3d_lc.py:27-29; ConvGRU alias keys, convrnn.py:55-58)"""
    keys: List[str] = []
    base = [k for k in param_shapes(network, widths, with_alias=True) if not k.startswith("network_pred.")]
    for k in base:
        keys.append(k)
        if k.startswith("backbone.") and k.endswith(".bias"):
            pre = k[: -len("bias")]
            keys += [pre + "running_mean", pre + "running_var", pre + "num_batches_tracked"]
    keys += ["final_bn.weight", "final_bn.bias", "final_bn.running_mean", "final_bn.running_var", "final_bn.num_batches_tracked",
             "final_fc.1.weight", "final_fc.1.bias"]
    return keys


def lc_shapes(network: str = "resnet18", num_class: int = 101, widths: Sequence[int] = LAYER_WIDTH) -> "Dict[str, Tuple[int, ...]]":
    base = param_shapes(network, widths, with_alias=True)
    D = widths[3]
    out: Dict[str, Tuple[int, ...]] = {}
    for k in lc_state_dict_keys(network, num_class, widths):
        if k in base:
            out[k] = base[k]
        elif k.endswith("num_batches_tracked"):
            out[k] = ()
        elif k.startswith("final_fc.1."):
            out[k] = (num_class, D) if k.endswith("weight") else (num_class,)
        elif k.startswith("final_bn."):
            out[k] = (D,)
        else:  # running_mean / running_var of a backbone BatchNorm3d: its channel count
            out[k] = base[k.rsplit(".", 1)[0] + ".weight"]
    return out


def make_lc_params_pcg(network: str = "resnet18", num_class: int = 101, widths: Sequence[int] = LAYER_WIDTH) -> Params:
    """portable recipe for every LC state_dict entry: as make_params_pcg (key i -> PCG64(3000+i)); running_mean 0.1 n,
    running_var 1 + 0.1 |n|, num_batches_tracked 0, the Linear scaled 1/sqrt(fan_in)"""
    shapes = lc_shapes(network, num_class, widths)
    params: Params = {}
    for i, (k, shp) in enumerate(shapes.items()):
        if k.startswith("agg.cell_list.0."):
            params[k] = params[k.replace("agg.cell_list.0.", "agg.ConvGRUCell_00.")]
            continue
        if k.endswith("num_batches_tracked"):
            params[k] = torch.zeros((), dtype=torch.int64)
            continue
        n = np.random.Generator(np.random.PCG64(3000 + i)).standard_normal(shp, dtype=np.float32)
        if k.endswith("running_mean"):
            v = 0.1 * n
        elif k.endswith("running_var"):
            v = 1.0 + 0.1 * np.abs(n)
        elif len(shp) >= 2:
            v = n / np.float32(math.sqrt(int(np.prod(shp[1:]))))
        elif ".bn" in k or "downsample.1" in k or k.startswith("final_bn"):
            v = (1.0 + 0.1 * n) if k.endswith("weight") else 0.1 * n
        else:
            v = 0.05 * n
        params[k] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return params


def _bn_running(x: torch.Tensor, p: Params, new: Params, pre: str, train: bool, dims, shp, eps: float = BN_EPS) -> torch.Tensor:
    """BatchNorm with track_running_stats=True (torch.nn.functional.batch_norm semantics): train = batch statistics and
    running <- (1-m) running + m batch (unbiased variance); eval = running statistics"""
    g, b = p[pre + "weight"].view(shp), p[pre + "bias"].view(shp)
    if train:
        mean = x.mean(dims, keepdim=True)
        var = x.var(dims, unbiased=False, keepdim=True)
        n = x.numel() / x.shape[1]
        with torch.no_grad():
            new[pre + "running_mean"] = (1 - BN_MOMENTUM) * p[pre + "running_mean"] + BN_MOMENTUM * mean.reshape(-1).to(torch.float32)
            new[pre + "running_var"] = (1 - BN_MOMENTUM) * p[pre + "running_var"] + BN_MOMENTUM * (var.reshape(-1) * n / max(n - 1, 1)).to(torch.float32)
            new[pre + "num_batches_tracked"] = p[pre + "num_batches_tracked"] + 1
    else:
        mean, var = p[pre + "running_mean"].view(shp).to(x.dtype), p[pre + "running_var"].view(shp).to(x.dtype)
    return (x - mean) / torch.sqrt(var + eps) * g + b


def _lc_block(x, p, new, pre, is3d, stride, final_relu, train):
    """BasicBlock2d / 3d with running-stat BatchNorm (resnet_2d3d.py:47-116, track_running_stats=True)"""
    s1, pad = ((stride,) * 3, (1, 1, 1)) if is3d else ((1, stride, stride), (0, 1, 1))
    bn = lambda t, name: _bn_running(t, p, new, pre + name + ".", train, (0, 2, 3, 4), (1, -1, 1, 1, 1))
    out = F.relu(bn(F.conv3d(x, p[pre + "conv1.weight"], None, s1, pad), "bn1"))
    out = bn(F.conv3d(out, p[pre + "conv2.weight"], None, 1, pad), "bn2")
    if (pre + "downsample.0.weight") in p:
        res = bn(F.conv3d(x, p[pre + "downsample.0.weight"], None, s1, 0), "downsample.1")
    else:
        res = x
    out = out + res
    return F.relu(out) if final_relu else out


def lc_forward(p: Params, block: torch.Tensor, network: str = "resnet18", train: bool = False,
               gru_masks: Optional[List[torch.Tensor]] = None, fc_mask: Optional[torch.Tensor] = None):
    """LC.forward (model_3d_lc.py:47-65).  Returns output [B,1,num_class], context [B,1,D] and the dict of updated buffers
    (train mode).  gru_masks: pre-scaled masks [B,D,ls,ls] per ConvGRU step (None = no dropout); fc_mask [B,D] likewise."""
    B, N, Cc, SL, H, W = block.shape
    last_duration, last_size = derived_sizes(H, SL)
    D = p["final_bn.weight"].shape[0]
    new: Params = {}
    plan = LAYER_PLAN[network]
    x = block.reshape(B * N, Cc, SL, H, W)
    x = F.conv3d(x, p["backbone.conv1.weight"], None, (1, 2, 2), (0, 3, 3))
    x = F.relu(_bn_running(x, p, new, "backbone.bn1.", train, (0, 2, 3, 4), (1, -1, 1, 1, 1)))
    x = F.max_pool3d(x, (1, 3, 3), (1, 2, 2), (0, 1, 1))
    for li in range(4):
        for bi in range(plan[li]):
            stride = 2 if (li > 0 and bi == 0) else 1
            last = li == 3 and bi == plan[li] - 1
            x = _lc_block(x, p, new, f"backbone.layer{li + 1}.{bi}.", li >= 2, stride, not last, train)
    feature = F.avg_pool3d(F.relu(x), (last_duration, 1, 1), stride=1)  # model_3d_lc.py:52-54: ReLU first
    feature = feature.view(B, N, D, last_size, last_size)
    h = torch.zeros(B, D, last_size, last_size, dtype=block.dtype)
    for t in range(N):  # convrnn.py:76-79
        h = convgru_cell(feature[:, t], h, p)
        if gru_masks is not None:
            h = h * gru_masks[t]
    context = h.mean(dim=(2, 3))  # model_3d_lc.py:58-60: avg_pool3d over the spatial extent of the LAST state
    context = _bn_running(context.unsqueeze(-1), p, new, "final_bn.", train, (0, 2), (1, -1, 1)).squeeze(-1)  # BatchNorm1d on [B,C,1]
    y = context * fc_mask if fc_mask is not None else context
    output = y @ p["final_fc.1.weight"].t() + p["final_fc.1.bias"]
    return output.view(B, 1, -1), context.view(B, 1, D), new


def lc_loss_acc(output: torch.Tensor, target: torch.Tensor):
    """eval/test.py:244-255: CrossEntropyLoss on [B*N', C] logits with the clip label repeated, top-1 accuracy"""
    B, Np, Cn = output.shape
    flat = output.reshape(B * Np, Cn)
    tgt = target.view(B, 1).repeat(1, Np).view(-1)
    loss = F.cross_entropy(flat, tgt)
    acc = (flat.argmax(1) == tgt).float().mean()
    return loss, acc


def lc_train_step_reference(p: Params, block: torch.Tensor, target: torch.Tensor, network: str = "resnet18",
                            gru_masks=None, fc_mask=None):
    """train-mode forward + loss + backward; returns loss, acc, {name: grad}, output, context, updated buffers"""
    names = [k for k in p if not k.startswith("agg.cell_list.0.") and p[k].dtype.is_floating_point and
             not k.endswith(("running_mean", "running_var"))]
    leaves = {k: p[k].detach().clone().requires_grad_(True) for k in names}
    full = dict(p)
    full.update(leaves)
    for k in p:
        if k.startswith("agg.cell_list.0."):
            full[k] = leaves[k.replace("agg.cell_list.0.", "agg.ConvGRUCell_00.")]
    output, context, new = lc_forward(full, block, network, True, gru_masks, fc_mask)
    loss, acc = lc_loss_acc(output, target)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    return loss.detach(), acc.item(), dict(zip(names, grads)), output.detach(), context.detach(), new
