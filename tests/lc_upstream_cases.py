"""dpc_lc_head_bwd from an upstream gradient (torch autograd through LC.forward): a random d loss / d output in the `dlogits`
buffer and a random d loss / d context in the descriptor's d_bn_out, fixed keep mask, against f64 torch autograd on the same
inputs.  Built as kcases.case_lc_head is (same inputs, descriptor and bound rule: 8 x the error of the f32 torch chain against the
f64 one, floor 1e-6, never above tol(f32)).  Shared by the CPU and the GPU tier."""
import ctypes as C

import torch
import torch.nn.functional as F

import kcases as kc

QUANTITIES = ("d_hlast", "g_bn_weight", "g_bn_bias", "g_fc_weight", "g_fc_bias")


def _chain(inp, dt, R, S):
    """spatial mean -> BatchNorm1d (train) -> keep mask -> Linear in `dt`; loss = (logits * R).sum() + (bn * S).sum()"""
    B, SQ, D = inp["B"], inp["SQ"], inp["D"]
    h = inp["h"].to(dt).requires_grad_()
    gam, bet, W, bias = (inp[n].to(dt).requires_grad_() for n in ("gamma", "beta", "W", "bias"))
    ctx = h.view(B, SQ, D).mean(1)
    bn = F.batch_norm(ctx, None, None, gam, bet, True, kc.LC_MOMENTUM, kc.LC_EPS)
    logits = F.linear(bn * inp["keep"].to(dt), W, bias)
    ((logits * R.to(dt)).sum() + (bn * S.to(dt)).sum()).backward()
    out = dict(d_hlast=h.grad, g_bn_weight=gam.grad, g_bn_bias=bet.grad, g_fc_weight=W.grad, g_fc_bias=bias.grad)
    return {n: v.detach().double() for n, v in out.items()}


def case_lc_head_upstream(k: kc.K, dtype, B, SQ, D, NC, report=print):
    inp = kc._lc_head_inputs(dtype, B, SQ, D, NC, "centred", 51)
    g = torch.Generator().manual_seed(77)
    R, S = torch.randn(B, NC, generator=g), torch.randn(B, D, generator=g)
    want, f32 = _chain(inp, torch.float64, R, S), _chain(inp, torch.float32, R, S)
    bound = {n: max(8.0 * kc.relerr(f32[n], want[n]), 1e-6) for n in QUANTITIES}
    assert max(bound.values()) <= kc.tol(torch.float32)
    d, t = kc._lc_head_desc(k, dtype, inp, 0.5, keep=inp["keep"])
    k.call("dpc_lc_head_fwd", C.byref(d))
    # (1) a null d_bn_out: the bits of the call as it was (CE gradient left by the forward)
    k.call("dpc_lc_head_bwd", C.byref(d))
    k.sync()
    ce = {n: t[n].cpu().clone() for n in QUANTITIES + ("dctx",)}
    zero = k.zeros(B, D)   # real input: an upstream gradient of +0
    d.d_bn_out = zero.data_ptr()
    k.call("dpc_lc_head_bwd", C.byref(d))
    k.sync()
    for n in ce:   # adding +0 changes no bit either (no NaN / -0 arithmetic in between: x + 0 == x)
        assert torch.equal(t[n].cpu(), ce[n]), n
    d.d_bn_out = None
    k.call("dpc_lc_head_bwd", C.byref(d))
    k.sync()
    for n in ce:
        assert torch.equal(t[n].cpu().view(torch.int32), ce[n].view(torch.int32)), n
    # (2) arbitrary upstream gradients
    t["dlogits"].copy_(k.t(R))
    ds = k.t(S)
    d.d_bn_out = ds.data_ptr()
    k.call("dpc_lc_head_bwd", C.byref(d))
    k.sync()
    errs = {n: kc.relerr(t[n], want[n]) for n in QUANTITIES}
    report(f"lc_head_bwd upstream {dtype}: " + ", ".join(f"{n} {errs[n]:.2e} (bound {bound[n]:.2e})" for n in QUANTITIES))
    bad = {n: (errs[n], bound[n]) for n in QUANTITIES if not errs[n] < bound[n]}
    assert not bad, f"(error, bound) {bad}"
    # d context matters: without it the BatchNorm gradients are others
    d.d_bn_out = None
    k.call("dpc_lc_head_bwd", C.byref(d))
    k.sync()
    assert kc.relerr(t["g_bn_bias"], want["g_bn_bias"]) > 0.1
    return errs
