"""torch autograd through dpc_amd.lc.LC and the reference's training lines (eval/test.py:229-255) over it, shared by the CPU tier
(host SIMT simulator, width-reduced net: tests/test_lc_autograd_emu.py) and the GPU tier (tests/test_lc_groups_gpu.py)."""
from dataclasses import dataclass
from typing import Any, Sequence

import torch

from dpc_amd.lc import LC
from dpc_amd.optim import Adam
from oracle import dpc_oracle as O

EXTRACTOR = ("backbone.", "agg.")


@dataclass
class Cfg:
    device: str
    simulator: Any
    widths: Sequence[int]
    num_class: int
    size: int = 64
    B: int = 2
    N: int = 8
    SL: int = 5
    dtype: torch.dtype = torch.float32


def module(cfg: Cfg, seed: int = 4, pcg: bool = False) -> LC:
    m = LC(cfg.size, cfg.N, cfg.SL, "resnet18", 0.5, cfg.num_class, compute_dtype=cfg.dtype, widths=cfg.widths, seed=seed,
           _simulator=cfg.simulator)
    if pcg:
        m.load_state_dict(O.make_lc_params_pcg("resnet18", cfg.num_class, cfg.widths))
    return m.to(cfg.device).train()


def masks(cfg: Cfg, seed: int = 3):
    """pre-scaled keep masks of both dropouts: (for LC._forced_masks, for the oracle)"""
    g = torch.Generator().manual_seed(seed)
    ls, D, B, N = cfg.size // 32, cfg.widths[3], cfg.B, cfg.N
    keep = (torch.rand(N, B, ls, ls, D, generator=g) > 0.1).float() / 0.9
    fc_keep = (torch.rand(B, D, generator=g) > 0.5).float() / 0.5
    forced = (keep.reshape(N, B * ls * ls, D).to(cfg.device), fc_keep.to(cfg.device))
    return forced, ([keep[i].permute(0, 3, 1, 2).contiguous() for i in range(N)], fc_keep)


def ref_loop_step(model, optimizer, input_seq, target, criterion):
    """eval/test.py:228-255, the lines that matter"""
    B = input_seq.size(0)
    output, _ = model(input_seq)
    [_, N, D] = output.size()
    output = output.view(B * N, D)
    target = target.repeat(1, N).view(-1)
    loss = criterion(output, target)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss


def ft_groups(model, lr):
    """eval/test.py:76-84 with the name filter corrected to the names LC's parameters have: one group per parameter"""
    params = []
    for name, param in model.named_parameters():
        if ('backbone' in name) or ('agg' in name):
            params.append({'params': param, 'lr': lr / 10})
        else:
            params.append({'params': param})
    return params


def assert_params_agree(ma, mb, what):
    for (ka, pa), (kb, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert ka == kb
        err, bound = (pa - pb).abs().max().item(), 1e-7 * max(1.0, pb.abs().max().item())
        assert err <= bound, (what, ka, err, bound)


def same_start(ma, mb):
    """the comparison is per step: the next one starts both replicas from the same parameter bits.  So a two-step test is two
    one-step comparisons; the Adam moments (and running buffers) are NOT re-synchronised -- each optimizer carries its own into the
    second step, which is what makes that step a test of the carried state"""
    with torch.no_grad():
        for pa, pb in zip(ma.parameters(), mb.parameters()):
            pb.copy_(pa)


def case_upstream_gradient(cfg: Cfg, report=print):
    """loss = (output * R).sum() + (context * S).sum() through the module against the oracle's lc_forward under torch autograd with the
    same masks: every parameter gradient within 2e-3 of its max (the bound of tests/test_lc.py:102); S must matter.

    The oracle runs in float64.  Run in float32 it is itself 3.9e-3 away from its float64 run on this loss (eight blocks per clip,
    width-reduced net; worst parameter
    backbone.layer2.0.bn1.bias; 2.3e-3 on backbone.layer1.0.bn2.weight; 6e-4 under the cross-entropy loss of tests/test_lc.py): a
    BatchNorm1d over TWO clips turns the f32 noise of the context into gradient noise, and a random d output excites it more than
    the softmax's does.  The kernels on the simulator are within 7.2e-5 of the float64 oracle on every parameter, and within
    3.9e-3 of the float32 one -- that distance is the float32 oracle's own, so the float64 run is the reference and the bound stays."""
    forced, (gm_ref, fm_ref) = masks(cfg)
    m = module(cfg, pcg=True)
    m._forced_masks = forced
    p = O.make_lc_params_pcg("resnet18", cfg.num_class, cfg.widths)
    x = O.make_input_pcg(cfg.B, cfg.N, cfg.SL, cfg.size)
    g = torch.Generator().manual_seed(9)
    R, S = torch.randn(cfg.B, 1, cfg.num_class, generator=g), torch.randn(cfg.B, 1, cfg.widths[3], generator=g)
    names = [k for k, _ in m.named_parameters()]
    f64 = torch.float64
    leaves = {k: p[k].detach().clone().to(f64).requires_grad_(True) for k in names}
    full = {k: (v.to(f64) if v.dtype.is_floating_point else v) for k, v in p.items()}
    full.update(leaves)
    for k in p:
        if k.startswith("agg.cell_list.0."):
            full[k] = leaves[k.replace("agg.cell_list.0.", "agg.ConvGRUCell_00.")]
    ro, rc, _ = O.lc_forward(full, x.to(f64), "resnet18", True, [g_.to(f64) for g_ in gm_ref], fm_ref.to(f64))
    want = dict(zip(names, torch.autograd.grad((ro * R.to(f64)).sum() + (rc * S.to(f64)).sum(), [leaves[k] for k in names])))

    def run(Sx):
        out, ctx = m(x.to(cfg.device))
        assert out.requires_grad and ctx.requires_grad and tuple(out.shape) == (cfg.B, 1, cfg.num_class)
        m.zero_grad()
        ((out * R.to(cfg.device)).sum() + (ctx * Sx.to(cfg.device)).sum()).backward()
        return out, ctx, {k: q.grad.detach().cpu().clone() for k, q in m.named_parameters()}

    out, ctx, got = run(S)
    assert (out.detach().cpu().double() - ro.detach()).abs().max().item() < 1e-3
    worst = ("", 0.0)
    for k in names:
        e = (got[k].double() - want[k]).abs().max().item() / max(want[k].abs().max().item(), 1e-8)
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e < 2e-3, (k, e)
    report(f"upstream gradient vs oracle autograd: worst {worst[1]:.2e} ({worst[0]})")
    out, _, got0 = run(torch.zeros_like(S))
    d = (got0["final_bn.bias"] - got["final_bn.bias"]).abs().max().item()
    assert d > 0.1 * got["final_bn.bias"].abs().max().item(), "d context does not reach the BatchNorm1d gradient"
    try:
        out.sum().backward()
        raise AssertionError("a second backward must be refused")
    except RuntimeError:
        pass
    # one backward per forward, none after a later forward; only `context` used: d output arrives as None
    o1, _ = m(x.to(cfg.device))
    o2, c2 = m(x.to(cfg.device))
    try:
        o1.sum().backward()
        raise AssertionError("backward after a later forward must be refused")
    except RuntimeError as e:
        assert "later forward" in str(e)
    m.zero_grad()
    c2.sum().backward()
    assert getattr(m.final_fc, "1").weight.grad.abs().max().item() == 0 and torch.isfinite(m.backbone.conv1.weight.grad).all()
    m.eval()
    out, ctx = m(x.to(cfg.device))
    assert not out.requires_grad and not ctx.requires_grad   # eval mode: no graph


def case_reference_loop_grouped(cfg: Cfg, report=print):
    """two LC modules with the same seed run two steps of the reference's loop, one under dpc_amd.optim.Adam, one under
    torch.optim.Adam, both with one group per parameter (extractor at lr / 10) and a LambdaLR on top"""
    forced, _ = masks(cfg)
    x = O.make_input_pcg(cfg.B, cfg.N, cfg.SL, cfg.size).to(cfg.device)
    target = torch.tensor([[3], [7]], device=cfg.device)
    crit = torch.nn.CrossEntropyLoss()
    lr = 1e-3

    def make(opt_cls):
        m = module(cfg)
        m._forced_masks = forced
        o = opt_cls(ft_groups(m, lr), lr=lr, weight_decay=1e-3)
        return m, o, torch.optim.lr_scheduler.LambdaLR(o, lr_lambda=lambda ep: 0.1 ** ep)

    (ma, oa, sa), (mb, ob, sb) = make(Adam), make(torch.optim.Adam)
    assert len(oa.param_groups) == len(list(ma.parameters())) > 1
    # ---- .grad are arena views; a second backward without zero_grad accumulates
    out, _ = ma(x)
    loss = crit(out.view(cfg.B, -1), target.view(-1))
    oa.zero_grad()
    loss.backward()
    eng = ma.engine
    p0 = eng.flat_p.clone()
    assert all(q.grad.data_ptr() == eng.G[k].data_ptr() for k, q in ma.named_parameters())
    g1 = {k: q.grad.clone() for k, q in ma.named_parameters()}
    out, _ = ma(x)
    crit(out.view(cfg.B, -1), target.view(-1)).backward()   # same input, parameters and masks: exactly twice the gradient
    for k, q in ma.named_parameters():
        assert torch.equal(q.grad, 2 * g1[k]), k
        assert q.grad.data_ptr() == eng.G[k].data_ptr()
        q.grad.mul_(0.5)
    oa.step()                                               # step 1 of ma: the loop's lines, the backward run twice
    ref_loop_step(mb, ob, x, target, crit)
    assert_params_agree(ma, mb, "step 1")
    assert eng.step_count == 1 and eng.seg_uploads == 1
    d1 = (eng.flat_p - p0).abs().mean().item()
    sa.step()
    sb.step()
    same_start(ma, mb)
    p1 = eng.flat_p.clone()
    ref_loop_step(ma, oa, x, target, crit)
    ref_loop_step(mb, ob, x, target, crit)
    assert_params_agree(ma, mb, "step 2")
    d2 = (eng.flat_p - p1).abs().mean().item()
    report(f"mean |dp|: step 1 {d1:.3g}, step 2 after LambdaLR x0.1 {d2:.3g}")
    assert eng.seg_uploads == 2 and d2 < 0.5 * d1      # the schedule reached the kernel's table: one upload per change, smaller steps
    eng.set_param_groups(eng.param_groups)
    assert eng.seg_uploads == 2                         # same values again: nothing is uploaded
    # the extractor really runs at a tenth: the table says so
    tab = {g["params"][0]: g["lr"] for g in eng.param_groups}
    assert abs(tab["backbone.conv1.weight"] - lr / 100) < 1e-12 and abs(tab["final_fc.1.weight"] - lr / 10) < 1e-12


def case_frozen(cfg: Cfg, how: str, report=print, poison: bool = True):
    """requires_grad_(False) on backbone.* and agg.*: a linear probe on a frozen extractor.  how = 'all_parameters': the optimizer
    is given model.parameters() (the frozen ones never get a gradient); 'filter_requires_grad': Adam(filter(requires_grad, ...))"""
    forced, _ = masks(cfg)
    x = O.make_input_pcg(cfg.B, cfg.N, cfg.SL, cfg.size).to(cfg.device)
    target = torch.tensor([[3], [7]], device=cfg.device)
    crit = torch.nn.CrossEntropyLoss()

    def params_of(m):
        return list(m.parameters()) if how == "all_parameters" else list(filter(lambda q: q.requires_grad, m.parameters()))

    def make(opt_cls):
        m = module(cfg)
        m._forced_masks = forced
        for k, q in m.named_parameters():
            if k.startswith(EXTRACTOR):
                q.requires_grad_(False)
        return m, opt_cls(params_of(m), lr=1e-3, weight_decay=1e-3)

    (ma, oa), (mb, ob) = make(Adam), make(torch.optim.Adam)
    # first forward by hand: the engine exists, its extractor gradients are poisoned; the truncated backward must not touch them
    out, _ = ma(x)
    eng = ma.engine
    frozen = torch.zeros(eng.numel, dtype=torch.bool, device=eng.flat_p.device)
    for k, (o, n) in eng.offsets.items():
        if k.startswith(EXTRACTOR):
            frozen[o:o + n] = True
    init = [t.clone() for t in (eng.flat_p, eng.flat_m, eng.flat_v)]
    eng.flat_g[frozen] = float("nan")
    loss = crit(out.view(cfg.B, -1), target.view(-1))
    oa.zero_grad()
    loss.backward()
    assert torch.isnan(eng.flat_g[frozen]).all(), "the truncated backward wrote extractor gradients"
    assert torch.isfinite(eng.flat_g[~frozen]).all()
    assert all((q.grad is None) == k.startswith(EXTRACTOR) for k, q in ma.named_parameters())
    assert eng.grad_wanted([k for k, q in ma.named_parameters() if q.requires_grad]) == (False, False)
    oa.step()
    ref_loop_step(mb, ob, x, target, crit)
    assert_params_agree(ma, mb, "step 1")
    same_start(ma, mb)
    ref_loop_step(ma, oa, x, target, crit)
    ref_loop_step(mb, ob, x, target, crit)
    assert_params_agree(ma, mb, "step 2")
    bits = lambda t: t.view(torch.int32)   # noqa: E731
    for now, was in zip((eng.flat_p, eng.flat_m, eng.flat_v), init):
        assert torch.equal(bits(now)[frozen], bits(was)[frozen])
    assert not torch.equal(eng.flat_p[~frozen], init[0][~frozen])
    assert torch.isnan(eng.flat_g[frozen]).all()
    assert int(ma.backbone.bn1.num_batches_tracked) == 2 and int(ma.final_bn.num_batches_tracked) == 2   # train mode: batch statistics, buffers move
    assert not torch.equal(ma.backbone.bn1.running_mean.cpu(), torch.zeros_like(ma.backbone.bn1.running_mean.cpu()))
    # ---- state_dict: torch's layout, state only for what was updated; loads into torch's Adam and a fresh fused one; the next step agrees
    sd = oa.state_dict()
    n_head = sum(1 for k, _ in ma.named_parameters() if not k.startswith(EXTRACTOR))
    assert len(sd["param_groups"]) == 1 and len(sd["param_groups"][0]["params"]) == len(params_of(ma))
    assert len(sd["state"]) == n_head and all(float(s["step"]) == 2.0 for s in sd["state"].values())
    ob2 = torch.optim.Adam(params_of(mb), lr=5e-4, weight_decay=0.0)
    ob2.load_state_dict(sd)
    oa2 = Adam(params_of(ma), lr=5e-4, weight_decay=0.0)
    m_before = eng.flat_m.clone()
    eng.flat_m.zero_()
    oa2.load_state_dict(sd)
    assert torch.equal(eng.flat_m[~frozen], m_before[~frozen]) and oa2.param_groups[0]["lr"] == 1e-3
    same_start(ma, mb)
    ref_loop_step(ma, oa2, x, target, crit)
    ref_loop_step(mb, ob2, x, target, crit)
    assert_params_agree(ma, mb, "step 3, after load_state_dict")
    assert eng.step_count == 3
    with torch.no_grad():   # differing step counts stay refused
        bad = {"state": {i: dict(s) for i, s in sd["state"].items()}, "param_groups": sd["param_groups"]}
        first = next(iter(bad["state"]))
        bad["state"][first]["step"] = torch.tensor(7.0)
        try:
            oa2.load_state_dict(bad)
            raise AssertionError("differing per-parameter step counts must be refused")
        except ValueError:
            pass


def case_set_param_groups(cfg: Cfg):
    """the table: merged neighbours, alternating patterns, validation, uploads only on change, and the one-group path untouched"""
    from dpc_amd import _lib as L
    from dpc_amd.lc import LCEngine
    eng = LCEngine("resnet18", cfg.size, cfg.N, cfg.SL, cfg.B, cfg.device, cfg.dtype, cfg.widths, lib=cfg.simulator, num_class=cfg.num_class)
    names = list(eng.offsets)

    def segments():
        return list((L.AdamSegment * eng._seg_n).from_buffer_copy(eng._seg_host))

    head = [k for k in names if not k.startswith(EXTRACTOR)]
    eng.set_param_groups([{"params": head, "lr": 1e-3, "weight_decay": 0.0}])
    s = segments()
    assert len(s) == 2 and (s[0].active, s[1].active) == (0, 1) and s[0].begin == 0 and s[0].end == s[1].begin == eng.offsets[head[0]][0]
    assert s[1].end == eng.numel and eng.frozen_params() == [k for k in names if k.startswith(EXTRACTOR)] and eng.seg_uploads == 1
    eng.set_param_groups([{"params": head, "lr": 1e-3, "weight_decay": 0.0}])
    assert eng.seg_uploads == 1
    eng.set_param_groups([{"params": head, "lr": 5e-4, "weight_decay": 0.0}])
    assert eng.seg_uploads == 2
    eng.set_param_groups([{"params": names[0::2], "lr": 1e-3, "weight_decay": 0.0}, {"params": names[1::2], "lr": 1e-4, "weight_decay": 0.0}])
    s = segments()
    assert len(s) == len(names) and all(a.end == b.begin for a, b in zip(s, s[1:])) and all(x.begin % 4 == 0 and x.end % 4 == 0 for x in s)
    for bad in ([{"params": ["no.such"], "lr": 1e-3}], [{"params": names[:1], "lr": 1e-3}, {"params": names[:1], "lr": 1e-3}],
                [{"params": names[:1], "lr": -1.0}], [{"params": names[:1], "lr": float("nan")}]):
        try:
            eng.set_param_groups(bad)
            raise AssertionError(f"{bad} must be refused")
        except (KeyError, ValueError):
            pass
    eng.set_param_groups(None)
    assert eng.param_groups is None and eng.frozen_params() == []


def case_autograd_decides_the_truncation(cfg: Cfg):
    """Where the backward stops is decided by what autograd asks for, never by which parameters the optimizer holds.
    (1) The extractor keeps requires_grad = True while the optimizer holds the head only: after a step (which freezes the extractor
    in the engine's segment table) its gradients are still those of a full backward.  (2) requires_grad_(False) for one step under
    Adam(model.parameters()), then requires_grad_(True): the very next backward is complete again and the step updates everything."""
    forced, _ = masks(cfg)
    x = O.make_input_pcg(cfg.B, cfg.N, cfg.SL, cfg.size).to(cfg.device)
    target = torch.tensor([[3], [7]], device=cfg.device)
    crit = torch.nn.CrossEntropyLoss()

    def fresh():
        m = module(cfg)
        m._forced_masks = forced
        return m

    def grads_of(m):
        out, _ = m(x)
        m.zero_grad()
        crit(out.view(cfg.B, -1), target.view(-1)).backward()
        return {k: (None if q.grad is None else q.grad.detach().clone()) for k, q in m.named_parameters()}

    ref = fresh()   # the full backward, under no optimizer
    # ---- (1)
    ma = fresh()
    oa = Adam([q for k, q in ma.named_parameters() if not k.startswith(EXTRACTOR)], lr=1e-3, weight_decay=1e-3)
    ref_loop_step(ma, oa, x, target, crit)
    assert ma.engine.frozen_params() and ma.engine.grad_wanted() == (False, False)   # the optimizer's table froze the extractor ...
    same_start(ma, ref)
    ga, gr = grads_of(ma), grads_of(ref)
    for k in gr:                                                                     # ... and the gradients do not care
        assert ga[k] is not None and torch.equal(ga[k], gr[k]), k
    assert ga["backbone.conv1.weight"].abs().max().item() > 0
    # ---- (2)
    mc = fresh()
    oc = Adam(mc.parameters(), lr=1e-3, weight_decay=1e-3)
    for k, q in mc.named_parameters():
        if k.startswith(EXTRACTOR):
            q.requires_grad_(False)
    ref_loop_step(mc, oc, x, target, crit)
    assert all((q.grad is None) == k.startswith(EXTRACTOR) for k, q in mc.named_parameters())
    for q in mc.parameters():
        q.requires_grad_(True)
    same_start(mc, ref)
    gc, gr = grads_of(mc), grads_of(ref)
    for k in gr:
        assert gc[k] is not None and torch.equal(gc[k], gr[k]), k
    before = {k: q.detach().clone() for k, q in mc.named_parameters()}
    oc.step()
    assert mc.engine.param_groups is None and mc.engine.step_count == 2              # one group over everything again
    assert all(not torch.equal(q, before[k]) and torch.isfinite(q).all() for k, q in mc.named_parameters())
