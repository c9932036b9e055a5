"""Gradient accumulation (csrc/grad_accum.hip: dpc_grad_accumulate; BackboneEngine.set_grad_accum; --accum_steps of both entries),
shared by the CPU tier (host SIMT simulator, tests/test_accum_emu.py) and the GPU tier (tests/test_accum_gpu.py).

Bounds:
  kernel                 : bit identity to torch's f32 add and multiply on the host, in the kernel's order (one add, rounded, per
                           micro-batch from +0; the last sum times float32(1 / N), rounded); exact on integer data
  engine against a twin  : bit identity (the twin's sum and scale are the same torch f32 ops, written into its flat_g by hand)
  engine against f64 Adam: the bounds of tests/adam_groups_cases.py, the reference fed the f64 mean of the micro-gradients
"""
import math
import os
import re

import pytest
import torch

import adam_groups_cases as ac
import grad_guard_cases as gc
from dpc_amd import _lib as L
from kcases import K

TILE = ac.TILE
ADD, FINISH = L.ACCUM_ADD, L.ACCUM_FINISH
bits = gc.bits
live_mask = gc.live_mask
Cfg = gc.Cfg


def f32(x: float) -> torch.Tensor:
    return torch.tensor(x, dtype=torch.float32)


def accumulate(k: K, acc, g, n, begin, end, tab, nseg, mode, scale):
    k.call("dpc_grad_accumulate", acc, g, n, begin, end, tab, nseg, mode, float(scale))
    k.sync()


def host_cycle(gs, scale: float):
    """what a cycle leaves in g, in torch f32 on the host: ((0 + g0) + g1) + ..., then (acc + g_last) * scale"""
    acc = torch.zeros_like(gs[0])
    for g in gs[:-1]:
        acc = acc + g
    return (acc + gs[-1]) * f32(scale), acc


def split_of(segs):
    """the layout's analogue of grad_split: the first segment edge behind the long segment"""
    return segs[40][0]


def arenas_of_layout():
    """(n, segments or None, live mask) of the three arenas the kernel cases run on"""
    segs, n, sp = ac.layout()
    big = (L.GRAD_PARTIALS + 1) * TILE + 8   # one workgroup takes a second tile; the last tile is partial
    return [(n, segs, live_mask(segs, n)), (n, None, torch.ones(n, dtype=torch.bool)), (big, None, torch.ones(big, dtype=torch.bool))], segs, sp


# ------------------------------------------------------------------ K1
def case_bit_identity(k: K):
    layouts, segs, sp = arenas_of_layout()
    scale = float(f32(1.0 / 3.0))
    for li, (n, sg, act) in enumerate(layouts):
        gen = torch.Generator().manual_seed(20 + li)
        gs = [torch.randn(n, generator=gen) for _ in range(4)]
        live = act.nonzero().flatten()
        a, b, c = (int(live[i]) for i in (1, 6, 11))
        gs[1][a] = -0.0                                  # a micro-gradient of -0.0
        for g in gs:                                     # every term -0.0: +0 + -0 is +0, and (+0 + -0) * scale is +0
            g[b] = -0.0
        gs[0][c] = -1e-45                                # the sum is the smallest negative subnormal, times 1/3 rounds to -0.0
        for g in gs[1:]:
            g[c] = -0.0
        tab, nseg = (ac.table(k, sg), len(sg)) if sg is not None else (None, 0)
        acc0 = torch.zeros(n)
        if sg is not None:
            for t in gs + [acc0]:
                gc.poisoned_layout(t, segs, sp)
        acc = k.t(acc0.clone())
        want_acc = torch.zeros(n)
        for g in gs[:3]:
            gd = k.t(g.clone())
            accumulate(k, acc, gd, n, 0, n, tab, nseg, ADD, scale)
            want_acc = want_acc + g
            assert torch.equal(bits(gd.cpu()), bits(g))                                   # ADD only reads g
            assert torch.equal(bits(acc.cpu())[act], bits(want_acc)[act])
        gd = k.t(gs[3].clone())
        accumulate(k, acc, gd, n, 0, n, tab, nseg, FINISH, scale)
        want, _ = host_cycle(gs, scale)
        got, got_acc = gd.cpu(), acc.cpu()
        assert torch.equal(bits(got)[act], bits(want)[act])
        assert not bits(got_acc)[act].any()                                               # +0 on every live unit
        assert torch.equal(bits(got)[~act], bits(gs[3])[~act]) and torch.equal(bits(got_acc)[~act], bits(acc0)[~act])
        assert bits(got)[a] == bits(want)[a] and bits(got)[b] == 0
        assert bits(want)[c] == bits(f32(-0.0)) == bits(got)[c]


# ------------------------------------------------------------------ K2
def case_integer_data(k: K):
    layouts, segs, sp = arenas_of_layout()
    for li, (n, sg, act) in enumerate(layouts):
        gen = torch.Generator().manual_seed(30 + li)
        gs = [torch.randint(-3, 4, (n,), generator=gen).float() for _ in range(4)]
        tab, nseg = (ac.table(k, sg), len(sg)) if sg is not None else (None, 0)
        acc = k.t(torch.zeros(n))
        for g in gs[:3]:
            accumulate(k, acc, k.t(g), n, 0, n, tab, nseg, ADD, 0.25)
        gd = k.t(gs[3].clone())
        accumulate(k, acc, gd, n, 0, n, tab, nseg, FINISH, 0.25)
        exact = (gs[0].double() + gs[1].double() + gs[2].double() + gs[3].double()) / 4
        assert torch.equal(gd.cpu().double()[act], exact[act])
        assert not bits(acc.cpu())[act].any()


# ------------------------------------------------------------------ K3
def case_segment_table(k: K):
    segs, n, sp = ac.layout()
    tab, act = ac.table(k, segs), live_mask(segs, n)
    gen = torch.Generator().manual_seed(40)
    g0 = gc.poisoned_layout(torch.randn(n, generator=gen), segs, sp)
    a0 = gc.poisoned_layout(torch.randn(n, generator=gen), segs, sp)
    assert not torch.isfinite(g0[~act]).any() and not torch.isfinite(a0[~act]).any()
    for mode in (ADD, FINISH):
        gd, acc = k.t(g0.clone()), k.t(a0.clone())
        accumulate(k, acc, gd, n, 0, n, tab, len(segs), mode, 0.5)
        g, a = gd.cpu(), acc.cpu()
        assert torch.equal(bits(g)[~act], bits(g0)[~act]) and torch.equal(bits(a)[~act], bits(a0)[~act])   # never loaded, never stored
        assert torch.isfinite(g[act]).all() and torch.isfinite(a[act]).all()
        if mode == ADD:
            assert torch.equal(bits(a)[act], bits(a0 + g0)[act]) and torch.equal(bits(g), bits(g0))
        else:
            assert torch.equal(bits(g)[act], bits((a0 + g0) * f32(0.5))[act]) and not bits(a)[act].any()


# ------------------------------------------------------------------ K4
def case_range(k: K):
    segs, n, sp = ac.layout()
    tab, act = ac.table(k, segs), live_mask(segs, n)
    gen = torch.Generator().manual_seed(50)
    g0 = gc.poisoned_layout(torch.randn(n, generator=gen), segs, sp)
    a0 = gc.poisoned_layout(torch.randn(n, generator=gen), segs, sp)
    scale = float(f32(1.0 / 3.0))
    edges = sorted({e for s in segs for e in s[:2]})
    assert TILE in range(n) and all(e % 4 == 0 for e in edges)
    pairs = [(8, 4000), (TILE - 4, TILE + 8), (0, TILE), (TILE, n), (TILE, TILE + 400), (n - 4, n), (0, n)]   # inside a tile, across and at tile edges
    pairs += [(e, min(e + 12, n)) for e in edges] + [(max(e - 12, 0), e) for e in edges]                  # every segment edge, as begin and as end
    for lay_tab, nseg, live in ((tab, len(segs), act), (None, 0, torch.isfinite(g0))):
        for mode in (ADD, FINISH):
            for b, e in (pairs if lay_tab is not None else pairs[:7]):
                gd, acc = k.t(g0.clone()), k.t(a0.clone())
                accumulate(k, acc, gd, n, b, e, lay_tab, nseg, mode, scale)
                g, a = gd.cpu(), acc.cpu()
                inside = torch.zeros(n, dtype=torch.bool)
                inside[b:e] = True
                if lay_tab is None:   # (without a table the poisoned units inside the range are live too: judged over the finite ones)
                    hit = inside & live
                else:
                    hit = inside & act
                    assert torch.equal(bits(g)[~hit], bits(g0)[~hit]) and torch.equal(bits(a)[~hit], bits(a0)[~hit]), (mode, b, e)
                assert torch.equal(bits(g)[~inside], bits(g0)[~inside]) and torch.equal(bits(a)[~inside], bits(a0)[~inside]), (mode, b, e)
                if mode == ADD:
                    assert torch.equal(bits(a)[hit], bits(a0 + g0)[hit]) and torch.equal(bits(g), bits(g0)), (b, e)
                else:
                    assert torch.equal(bits(g)[hit], bits((a0 + g0) * f32(scale))[hit]) and not bits(a)[hit].any(), (b, e)
    # FINISH over [0, s) and then [s, n) is FINISH over [0, n), at the layout's grad_split and at every other edge
    gd, acc = k.t(g0.clone()), k.t(a0.clone())
    accumulate(k, acc, gd, n, 0, n, tab, len(segs), FINISH, scale)
    whole_g, whole_a = gd.cpu(), acc.cpu()
    for s in [split_of(segs)] + edges:
        gd, acc = k.t(g0.clone()), k.t(a0.clone())
        accumulate(k, acc, gd, n, 0, s, tab, len(segs), FINISH, scale)
        accumulate(k, acc, gd, n, s, n, tab, len(segs), FINISH, scale)
        assert torch.equal(bits(gd.cpu()), bits(whole_g)) and torch.equal(bits(acc.cpu()), bits(whole_a)), s
    # begin == end: a successful no-op
    gd, acc = k.t(g0.clone()), k.t(a0.clone())
    accumulate(k, acc, gd, n, 64, 64, tab, len(segs), FINISH, scale)
    assert torch.equal(bits(gd.cpu()), bits(g0)) and torch.equal(bits(acc.cpu()), bits(a0))


# ------------------------------------------------------------------ K5
def case_refused_calls(k: K):
    segs, n, _ = ac.layout()
    tab, S = ac.table(k, segs), len(segs)
    gen = torch.Generator().manual_seed(60)
    g0, a0 = torch.randn(n + 4, generator=gen), torch.randn(n + 4, generator=gen)
    g, a = k.t(g0.clone()), k.t(a0.clone())
    call = lambda *args: k.call("dpc_grad_accumulate", *args)   # noqa: E731
    bad = [
        lambda: call(None, g, n, 0, n, tab, S, ADD, 1.0),
        lambda: call(a, None, n, 0, n, tab, S, ADD, 1.0),
        lambda: call(g, g, n, 0, n, tab, S, ADD, 1.0),
        lambda: call(a, g, 0, 0, 0, tab, S, ADD, 1.0),
        lambda: call(a, g, -4, 0, 0, tab, S, ADD, 1.0),
        lambda: call(a, g, n + 2, 0, n, tab, S, ADD, 1.0),
        lambda: call(a[1:], g, n, 0, n, tab, S, ADD, 1.0),
        lambda: call(a, g[1:], n, 0, n, tab, S, FINISH, 1.0),
        lambda: call(a, g, n, 2, n, tab, S, ADD, 1.0),
        lambda: call(a, g, n, 0, n - 2, tab, S, FINISH, 1.0),
        lambda: call(a, g, n, 8, 4, tab, S, ADD, 1.0),
        lambda: call(a, g, n, 0, n + 4, tab, S, FINISH, 1.0),
        lambda: call(a, g, n, -4, n, tab, S, ADD, 1.0),
        lambda: call(a, g, n, 0, n, tab, S, 2, 1.0),
        lambda: call(a, g, n, 0, n, tab, S, -1, 1.0),
        lambda: call(a, g, n, 0, n, tab, S, FINISH, float("nan")),
        lambda: call(a, g, n, 0, n, tab, S, FINISH, float("inf")),
        lambda: call(a, g, n, 0, n, tab, S, ADD, float("-inf")),
        lambda: call(a, g, n, 0, n, tab, 0, ADD, 1.0),
        lambda: call(a, g, n, 0, n, tab, L.ADAM_MAX_SEGMENTS + 1, FINISH, 1.0),
    ]
    for f in bad:
        with pytest.raises(L.DpcError, match=f"code {L.ERR_ARG}$"):
            f()
    k.sync()
    assert torch.equal(bits(g.cpu()), bits(g0)) and torch.equal(bits(a.cpu()), bits(a0))


# ====================================================================== engine
def micro_inputs(cfg: Cfg, count: int):
    """`count` different micro-batches: N(0, 1) videos, one seed each"""
    shape = gc.dpc_input(cfg).shape
    return [torch.randn(shape, generator=torch.Generator().manual_seed(100 + j)).to(cfg.device) for j in range(count)]


def all_arenas(eng):
    out = [eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v, eng.dev_step, eng.dev_bc, eng.dev_draw]
    if eng.flat_ema is not None:
        out.append(eng.flat_ema)
    return [t.detach().clone() for t in out]


same_bits = gc.same_bits


def acc_is_zero(eng, mask=None):
    a = bits(eng.flat_acc.detach().cpu())
    return not (a if mask is None else a[mask]).any()


def case_off_is_the_engine_as_it_was(cfg: Cfg, dtype=torch.float32):   # E1
    a, b = gc.dpc_engine(cfg, dtype), gc.dpc_engine(cfg, dtype)
    b.set_grad_accum(1)
    assert b.flat_acc is None and b.accum_steps == 1 and b.accum_pending == 0 and a._baked_scalars() == b._baked_scalars()
    la, lb = a._launches, b._launches
    for x in micro_inputs(cfg, 2):
        a.train_step(x)
        b.train_step(x)
    assert same_bits(all_arenas(a), all_arenas(b)) and a._launches - la == b._launches - lb
    assert b.flat_acc is None and a.step_count == b.step_count == 2
    with pytest.raises(ValueError):
        b.set_grad_accum(0)


def by_hand_cycle(twin, xs, scale):
    """forward and backward per micro-batch, flat_g cloned each time; the host forms the sum and the scale with torch f32 in the
    kernel's order and writes them into flat_g; adam_step().  Returns the micro-batches' results and gradients"""
    gs, res = [], []
    for x in xs:
        twin._forward_loss(x, True)
        twin.backward()
        gs.append(twin.flat_g.detach().cpu().clone())
        res.append(twin.result.detach().clone())
    mean, _ = host_cycle(gs, scale)
    twin.flat_g.copy_(mean.to(twin.flat_g.device))
    twin.adam_step()
    return res, gs


def case_against_a_by_hand_twin(cfg: Cfg, dtype=torch.float32):   # E2
    N = 3
    eng, twin = gc.dpc_engine(cfg, dtype), gc.dpc_engine(cfg, dtype)
    eng.set_grad_accum(N)
    assert eng.accum_steps == N and acc_is_zero(eng) and ("accum", N) in eng._baked_scalars()
    xs = micro_inputs(cfg, 2 * N)
    scale = float(f32(1.0 / N))
    steps_before = twin._step_count
    for c in range(2):
        got = []
        for j, x in enumerate(xs[c * N:(c + 1) * N]):
            assert eng.accum_pending == j
            if j:
                with pytest.raises(RuntimeError):
                    eng.set_grad_accum(2)          # refused while a cycle is open
            got.append(eng.train_step(x).clone())
            assert int(eng.dev_step.item()) == c + (j == N - 1)
        want, _ = by_hand_cycle(twin, xs[c * N:(c + 1) * N], scale)
        assert eng.accum_pending == 0 and acc_is_zero(eng)
        assert all(torch.equal(bits(r), bits(w)) for r, w in zip(got, want))
        assert same_bits(all_arenas(eng), all_arenas(twin)), c
    assert twin._step_count - steps_before == 2 == eng.step_count and int(eng.dev_draw.item()) == 2 * N
    assert not torch.equal(got[0], got[1])


def case_against_f64_adam(cfg: Cfg, report=print, check_rejection=False):   # E3
    """the second cycle (the moments of the first are in place: a first Adam step moves every parameter by lr * sign(g), whatever g's
    size) against adam_groups_cases.adam_f64 fed the f64 mean of the micro-gradients, at that module's bounds.

    N = 2: the bounds of adam_groups_cases are relative to |g| of an f32 gradient taken as exact.  With two micro-batches the
    accumulated gradient is fl(g0 + g1) * 0.5 -- the first add into +0 and the halving are exact --, ONE rounding of the f64 mean, so
    those bounds apply with one more rounding on their (1 - beta) |g| term, inside their count of eight.  From N = 3 on the partial
    sums are rounded at their own size, which chance cancellation makes many times |mean g| on some elements: measured on the
    simulator at N = 3 with these inputs, p 2.98e-08 (bound 1.28e-07), but m 4.08 and v 6.9 times their bounds, at such elements.
    That is the f32 sum the kernel is specified to form (bit-identical to torch's: case_against_a_by_hand_twin), not an error of
    the step."""
    N = 2
    eng, probe = gc.dpc_engine(cfg), gc.dpc_engine(cfg)
    eng.set_grad_accum(N)
    xs = micro_inputs(cfg, 2 * N)
    for x in xs[:N]:
        eng.train_step(x)
    probe.flat_p.copy_(eng.flat_p)
    probe.dev_draw.copy_(eng.dev_draw)
    p1, m1, v1 = (t.detach().cpu().clone() for t in (eng.flat_p, eng.flat_m, eng.flat_v))
    gs = []
    for x in xs[N:]:   # the micro-gradients of the second cycle, from an engine with the same parameters and the same draws
        probe._forward_loss(x, True)
        probe.backward()
        gs.append(probe.flat_g.detach().cpu().double())
        eng.train_step(x)
    n = eng.numel
    real = torch.zeros(n, dtype=torch.bool)   # the parameters' own floats (not the padding of their 16-byte slots)
    for o, cnt in eng.offsets.values():
        real[o:o + cnt] = True
    lr, wd, bc = torch.full((n,), eng.lr), torch.full((n,), eng.wd), eng.dev_bc.cpu()
    bp = 1e-7 * max(1.0, p1.abs().max().item())
    p, m, v = (t.detach().cpu().double() for t in (eng.flat_p, eng.flat_m, eng.flat_v))

    def misses(g64):
        p2, m2, v2, bm, bv = ac.adam_f64(p1, g64, m1, v1, lr, wd, bc, 1.0)
        ep = (p - p2.float().double()).abs()
        em = (m - m2.float().double()).abs() / bm.clamp_min(1e-300)
        ev = (v - v2.float().double()).abs() / bv.clamp_min(1e-300)
        return ep, em, ev

    ep, em, ev = misses(sum(gs) / N)
    report(f"accumulated step vs f64 Adam on the f64 mean: p {ep[real].max().item():.3g} (bound {bp:.3g}), m {em[real].max().item():.3g} of its "
           f"bound, v {ev[real].max().item():.3g} of its bound")
    assert ep[real].max().item() <= bp and em[real].max().item() <= 1.0 and ev[real].max().item() <= 1.0
    if check_rejection:   # the same reference fed only the last micro-gradient misses on more than half of the elements
        ep, em, ev = misses(gs[-1])
        frac = ((ep > bp) | (em > 1.0) | (ev > 1.0))[real].double().mean().item()
        report(f"the reference fed the last micro-gradient alone misses the bound on {frac:.3f} of the elements")
        assert frac > 0.5


def guarded(cfg: Cfg, N: int):
    from dpc_amd.optim import LRSchedule
    eng = gc.dpc_engine(cfg)
    eng.set_grad_guard(max_norm=1e30, skip_nonfinite=True)
    eng.set_ema(0.99)
    eng.set_lr_schedule(LRSchedule("cosine", 2, 10, 0.1))
    eng.set_optimizer("lamb")
    eng.set_grad_accum(N)
    return eng


def case_dropped_cycle(cfg: Cfg):   # E4
    N = 3
    eng, twin = guarded(cfg, N), guarded(cfg, N)
    xs = micro_inputs(cfg, N)
    nan_x = torch.full_like(xs[0], float("nan"))
    before, lr_before, st0 = all_arenas(eng), eng._lr_state.clone(), eng.grad_stats()
    for x in (xs[0], nan_x, xs[2]):   # a NaN in the second micro-batch's gradient reaches the sum
        eng.train_step(x)
    after = all_arenas(eng)
    g_slot, draw_slot = 1, 6
    keep = [i for i in range(len(before)) if i not in (g_slot, draw_slot)]
    assert same_bits([after[i] for i in keep], [before[i] for i in keep])          # p, m, v, dev_step, bias corrections, the average
    assert torch.equal(eng._lr_state, lr_before) and int(eng.dev_step.item()) == 0 == eng.step_count
    st = eng.grad_stats()
    assert st["n_skipped"] == st0["n_skipped"] + 1 and st["n_clipped"] == st0["n_clipped"] and st["skip"] == 1
    assert acc_is_zero(eng) and eng.accum_pending == 0 and int(eng.dev_draw.item()) == N
    # the next, clean cycle equals a twin's first cycle that never saw the bad one (its draw counter three draws on)
    twin.dev_draw.add_(N)
    for x in xs:
        eng.train_step(x)
        twin.train_step(x)
    assert same_bits(all_arenas(eng), all_arenas(twin)) and int(eng.dev_step.item()) == 1
    assert torch.equal(eng._lr_state, twin._lr_state) and eng.lamb_stats() == twin.lamb_stats()
    assert eng.grad_stats()["n_skipped"] == 1 and twin.grad_stats()["n_skipped"] == 0 and acc_is_zero(eng)
    assert not torch.equal(eng.flat_p, before[0]) and not torch.equal(eng.flat_ema, before[7])


def case_lc_head_groups(cfg: Cfg, num_class: int = 11):   # E5
    N = 3
    eng, twin = gc.lc_engine(cfg, num_class), gc.lc_engine(cfg, num_class)
    head = [k for k in eng.offsets if k.startswith(("final_bn.", "final_fc."))]
    eng.set_param_groups([{"params": head, "lr": 1e-3, "weight_decay": 1e-3}])
    eng.set_grad_guard(skip_nonfinite=True)
    eng.set_grad_accum(N)
    live = torch.zeros(eng.numel, dtype=torch.bool)
    for k in head:
        o, n = eng.offsets[k]
        live[o:o + (n + 3) // 4 * 4] = True
    o, n = eng.offsets["backbone.layer1.0.conv1.weight"]
    eng.flat_g[o:o + n] = float("nan")   # a frozen parameter's slot: not read, not summed, not scaled
    xs = micro_inputs(cfg, N)
    target = (torch.arange(cfg.B) % num_class).to(cfg.device)
    p0 = eng.flat_p.detach().cpu().clone()
    for x in xs:
        eng.train_step(x, target)
        twin.forward(x, target, train=True)
        assert not bits(eng.flat_acc.detach().cpu())[~live].any()   # frozen slices of flat_acc stay +0
    st = eng.grad_stats()
    assert st["skip"] == 0 and st["n_skipped"] == 0 and math.isfinite(st["norm"]) and st["norm"] > 0
    assert int(eng.dev_step.item()) == 1 and acc_is_zero(eng) and torch.isnan(eng.flat_g[o:o + n]).all()
    p = eng.flat_p.detach().cpu()
    assert torch.isfinite(p).all() and torch.equal(bits(p)[~live], bits(p0)[~live]) and not torch.equal(p[live], p0[live])
    for name in eng.BUF:   # the running buffers moved once per micro-batch
        assert torch.equal(eng.BUF[name], twin.BUF[name]), name
    assert int(eng.BUF["backbone.bn1.num_batches_tracked"].item()) == N


def case_checkpoint(cfg: Cfg, tmp_path):   # E6
    from dpc_amd import checkpoint as ckpt
    N = 3
    a, b = gc.dpc_engine(cfg), gc.dpc_engine(cfg)
    a.set_grad_accum(N)
    xs = micro_inputs(cfg, 2 * N)
    a.train_step(xs[0])
    for refused in (lambda: ckpt.build_state(a, 1, "resnet18", 0.0, 1), a.state_dict):
        with pytest.raises(RuntimeError, match="accumulation cycle is open"):
            refused()
    a.train_step(xs[1])
    a.train_step(xs[2])
    state = ckpt.build_state(a, 1, "resnet18", 0.0, 1)
    assert state["accum_steps"] == N and float(state["optimizer"]["state"][0]["step"]) == 1.0
    path = str(tmp_path / "epoch1.pth.tar")
    ckpt.save_checkpoint(state, filename=path)
    b.set_grad_accum(N)
    ckpt.resume(b, path)
    assert int(b.dev_draw.item()) == N == int(a.dev_draw.item()) and b.step_count == 1
    for x in xs[N:]:
        a.train_step(x)
        b.train_step(x)
    assert same_bits(all_arenas(a), all_arenas(b)) and a.step_count == 2   # dropout included: the mask stream continued
    c = gc.dpc_engine(cfg)
    with pytest.warns(UserWarning, match="micro-batches per optimizer step"):
        ckpt.resume(c, path)
    assert "accum_steps" not in ckpt.build_state(c, 1, "resnet18", 0.0, 1)
    # reset_accum drops an open cycle; adopt_optimizer_state carries the sum and the position
    a.train_step(xs[0])
    d = gc.dpc_engine(cfg)
    d.adopt_optimizer_state(a)
    assert d.accum_steps == N and d.accum_pending == 1 and torch.equal(bits(d.flat_acc), bits(a.flat_acc)) and not acc_is_zero(d)
    a.reset_accum()
    assert a.accum_pending == 0 and acc_is_zero(a)
    a.set_grad_accum(1)
    assert a.accum_steps == 1 and ("accum", N) not in a._baked_scalars()


# ---------------------------------------------------------------------- captured steps (HIP device only)
class CountingExchange:
    """a one-bucket exchange (a callable on the whole arena) around `inner`, which may be None; counts how often it is entered"""

    def __init__(self, inner=None):
        self.inner, self.calls, self.floats = inner, 0, 0

    def __call__(self, flat):
        self.calls += 1
        self.floats += flat.numel()
        if self.inner is not None:
            self.inner(flat)


class CountingTwoBuckets(CountingExchange):
    """the two-bucket form: start(tail) / finish(head); one entry per start"""

    def start(self, tail):
        self.calls += 1
        self.floats += tail.numel()
        if self.inner is not None:
            self.inner.start(tail)

    def finish(self, head):
        self.floats += head.numel()
        if self.inner is not None:
            self.inner.finish(head)

    def __call__(self, flat):
        raise AssertionError("the two-bucket exchange is entered through start / finish")


def case_captured_step(cfg: Cfg, N: int, dtype, exchange=None, inner=None):   # E7
    """two cycles of replays against an eager twin, bit for bit.  exchange: None, "one" or "two" (buckets) around `inner`"""
    mk = {None: lambda: None, "one": lambda: CountingExchange(inner), "two": lambda: CountingTwoBuckets(inner)}[exchange]
    xs = micro_inputs(cfg, 3 * N)
    a, b, c = (gc.dpc_engine(cfg, dtype) for _ in range(3))
    ea, eb, ec = mk(), mk(), mk()
    for e, ex in ((a, ea), (b, eb)):
        e.set_grad_accum(N)
        for x in xs[:N]:   # an eager cycle sizes every lazy buffer; both engines take it
            e.train_step(x, allreduce=ex)
    for x in xs[:2]:
        c.train_step(x, allreduce=ec)
    # launches of forward + backward, and the capture without accumulation
    c.packed_for_step = -1
    l0 = c._launches
    c._forward_loss(xs[0], True)
    c.backward()
    fwd_bwd = c._launches - l0
    block = xs[0].clone()
    plain = c.capture_train_step(block, allreduce=ec, warmup=0)
    replay = a.capture_train_step(block, allreduce=ea, warmup=0)
    finishes = 2 if exchange == "two" else 1
    assert replay.micro.kernels == [fwd_bwd + 1] and len(replay.micro.graphs) == 1
    assert len(replay.last.kernels) == len(plain.kernels) and sum(replay.last.kernels) == sum(plain.kernels) + finishes
    if exchange == "two":
        assert [x - y for x, y in zip(replay.last.kernels, plain.kernels)] == [1, 1, 0]
    assert all(replay.micro.kernels) and all(replay.last.kernels)
    assert a.capture_train_step(block, allreduce=ea, warmup=0) is replay
    calls0 = ea.calls if ea is not None else 0
    for cyc in range(2):
        for j, x in enumerate(xs[(1 + cyc) * N:(2 + cyc) * N]):
            block.copy_(x)
            ra = replay().clone()
            rb = b.train_step(x, allreduce=eb).clone()
            assert torch.equal(bits(ra), bits(rb)) and a.accum_pending == b.accum_pending == (j + 1) % N
        assert same_bits(all_arenas(a), all_arenas(b)) and acc_is_zero(a), cyc
        if ea is not None:
            assert ea.calls - calls0 == cyc + 1 and ea.calls == eb.calls   # the exchange is entered once per cycle
    assert a.step_count == b.step_count == 3 == int(a.dev_step.item())
    a.set_grad_accum(N + 1)
    with pytest.raises(RuntimeError):
        replay()
    assert a.accum_pending == 0
    a.set_grad_accum(N)
    a.release_captures()
    c.release_captures()


# ---------------------------------------------------------------------- two ranks over gloo (simulator)
def _gloo_rank(rank: int, world: int, port: int, out_dir: str, widths):
    import torch.distributed as dist
    from dpc_amd.parallel import make_allreduce
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    cfg = Cfg(device="cpu", simulator=L.load_emulator(), widths=widths)
    N = 2
    out = {}
    for kind, wrap in (("one", CountingExchange), ("two", CountingTwoBuckets)):
        eng = gc.dpc_engine(cfg)
        eng.set_grad_accum(N)
        ex = wrap(make_allreduce(dist, world))
        gen = torch.Generator().manual_seed(500 + rank)   # every rank its own shard
        per_cycle = []
        for _ in range(2 * N):
            eng.train_step(torch.randn(gc.dpc_input(cfg).shape, generator=gen), allreduce=ex)
            per_cycle.append(ex.calls)
        out[kind] = {"calls": per_cycle, "p": eng.flat_p.clone(), "m": eng.flat_m.clone(), "g": eng.flat_g.clone(), "step": eng.step_count,
                     "floats": ex.floats, "numel": eng.numel, "acc0": acc_is_zero(eng)}
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def case_two_ranks(widths, tmp_path):   # E8
    import torch.multiprocessing as mp
    mp.spawn(_gloo_rank, args=(2, 29700 + os.getpid() % 200, str(tmp_path), tuple(widths)), nprocs=2, join=True)
    r = [torch.load(os.path.join(str(tmp_path), f"rank{i}.pt")) for i in range(2)]
    for kind in ("one", "two"):
        a, b = r[0][kind], r[1][kind]
        assert a["calls"] == b["calls"] == [0, 1, 1, 2]                        # one exchange per cycle, none for a non-final micro-batch
        assert a["floats"] == 2 * a["numel"]                                   # ... of the whole arena
        for key in ("p", "m", "g"):
            assert torch.equal(bits(a[key]), bits(b[key])), (kind, key)         # both ranks end bit-identical
        assert a["step"] == b["step"] == 2 and a["acc0"] and b["acc0"] and a["m"].abs().sum() > 0
    assert torch.equal(bits(r[0]["one"]["p"]), bits(r[0]["two"]["p"]))          # the two exchanges agree


# ---------------------------------------------------------------------- entries (simulator)
def _strip_times(out: str) -> str:
    return re.sub(r"T:\d+\.\d+", "T:", out)


def case_entries(emu, widths, capsys):   # C1
    from dpc_amd import lc_main, main as dpc_main
    common = ["--net", "resnet18", "--img_dim", "64", "--batch_size", "1", "--gpu", "0", "--print_freq", "1", "--dtype", "f32", "--num_seq", "4",
              "--epochs", "1"]
    for entry, extra in ((dpc_main, ["--pred_step", "1"]), (lc_main, ["--train_what", "head"])):
        run = lambda flags: (entry.main(common + extra + flags, _simulator=emu, _widths=widths), capsys.readouterr().out)[1]   # noqa: E731
        out = run(["--synthetic", "3", "--accum_steps", "2", "--clip_grad", "1e9", "--lr_schedule", "cosine"])
        lines = out.splitlines()
        assert lines.count("Accumulation: 2 micro-batches of 1 per optimizer step (effective batch 2), 1 batches per epoch dropped") == 1, out
        train = [ln for ln in lines if ln.startswith("Epoch: [0][")]
        assert len(train) == 2 and train[0].startswith("Epoch: [0][0/2]") and train[1].startswith("Epoch: [0][1/2]"), out   # the truncated epoch
        assert re.search(r"^Grad guard: 0 skipped, [01] clipped of 1 steps$", out, re.M), out                                # optimizer steps
        assert re.search(r"^LR schedule: cosine, warmup_steps 0, total_steps 1, ", out, re.M), out                           # epochs x optimizer steps
        out = run(["--synthetic", "2", "--accum_steps", "2"])
        assert "Accumulation: 2 micro-batches of 1 per optimizer step (effective batch 2)\n" in out and "dropped" not in out
        with pytest.raises((ValueError, SystemExit)):
            entry.main(common + extra + ["--synthetic", "2", "--accum_steps", "0"], _simulator=emu, _widths=widths)
        capsys.readouterr()
        off, one = run(["--synthetic", "1"]), run(["--synthetic", "1", "--accum_steps", "1"])
        assert "Accumulation" not in off and _strip_times(off) == _strip_times(one) and "Epoch: [0][0/1]" in off
