"""The parameter average of the fused Adam (dpc_adam_dev_ema / dpc_adam_groups_dev_ema / dpc_arena_swap in csrc/loss.hip,
BackboneEngine.set_ema / swap_ema / ema_weights / ema_state_dict, the checkpoint's 'ema' entry, optim.Adam(ema_decay=), the entries'
--ema / --ema_eval / --use_ema), shared by the CPU tier (host SIMT simulator, tests/test_ema_emu.py) and the GPU tier
(tests/test_ema_gpu.py).

The kernel does, per element and in f32,   e_new = e + w * (p_new - e),  w = 1 - d,  d = min(decay, (1 + t) / (10 + t)).
Bounds, all from the number format (f32, unit roundoff 2^-24):
  p / m / v       : bit-identical to the _ex entries on a twin copy -- the EMA arm must not change the update
  e_new           : 2^-23 * (|e_ref| + w |p_new - e|) against e + w (p_new - e) in f64, with p_new the bits the kernel wrote and w the
                    f32 value: three f32 roundings (the difference, the product, the sum) of half an ulp each, each on a quantity no
                    larger than |e_ref| + w |p_new - e| up to second order; a fused multiply-add drops one of them
  integer data, w = 1/2 : exact
  several steps   : the one-step bound summed over the steps (an error carried in e is multiplied by d < 1 per step)
"""
import os
import re
import warnings

import pytest
import torch

import adam_groups_cases as ac
import grad_guard_cases as gc
from dpc_amd import _lib as L
from kcases import K

U23 = 2.0 ** -23
B1, B2, EPS = ac.B1, ac.B2, ac.EPS
TILE = ac.TILE
bits = gc.bits
new_state = gc.new_state
# more floats than one launch of either Adam kernel or of the swap covers in one sweep (adam_dev_kernel / arena_swap_kernel: 8192
# workgroups x 256 lanes x 4 floats; adam_groups_kernel: 2048 workgroups x TILE): a workgroup takes a second tile, the last is partial
BIG = 8192 * 256 * 4 + TILE + 8


def f32(x):
    return torch.tensor(x, dtype=torch.float32)


def ema_weight(t: int, decay: float):
    """(d, 1 - d) as the kernel forms them: every operation in f32"""
    d = torch.minimum(f32(decay), f32(float(1 + t)) / f32(float(10 + t)))
    return float(d), float(f32(1.0) - d)


def ema_ref(e, p_new, w):
    """e + w (p_new - e) in f64 and the per-element bound"""
    e, p_new = e.double(), p_new.double()
    step = w * (p_new - e)
    ref = e + step
    return ref, U23 * (ref.abs() + step.abs())


def bias_corr(k: K, t: int = 3):
    return k.t(torch.tensor([1 - B1 ** t, 1 - B2 ** t], dtype=torch.float32))


def step_at(k: K, t: int):
    return k.t(torch.tensor([t], dtype=torch.int32))


def run_plain(k: K, arenas, lr, wd, bc, gscale, state=None, ema=None, step=None, decay=None):
    """dpc_adam_dev_ex, or with `ema` dpc_adam_dev_ema, on device copies; returns the host copies [p, g, m, v(, ema)]"""
    dev = [k.t(t.clone()) for t in arenas]
    n = arenas[0].numel()
    if ema is None:
        k.call("dpc_adam_dev_ex", *dev, n, lr, B1, B2, EPS, wd, bc, gscale, state)
    else:
        dev.append(k.t(ema.clone()))
        k.call("dpc_adam_dev_ema", *dev[:4], n, lr, B1, B2, EPS, wd, bc, gscale, state, dev[4], step, decay)
    k.sync()
    return [t.cpu() for t in dev]


def run_groups(k: K, arenas, tab, nseg, bc, gscale, state=None, ema=None, step=None, decay=None):
    dev = [k.t(t.clone()) for t in arenas]
    n = arenas[0].numel()
    if ema is None:
        k.call("dpc_adam_groups_dev_ex", *dev, n, tab, nseg, B1, B2, EPS, bc, gscale, state)
    else:
        dev.append(k.t(ema.clone()))
        k.call("dpc_adam_groups_dev_ema", *dev[:4], n, tab, nseg, B1, B2, EPS, bc, gscale, state, dev[4], step, decay)
    k.sync()
    return [t.cpu() for t in dev]


def same(a, b):
    return torch.equal(bits(a), bits(b))


def random_arenas(n, seed=11):
    gen = torch.Generator().manual_seed(seed)
    p0, g0 = torch.randn(n, generator=gen) * 0.5, torch.randn(n, generator=gen)
    m0, v0 = torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 1e-2
    e0 = p0 + torch.randn(n, generator=gen) * 0.05
    return p0, g0, m0, v0, e0


def layout_lr(lr):
    """adam_groups_cases.layout() with every non-zero learning rate replaced"""
    segs, n, sp = ac.layout()
    return [(b, e, lr if s_lr > 0 else 0.0, wd, a) for b, e, s_lr, wd, a in segs], n, sp


# ------------------------------------------------------------------ case 1
def case_exact(k: K):
    gen = torch.Generator().manual_seed(21)
    n = BIG
    p0 = torch.randint(-8, 9, (n,), generator=gen).float()
    e0 = torch.randint(-8, 9, (n,), generator=gen).float()
    e0[::3] = p0[::3]                      # the fixed point of the lerp form
    g0 = torch.randint(-3, 4, (n,), generator=gen).float()
    m0, v0 = torch.zeros(n), torch.zeros(n)
    bc, step = bias_corr(k), step_at(k, 1000)
    assert ema_weight(1000, 0.5) == (0.5, 0.5)
    want = (e0 + p0) / 2                   # exact in f32: small integers and halves
    ref = run_plain(k, (p0, g0, m0, v0), 0.0, 0.0, bc, 1.0)
    out = run_plain(k, (p0, g0, m0, v0), 0.0, 0.0, bc, 1.0, None, e0, step, 0.5)
    assert same(out[4], want) and same(out[0], p0) and same(out[1], g0)
    assert same(out[2], ref[2]) and same(out[3], ref[3]) and not same(out[2], m0)
    assert same(out[4][::3], e0[::3])
    tab = ac.table(k, [(0, n, 0.0, 0.0, 1)])
    ref = run_groups(k, (p0, g0, m0, v0), tab, 1, bc, 1.0)
    out = run_groups(k, (p0, g0, m0, v0), tab, 1, bc, 1.0, None, e0, step, 0.5)
    assert same(out[4], want) and same(out[0], p0) and same(out[2], ref[2]) and same(out[3], ref[3])
    assert int(step.cpu()) == 1000         # the counter is only read


# ------------------------------------------------------------------ case 2
def check_ema(out_e, e0, p_new, w, sel=None, report=print, what=""):
    ref, bound = ema_ref(e0, p_new, w)
    err = (out_e.double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300))
    ratio = ratio if sel is None else ratio[sel]
    report(f"{what}: ema vs f64 lerp, worst error / bound = {ratio.max().item():.3g}")
    assert ratio.max().item() <= 1.0
    return ref, bound


def case_rounding(k: K, report=print):
    lr, decay, t = 1e-2, 0.9, 100000
    d, w = ema_weight(t, decay)
    assert d == float(f32(decay))
    bc, step = bias_corr(k), step_at(k, t)
    segs, n, sp = layout_lr(lr)
    act = gc.live_mask(segs, n)
    tab = ac.table(k, segs)
    p0, g0, m0, v0, e0 = random_arenas(n)
    for name, run, sel in (("plain", lambda **kw: run_plain(k, (p0, g0, m0, v0), lr, 1e-5, bc, 0.5, **kw), torch.ones(n, dtype=torch.bool)),
                           ("groups", lambda **kw: run_groups(k, (p0, g0, m0, v0), tab, len(segs), bc, 0.5, **kw), act)):
        ref = run()
        out = run(ema=e0, step=step, decay=decay)
        assert all(same(a, b) for a, b in zip(out[:4], ref))        # the EMA arm does not change the update
        assert not same(out[0][sel], p0[sel])
        e_ref, bound = check_ema(out[4], e0, out[0], w, sel, report, "rounding, " + name)
        assert same(out[4][~sel], e0[~sel])
        # a kernel that averaged the parameter from before the update would be caught: the same reference fed p_old lies
        # outside the bound for more than half of the elements (host arithmetic only)
        old_ref, _ = ema_ref(e0, p0, w)
        outside = ((old_ref - e_ref).abs() > 2 * bound)[sel]     # (2 x: no value lies within the bound of both references)
        assert outside.float().mean().item() > 0.5
    # a length that is no multiple of four: the last lanes take the scalar path of adam_dev_kernel
    n2 = 4 * 300 + 3
    q = [t_[:n2].clone() for t_ in (p0, g0, m0, v0, e0)]
    ref = run_plain(k, q[:4], lr, 1e-5, bc, 0.5)
    out = run_plain(k, q[:4], lr, 1e-5, bc, 0.5, None, q[4], step, decay)
    assert all(same(a, b) for a, b in zip(out[:4], ref))
    check_ema(out[4], q[4], out[0], w, None, report, "rounding, odd length")
    assert not same(out[4][-3:], q[4][-3:])


# ------------------------------------------------------------------ case 3
def case_warmup(k: K, report=print):
    n = 4 * 256 + 4
    p0, g0, m0, v0, e0 = random_arenas(n, seed=12)
    # (decay, step counter before dpc_step_advance, t the kernel reads).  (1 + t) / (10 + t) reaches d at t = (10 d - 1) / (1 - d):
    # 80 for 0.9, 890 for 0.99
    plan = ((0.9, 0, 1), (0.9, 78, 79), (0.9, 79, 80), (0.9, 169, 170), (0.99, 888, 889), (0.99, 980, 981))
    for decay, preset, t in plan:
        step, bc = step_at(k, preset), k.t(torch.ones(2))
        k.call("dpc_step_advance", step, bc, B1, B2)       # as the engine does in front of the update
        k.sync()
        assert int(step.cpu()) == t
        d, w = ema_weight(t, decay)
        if t == 1:
            assert d == float(f32(2.0) / f32(11.0))
        if t in (170, 981):
            assert d == float(f32(decay))
        if t in (79, 889):
            assert d < float(f32(decay))
        out = run_plain(k, (p0, g0, m0, v0), 1e-2, 0.0, bc, 1.0, None, e0, step, decay)
        ref, bound = check_ema(out[4], e0, out[0], w, None, report, f"warm-up, decay {decay}, t {t}")
        if t == 1:   # the warm-up is not optional: the plain factor 1 - decay is far outside the bound
            wrong, _ = ema_ref(e0, out[0], float(f32(1.0) - f32(decay)))
            assert ((wrong - ref).abs() > 2 * bound).float().mean().item() > 0.9


# ------------------------------------------------------------------ case 4
def case_untouched(k: K, report=print):
    lr, decay, t = 1e-2, 0.9, 100000
    _, w = ema_weight(t, decay)
    bc, step = bias_corr(k), step_at(k, t)
    segs, n, sp = layout_lr(lr)
    act = gc.live_mask(segs, n)
    tab = ac.table(k, segs)
    p0, g0, m0, v0, e0 = random_arenas(n)
    fb, fe = segs[sp["frozen"]][:2]
    ga, gb = sp["gap"]
    e1 = e0.clone()
    e1[fb:fe] = float("nan")
    e1[ga:gb] = float("inf")
    four = (p0, g0, m0, v0)
    out = run_groups(k, four, tab, len(segs), bc, 0.5, None, e1, step, decay)
    assert same(out[4][~act], e1[~act]) and torch.isnan(out[4][fb:fe]).all() and torch.isinf(out[4][ga:gb]).all()
    assert not same(out[4][act], e1[act])
    # a guard record that says skip: all five arenas keep every bit, with either entry
    skip = new_state(k, coef=0.0, skip=1)
    for got in (run_groups(k, four, tab, len(segs), bc, 0.5, skip, e1, step, decay),
                run_plain(k, four, lr, 1e-5, bc, 0.5, skip, e1, step, decay)):
        assert all(same(a, b) for a, b in zip(got, four + (e1,)))
    # coef 0.25: the update of the _ex entry with the same record, and the average follows the new parameter
    quarter = new_state(k, coef=0.25)
    for name, ref, got, sel in (("groups", run_groups(k, four, tab, len(segs), bc, 0.5, quarter),
                                 run_groups(k, four, tab, len(segs), bc, 0.5, quarter, e0, step, decay), act),
                                ("plain", run_plain(k, four, lr, 1e-5, bc, 0.5, quarter),
                                 run_plain(k, four, lr, 1e-5, bc, 0.5, quarter, e0, step, decay), torch.ones(n, dtype=torch.bool))):
        assert all(same(a, b) for a, b in zip(got[:4], ref))
        check_ema(got[4], e0, got[0], w, sel, report, "coef 0.25, " + name)
    unclipped = run_plain(k, four, lr, 1e-5, bc, 0.5, new_state(k, coef=1.0), e0, step, decay)
    assert not same(unclipped[0], got[0]) and not same(unclipped[4], got[4])


# ------------------------------------------------------------------ case 5
def case_swap_and_argument_checks(k: K):
    gen = torch.Generator().manual_seed(31)
    n = BIG
    a0 = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=gen, dtype=torch.int64).to(torch.int32)   # every bit pattern, NaN payloads included
    b0 = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=gen, dtype=torch.int64).to(torch.int32)
    a0[:4] = torch.tensor([0x7FC00001, 0x7F800001, -1, 0x7FA5A5A5], dtype=torch.int64).to(torch.int32)   # quiet and signalling NaNs with payloads
    assert torch.isnan(a0.view(torch.float32)[:4]).all()
    a, b = k.t(a0.view(torch.float32).clone()), k.t(b0.view(torch.float32).clone())
    k.call("dpc_arena_swap", a, b, n)
    k.sync()
    assert torch.equal(a.cpu().view(torch.int32), b0) and torch.equal(b.cpu().view(torch.int32), a0)
    k.call("dpc_arena_swap", a, b, n)
    k.sync()
    assert torch.equal(a.cpu().view(torch.int32), a0) and torch.equal(b.cpu().view(torch.int32), b0)

    segs, m, _ = ac.layout()
    tab, S = ac.table(k, segs), len(segs)
    four = [k.t(torch.zeros(m + 4)) for _ in range(4)]
    ema = k.t(torch.zeros(m + 4))
    step, bc, st = step_at(k, 5), bias_corr(k), new_state(k, coef=1.0)
    plain = lambda p=four[0], e=ema, s=step, d=0.9, state=st: k.call(   # noqa: E731
        "dpc_adam_dev_ema", p, *four[1:], m, 1e-3, B1, B2, EPS, 0.0, bc, 1.0, state, e, s, d)
    groups = lambda p=four[0], e=ema, s=step, d=0.9, nn=m, tb=tab, ns=S: k.call(   # noqa: E731
        "dpc_adam_groups_dev_ema", p, *four[1:], nn, tb, ns, B1, B2, EPS, bc, 1.0, st, e, s, d)
    bad = [
        lambda: plain(e=None), lambda: plain(e=ema[1:]), lambda: plain(e=four[0]), lambda: plain(s=None),
        lambda: plain(d=0.0), lambda: plain(d=1.0), lambda: plain(d=-0.5), lambda: plain(d=float("nan")), lambda: plain(p=None),
        lambda: groups(e=None), lambda: groups(e=ema[1:]), lambda: groups(e=four[0]), lambda: groups(s=None),
        lambda: groups(d=0.0), lambda: groups(d=1.0), lambda: groups(d=float("nan")), lambda: groups(p=four[0][1:]),
        lambda: groups(nn=m + 2), lambda: groups(tb=None), lambda: groups(ns=0), lambda: groups(ns=L.ADAM_MAX_SEGMENTS + 1),
        lambda: k.call("dpc_arena_swap", None, ema, m), lambda: k.call("dpc_arena_swap", ema, None, m),
        lambda: k.call("dpc_arena_swap", ema, ema, m), lambda: k.call("dpc_arena_swap", ema, four[0], m + 2),
        lambda: k.call("dpc_arena_swap", ema[1:], four[0], m), lambda: k.call("dpc_arena_swap", ema, four[0][1:], m),
        lambda: k.call("dpc_arena_swap", ema, four[0], 0),
    ]
    for f in bad:
        with pytest.raises(L.DpcError, match=f"code {L.ERR_ARG}$"):
            f()
    plain(state=None)     # the guard's record is optional, as in the _ex entries
    groups()
    k.sync()


# ====================================================================== engine, checkpoints, module boundary, entries
Cfg = gc.Cfg
dpc_engine, dpc_input, lc_engine = gc.dpc_engine, gc.dpc_input, gc.lc_engine
DECAY = 0.9


def arenas(eng):
    return gc.arenas(eng)   # flat_p, flat_m, flat_v, dev_step, dev_bc


def same_bits(a, b):
    return gc.same_bits(a, b)


_RUNS = {}


def twin(cfg: Cfg, dtype=torch.float32):
    """the engine without an average, computed once per configuration and never changed afterwards: after each of three train steps
    the arenas, the launches the step issued and the kernel it launched last"""
    key = ("twin", cfg.device, tuple(cfg.widths), dtype)
    if key not in _RUNS:
        eng, x = dpc_engine(cfg, dtype), dpc_input(cfg)
        rec = {"p0": eng.flat_p.detach().clone(), "steps": []}
        for _ in range(3):
            n0 = eng._launches
            eng.train_step(x)
            rec["steps"].append({"arenas": arenas(eng), "launches": eng._launches - n0, "last": L.last_kernel(eng.lib)})
        assert eng.ema_decay is None and eng.flat_ema is None      # off: nothing allocated
        _RUNS[key] = rec
    return _RUNS[key]


def ema_run(cfg: Cfg, dtype=torch.float32):
    """three train steps with set_ema(DECAY), computed once: after each step the arenas and flat_ema; after the second the
    checkpoint dictionary"""
    from dpc_amd import checkpoint as ckpt
    key = ("ema", cfg.device, tuple(cfg.widths), dtype)
    if key not in _RUNS:
        eng, x = dpc_engine(cfg, dtype), dpc_input(cfg)
        eng.set_ema(DECAY)
        rec = {"p0": eng.flat_p.detach().clone(), "e0": eng.flat_ema.detach().clone(), "steps": []}
        for i in range(3):
            n0 = eng._launches
            eng.train_step(x)
            rec["steps"].append({"arenas": arenas(eng), "ema": eng.flat_ema.detach().clone(), "launches": eng._launches - n0,
                                 "last": L.last_kernel(eng.lib)})
            if i == 1:
                rec["state2"] = ckpt.build_state(eng, 1, "resnet18", 0.0, 2)
        _RUNS[key] = rec
    return _RUNS[key]


def case_ema_does_not_change_training(cfg: Cfg, dtype=torch.float32):   # case 6
    ref, run = twin(cfg, dtype), ema_run(cfg, dtype)
    assert same_bits([run["e0"]], [run["p0"]]) and same_bits([run["p0"]], [ref["p0"]])   # seeded with a copy of the parameters
    for a, b in zip(run["steps"], ref["steps"]):
        assert same_bits(a["arenas"], b["arenas"])
        assert a["launches"] == b["launches"] and "<true>" in a["last"] and "<false>" in b["last"]   # no launch of its own
    assert not torch.equal(run["steps"][2]["ema"], run["steps"][2]["arenas"][0]) and not torch.equal(run["steps"][2]["ema"], run["e0"])
    # off after having been on: the launches of the twin
    eng, x = dpc_engine(cfg, dtype), dpc_input(cfg)
    eng.set_ema(DECAY)
    base = eng._baked_scalars()
    assert base[-1] == ("ema", DECAY)
    eng.set_ema(None)
    assert eng.ema_decay is None and eng._baked_scalars() == base[:-1]
    n0 = eng._launches
    eng.train_step(x)
    first = ref["steps"][0]
    assert eng._launches - n0 == first["launches"] and L.last_kernel(eng.lib) == first["last"] and "<false>" in first["last"]
    assert same_bits(arenas(eng), first["arenas"]) and same_bits([eng.flat_ema], [run["e0"]])    # the average stood still
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            eng.set_ema(bad)


def recurrence(e0, ps, decay, t0=0):
    """the host recurrence in f64 over the parameters read back after each step, and the summed one-step bounds"""
    e, bound, out = e0.detach().cpu().double(), 0.0, []
    for i, p in enumerate(ps):
        _, w = ema_weight(t0 + i + 1, decay)
        p = p.detach().cpu().double()
        step = w * (p - e)
        e = e + step
        bound = bound + U23 * (e.abs() + step.abs())
        out.append((e, bound))
    return out


def case_matches_the_host_recurrence(cfg: Cfg, report=print):   # case 7
    run = ema_run(cfg)
    want = recurrence(run["e0"], [s["arenas"][0] for s in run["steps"]], DECAY)
    for i, (s, (e, bound)) in enumerate(zip(run["steps"], want)):
        ratio = ((s["ema"].cpu().double() - e).abs() / bound.clamp_min(1e-300)).max().item()
        report(f"flat_ema after step {i + 1} vs the f64 recurrence: worst error / bound = {ratio:.3g}")
        assert ratio <= 1.0
        assert int(s["arenas"][3].item()) == i + 1
    # the warm-up was in force (t = 1..3: 2/11, 3/12, 4/13, all below 0.9): the plain factor would be far off
    plain = run["e0"].cpu().double() + (1 - DECAY) * (run["steps"][0]["arenas"][0].cpu().double() - run["e0"].cpu().double())
    assert ((plain - want[0][0]).abs() > 2 * want[0][1]).float().mean().item() > 0.5


def case_evaluating_with_the_averaged_weights(cfg: Cfg):   # case 8
    ref = twin(cfg)
    eng, x = dpc_engine(cfg), dpc_input(cfg)
    eng.set_ema(DECAY)
    eng.train_step(x)
    p_before, e_before = eng.flat_p.detach().clone(), eng.flat_ema.detach().clone()
    averaged = eng.ema_state_dict()
    assert set(averaged) == set(eng.state_dict()) and "agg.cell_list.0.update_gate.weight" in averaged
    assert torch.equal(averaged["agg.cell_list.0.update_gate.weight"], averaged["agg.ConvGRUCell_00.update_gate.weight"])
    o, n = eng.offsets["backbone.layer2.0.conv1.weight"]
    assert same_bits([averaged["backbone.layer2.0.conv1.weight"].reshape(-1)], [e_before[o:o + n]])

    def evaluate(e):
        e.forward(x, train=False, materialise=False)
        return e.loss_topk(with_grad=False).detach().clone()

    raw = evaluate(eng)
    with eng.ema_weights() as inside:
        assert inside is eng and same_bits([eng.flat_p, eng.flat_ema], [e_before, p_before])
        got = evaluate(eng)
        for f in (lambda: eng.train_step(x), lambda: eng.adam_step(), lambda: eng.state_dict(), lambda: eng.ema_state_dict(),
                  lambda: eng.ema_weights().__enter__()):
            with pytest.raises(RuntimeError, match="averaged weights"):
                f()
        from dpc_amd import checkpoint as ckpt
        with pytest.raises(RuntimeError, match="averaged weights"):
            ckpt.build_state(eng, 1, "resnet18", 0.0, 2)
    third = dpc_engine(cfg)
    third.load_params(averaged)
    want = evaluate(third)
    assert same_bits([got], [want]) and not same_bits([got], [raw])
    assert same_bits([eng.flat_p, eng.flat_ema], [p_before, e_before])
    eng.train_step(x)                                  # ... from the trained weights, repacked
    assert same_bits(arenas(eng), ref["steps"][1]["arenas"])
    plain = dpc_engine(cfg)
    for f in (plain.swap_ema, plain.ema_state_dict, lambda: plain.ema_weights().__enter__()):
        with pytest.raises(RuntimeError, match="never enabled"):
            f()


def case_groups(cfg: Cfg, num_class: int = 11, report=print):   # case 9
    eng, x = lc_engine(cfg, num_class), dpc_input(cfg)
    head = [k for k in eng.offsets if k.startswith(("final_bn.", "final_fc."))]   # lc_main --train_what head
    eng.set_param_groups([{"params": head, "lr": 1e-3, "weight_decay": 1e-3}])
    eng.set_grad_guard(skip_nonfinite=True)
    eng.set_ema(DECAY)
    live = torch.zeros(eng.numel, dtype=torch.bool)
    for k in head:
        o, n = eng.offsets[k]
        live[o:o + n] = True
    live = live.to(cfg.device)
    target = (torch.arange(cfg.B) % num_class).to(cfg.device)
    e0, ps = eng.flat_ema.detach().clone(), []
    for _ in range(2):
        eng.train_step(x, target)
        ps.append(eng.flat_p.detach().clone())
    assert same_bits([eng.flat_ema[~live]], [e0[~live]])                 # the frozen backbone's slices keep their seed bits
    e, bound = recurrence(e0, ps, DECAY)[-1]
    ratio = ((eng.flat_ema.cpu().double() - e).abs() / bound.clamp_min(1e-300))[live.cpu()].max().item()
    report(f"head slices of flat_ema after two grouped steps: worst error / bound = {ratio:.3g}")
    assert ratio <= 1.0 and not torch.equal(eng.flat_ema[live], e0[live])
    # a NaN gradient under skip_nonfinite: the average keeps every bit
    before = [t.detach().clone() for t in (eng.flat_p, eng.flat_m, eng.flat_v, eng.flat_ema, eng.dev_step)]
    eng.forward(x, target, train=True)
    eng.backward()
    o, _ = eng.offsets["final_fc.1.weight"]
    eng.flat_g[o + 3] = float("nan")
    eng.adam_step()
    assert eng.grad_stats()["skip"] == 1
    assert same_bits([eng.flat_p, eng.flat_m, eng.flat_v, eng.flat_ema, eng.dev_step], before)
    # the running buffers are shared, not averaged
    sd, av = eng.state_dict(), eng.ema_state_dict()
    assert set(sd) == set(av) and all(torch.equal(sd[k], av[k]) for k in eng.BUF)
    assert not torch.equal(sd["final_fc.1.weight"], av["final_fc.1.weight"])


def case_checkpoint_round_trip(cfg: Cfg, tmp_path):   # case 10
    from dpc_amd import checkpoint as ckpt
    run, ref = ema_run(cfg), twin(cfg)
    x = dpc_input(cfg)
    state = run["state2"]
    assert list(state)[-1] == "ema" and state["ema"]["decay"] == DECAY
    assert list(state["ema"]["state_dict"]) == list(state["state_dict"])
    assert all(v.device.type == "cpu" for v in state["ema"]["state_dict"].values())
    fn = str(tmp_path / "epoch1.pth.tar")
    ckpt.save_checkpoint(state, filename=fn)
    # resumed with the average on: flat_ema bit-identical, the third step that of the uninterrupted run
    b = dpc_engine(cfg)
    b.set_ema(DECAY)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ckpt.resume(b, fn)
    assert same_bits([b.flat_ema], [run["steps"][1]["ema"]]) and same_bits(arenas(b)[:4], run["steps"][1]["arenas"][:4])
    b.train_step(x)
    assert same_bits(arenas(b) + [b.flat_ema], run["steps"][2]["arenas"] + [run["steps"][2]["ema"]])
    # the same file resumed with the average off: as today
    c = dpc_engine(cfg)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ckpt.resume(c, fn)
    assert c.flat_ema is None and c.ema_decay is None
    c.train_step(x)
    assert same_bits(arenas(c), ref["steps"][2]["arenas"])
    assert "ema" not in ckpt.build_state(c, 1, "resnet18", 0.0, 2)
    # a file written without the average, resumed with it on: one warning, seeded from the loaded parameters
    fn2 = str(tmp_path / "plain.pth.tar")
    ckpt.save_checkpoint({k: v for k, v in state.items() if k != "ema"}, filename=fn2)
    d = dpc_engine(cfg)
    d.set_ema(DECAY)
    with pytest.warns(UserWarning, match="no averaged weights") as rec:
        ckpt.resume(d, fn2)
    assert len([w for w in rec if "no averaged weights" in str(w.message)]) == 1
    assert same_bits([d.flat_ema, d.flat_p], [run["steps"][1]["arenas"][0]] * 2)
    # pretrain(use_ema=True) loads the averages, and raises on a file without them
    e = dpc_engine(cfg)
    ckpt.pretrain(e, fn, log=lambda *a: None, use_ema=True)
    assert same_bits([e.flat_p], [run["steps"][1]["ema"]]) and e.flat_ema is None
    ckpt.pretrain(e, fn, log=lambda *a: None)
    assert same_bits([e.flat_p], [run["steps"][1]["arenas"][0]])
    with pytest.raises(KeyError, match=re.escape(fn2)):
        ckpt.pretrain(e, fn2, log=lambda *a: None, use_ema=True)
    # adopt_optimizer_state carries the arena and the setting
    f = dpc_engine(cfg)
    f.load_params(b.state_dict())
    f.adopt_optimizer_state(b)
    assert f.ema_decay == DECAY and same_bits([f.flat_ema], [b.flat_ema]) and f.flat_ema.data_ptr() != b.flat_ema.data_ptr()


def case_captured_step(cfg: Cfg):   # case 11, HIP device only
    x = dpc_input(cfg)
    a, b = dpc_engine(cfg), dpc_engine(cfg)
    for e in (a, b):
        e.set_ema(DECAY)
        for _ in range(2):   # eager steps size every lazy buffer; both engines take them
            e.train_step(x)
    block = x.clone()
    replay = a.capture_train_step(block, warmup=0)
    for _ in range(3):
        replay()
        b.train_step(x)
    assert same_bits(arenas(a) + [a.flat_ema], arenas(b) + [b.flat_ema]) and a.step_count == 5 == int(a.dev_step.item())
    assert not torch.equal(a.flat_ema, a.flat_p)
    a.set_ema(0.5)
    with pytest.raises(RuntimeError, match="changed since"):
        replay()
    a.set_ema(DECAY)
    # a captured eval step replayed inside ema_weights() == the eager eval of an engine loaded from the averages
    a.forward(x, train=False, materialise=False)          # one eager evaluation first (capture_eval_step's rule); fills the operand
    a.loss_topk(with_grad=False)
    ev = a.capture_eval_step()
    raw = ev().detach().clone()
    with a.ema_weights():
        got = ev().detach().clone()
        with pytest.raises(RuntimeError, match="averaged weights"):
            replay()
    third = dpc_engine(cfg)
    third.load_params(a.ema_state_dict())
    third.forward(x, train=False, materialise=False)
    want = third.loss_topk(with_grad=False).detach().clone()
    assert same_bits([got], [want]) and not same_bits([got], [raw])
    assert same_bits([ev().detach().clone()], [raw])
    replay()
    b.train_step(x)
    assert same_bits(arenas(a) + [a.flat_ema], arenas(b) + [b.flat_ema])
    a.release_captures()


def case_module_boundary(cfg: Cfg, num_class: int = 11, report=print):   # case 12
    import lc_loop_cases as lc
    from dpc_amd import optim
    c = lc.Cfg(device=cfg.device, simulator=cfg.simulator, widths=cfg.widths, num_class=num_class, size=cfg.size, B=cfg.B, N=cfg.N, SL=cfg.SL)
    m = lc.module(c, pcg=True)
    m._forced_masks = lc.masks(c)[0]
    x = dpc_input(cfg)
    target = (torch.arange(cfg.B) % num_class).to(cfg.device).view(cfg.B, 1)
    opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-3, ema_decay=DECAY)
    criterion = torch.nn.CrossEntropyLoss()
    lc.ref_loop_step(m, opt, x, target, criterion)          # eval/test.py:228-255
    eng = m.engine
    assert eng.ema_decay == DECAY
    # the second step, taken twice from the same state: through the optimizer and by the engine itself
    names = ("flat_p", "flat_g", "flat_m", "flat_v", "flat_ema")
    output, _ = m(x)
    loss = criterion(output.view(cfg.B, -1), target.view(-1))
    opt.zero_grad()
    loss.backward()
    snap = [getattr(eng, k).detach().clone() for k in names]
    opt.step()
    via_optim = [getattr(eng, k).detach().clone() for k in names]
    for k, s in zip(names, snap):
        getattr(eng, k).copy_(s)
    eng.step_count = 1
    eng.adam_step()
    assert same_bits([getattr(eng, k) for k in names], via_optim) and int(eng.dev_step.item()) == 2
    assert not torch.equal(via_optim[4], snap[4])
    # ... and both follow the host recurrence from the first step's average
    e, bound = recurrence(snap[4], [via_optim[0]], DECAY, t0=1)[0]
    ratio = ((via_optim[4].cpu().double() - e).abs() / bound.clamp_min(1e-300)).max().item()
    report(f"module boundary, second step: worst error / bound = {ratio:.3g}")
    assert ratio <= 1.0
    # with optim.ema_weights(optimizer): model.parameters() show the averaged values, and get the trained ones back
    trained = [q.detach().clone() for q in m.parameters()]
    by_ptr = {t.data_ptr(): k for k, t in eng.PRM.items()}
    with optim.ema_weights(opt):
        for q in m.parameters():
            o, n = eng.offsets[by_ptr[q.data_ptr()]]
            assert same_bits([q.detach().reshape(-1)], [via_optim[4][o:o + n]])
        with pytest.raises(RuntimeError, match="averaged weights"):
            opt.step()
    assert all(same_bits([q.detach()], [t]) for q, t in zip(m.parameters(), trained))
    with pytest.raises(ValueError):
        optim.Adam(m.parameters(), ema_decay=1.0)


# ---------------------------------------------------------------------- entries (simulator)
COMMON = ["--net", "resnet18", "--img_dim", "64", "--batch_size", "1", "--gpu", "0", "--print_freq", "1", "--dtype", "f32", "--num_seq", "4"]


def case_entry_main(emu, widths, capsys, tmp_path):   # case 13, dpc_amd.main
    from dpc_amd import main as dpc_main
    d = str(tmp_path / "run")
    argv = COMMON + ["--pred_step", "1", "--synthetic", "3", "--epochs", "2", "--save_dir", d]
    pr = str(tmp_path / "probe")
    os.makedirs(pr)
    dpc_main.main(argv + ["--ema", "0.9", "--ema_eval"], _simulator=emu, _widths=widths, _probe=pr)
    out = capsys.readouterr().out
    assert out.count("EMA: decay 0.9\n") == 1 and "Epoch: [1][2/3]" in out, out
    end = torch.load(os.path.join(pr, "rank0.pt"))
    fn = os.path.join(d, "epoch2.pth.tar")
    ck = torch.load(fn, map_location="cpu", weights_only=False)
    assert ck["epoch"] == 2 and ck["ema"]["decay"] == 0.9 and list(ck["ema"]["state_dict"]) == list(ck["state_dict"])
    k = "module.backbone.layer2.0.conv1.weight"
    assert not torch.equal(ck["ema"]["state_dict"][k], ck["state_dict"][k])
    assert end["step"] == 6 and not torch.equal(end["flat_ema"], end["flat_p"])
    # resumes: the file's average ends up in flat_ema (no epoch is left to run, so the probe shows the arenas as loaded)
    pr2 = str(tmp_path / "probe2")
    os.makedirs(pr2)
    dpc_main.main(argv + ["--ema", "0.9", "--resume", fn], _simulator=emu, _widths=widths, _probe=pr2)
    out = capsys.readouterr().out
    assert "=> loaded resumed checkpoint" in out and "Epoch: [" not in out
    got = torch.load(os.path.join(pr2, "rank0.pt"))
    assert got["step"] == 6 and same(got["flat_ema"], end["flat_ema"]) and same(got["flat_p"], end["flat_p"])
    # without the flags: no line, no key
    d0 = str(tmp_path / "plain")
    dpc_main.main(COMMON + ["--pred_step", "1", "--synthetic", "1", "--epochs", "1", "--save_dir", d0], _simulator=emu, _widths=widths)
    out = capsys.readouterr().out
    assert "EMA" not in out
    assert "ema" not in torch.load(os.path.join(d0, "epoch1.pth.tar"), map_location="cpu", weights_only=False)


def case_flag_errors(emu, widths):
    from dpc_amd import lc_main, main as dpc_main
    for entry, extra in ((dpc_main, ["--pred_step", "1"]), (lc_main, ["--train_what", "head"])):
        base = COMMON + extra + ["--synthetic", "1", "--epochs", "1"]
        with pytest.raises(ValueError, match="--ema_eval needs --ema"):
            entry.main(base + ["--ema_eval"], _simulator=emu, _widths=widths)
        for bad in ("1.0", "-0.5", "1.5"):
            with pytest.raises(ValueError, match="--ema must lie in"):
                entry.main(base + ["--ema", bad], _simulator=emu, _widths=widths)


def case_two_ranks(emu, widths, tmp_path):
    from dpc_amd import main as dpc_main
    pr = str(tmp_path / "probe")
    os.makedirs(pr)
    dpc_main.main(["--net", "resnet18", "--img_dim", "64", "--batch_size", "2", "--gpu", "0,1", "--synthetic", "2", "--print_freq", "1",
                   "--dtype", "f32", "--num_seq", "4", "--pred_step", "1", "--epochs", "1", "--ema", "0.9"],
                  _simulator=emu, _widths=widths, _probe=pr)
    r = [torch.load(os.path.join(pr, f"rank{i}.pt")) for i in range(2)]
    assert torch.equal(r[0]["flat_ema"].view(torch.int32), r[1]["flat_ema"].view(torch.int32)) and torch.equal(r[0]["flat_p"], r[1]["flat_p"])
    assert all(x["step"] == 2 for x in r) and not torch.equal(r[0]["flat_ema"], r[0]["flat_p"]) and torch.isfinite(r[0]["flat_ema"]).all()


def case_entry_lc(emu, widths, capsys, tmp_path):   # case 13, dpc_amd.lc_main
    from dpc_amd import lc_main
    d = str(tmp_path / "lc")
    base = COMMON + ["--synthetic", "2"]
    lc_main.main(base + ["--train_what", "head", "--epochs", "1", "--ema", "0.9", "--ema_eval", "--save_dir", d], _simulator=emu, _widths=widths)
    out = capsys.readouterr().out
    assert out.count("EMA: decay 0.9\n") == 1, out
    fn = os.path.join(d, "epoch1.pth.tar")
    ck = torch.load(fn, map_location="cpu", weights_only=False)
    av, sd = ck["ema"]["state_dict"], ck["state_dict"]
    assert ck["ema"]["decay"] == 0.9 and list(av) == list(sd)
    assert not torch.equal(av["module.final_fc.1.weight"], sd["module.final_fc.1.weight"])
    assert torch.equal(av["module.final_bn.running_mean"], sd["module.final_bn.running_mean"])                # shared, not averaged
    assert torch.equal(av["module.backbone.layer2.0.conv1.weight"], sd["module.backbone.layer2.0.conv1.weight"])   # frozen: its seed

    def totals(argv):
        lc_main.main(argv, _simulator=emu, _widths=widths)
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Loss ")]
        assert len(lines) == 1
        return lines[0]

    # --test CKPT --use_ema == --test of a file loaded by hand from the averages (parameters from 'ema', buffers from 'state_dict')
    by_hand = dict(ck)
    by_hand["state_dict"] = {k: (sd[k] if "running_" in k or "num_batches" in k else av[k]) for k in sd}
    del by_hand["ema"]
    fn2 = os.path.join(d, "by_hand.pth.tar")
    torch.save(by_hand, fn2)
    with_flag, hand, raw = totals(base + ["--test", fn, "--use_ema"]), totals(base + ["--test", fn2]), totals(base + ["--test", fn])
    assert with_flag == hand and with_flag != raw
    with pytest.raises(KeyError, match=re.escape(fn2)):
        lc_main.main(base + ["--test", fn2, "--use_ema"], _simulator=emu, _widths=widths)
    # --resume reads the file's average
    pr = str(tmp_path / "probe")
    os.makedirs(pr)
    lc_main.main(base + ["--train_what", "head", "--epochs", "1", "--ema", "0.9", "--resume", fn], _simulator=emu, _widths=widths, _probe=pr)
    capsys.readouterr()
    got = torch.load(os.path.join(pr, "rank0.pt"))    # no epoch left to run: the arenas are those of the file
    eng = lc_engine(Cfg(device="cpu", simulator=emu, widths=widths, B=1), 101)
    o, n = eng.offsets["final_fc.1.weight"]
    assert torch.equal(got["flat_ema"][o:o + n].view(-1), av["module.final_fc.1.weight"].reshape(-1))
    assert torch.equal(got["flat_p"][o:o + n].view(-1), sd["module.final_fc.1.weight"].reshape(-1))
