"""The per-step learning-rate schedule of the fused step (dpc_step_advance_sched / dpc_adam_dev_sched / dpc_adam_groups_dev_sched in
csrc/loss.hip, BackboneEngine.set_lr_schedule / lr_now, the checkpoint's 'lr_schedule' entry, optim.LRSchedule / lr_multiplier /
Adam(lr_schedule=), the entries' --lr_schedule flags), shared by the CPU tier (host SIMT simulator, tests/test_lr_schedule_emu.py)
and the GPU tier (tests/test_lr_schedule_gpu.py).

The step after k completed optimizer steps uses lr_group * mult(k); mult is formed in double and rounded to f32 once, the product
lr * mult is one f32 multiplication.  Bounds, all from the number formats:
  mult, no transcendental : bit-identical to float32(optim.lr_multiplier(k)) -- both sides perform the same double operations one by
                            one (warm-up with W a power of two, linear with T - W a power of two and multistep with gamma = 0.5 are
                            exact in double anyway), then the same single rounding
  mult, cosine            : one f32 ulp -- the device's and the host's double cos may differ in the last double bit, which moves the
                            single rounding to f32 by at most one step; x = 0 and x >= 1 take no cos-dependent value and are exact
  step, bias_corr         : bit-identical to dpc_step_advance on a twin
  p / m / v (/ ema)       : mult = 1 -> bit-identical to the _ex / _ema entries; mult = 0.25 -> bit-identical to the _ex entry given
                            lr * 0.25 (a power of two commutes with the rounding); mult = 0.3 -> adam_groups_cases' bounds, p's widened
                            by 2^-24 of the step taken (one more rounding of the step size)
  engine                  : bit-identical to a twin whose host writes float(f32(lr)) * float(f32(mult(k))) into eng.lr / the table before
                            each step: the double product of two f32 values is exact, and its conversion to f32 is the rounding of the
                            kernel's f32 multiply
"""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
import torch

import adam_groups_cases as ac
import ema_cases as ec
import grad_guard_cases as gc
from dpc_amd import _lib as L
from dpc_amd.optim import LRSchedule, lr_multiplier
from kcases import K

B1, B2, EPS = ac.B1, ac.B2, ac.EPS
BIG = ec.BIG
same = ec.same
new_state = gc.new_state
SENTINEL = dict(mult=-7.5, k=-12345)


def f32(x) -> float:
    return float(np.float32(x))


def ulps(a: float, b: float) -> int:
    """distance of two positive f32 values in units of the last place"""
    ia, ib = (int(np.float32(v).view(np.int32)) for v in (a, b))
    return abs(ia - ib)


def new_record(dev: K, **fields):
    return dev.t(torch.frombuffer(bytearray(bytes(L.LrState(**fields))), dtype=torch.uint8).clone())


def read_record(k: K, rec) -> L.LrState:
    k.sync()
    return L.LrState.from_buffer_copy(rec.cpu().numpy().tobytes())


def advance(k: K, sched, at: int, state=None, record=None):
    """dpc_step_advance_sched with dev_step preset to `at`; returns (step, bias_corr, record) on the device"""
    step, bc = ec.step_at(k, at), k.t(torch.full((2,), -1.0))
    record = new_record(k, **SENTINEL) if record is None else record
    desc = sched.descriptor() if isinstance(sched, LRSchedule) else sched
    k.call("dpc_step_advance_sched", step, bc, B1, B2, state, C.byref(desc) if desc is not None else None, record)
    k.sync()
    return step, bc, record


# ------------------------------------------------------------------ case 1
W, T = 4, 20          # W and T - W powers of two
TABLE = (
    LRSchedule("constant"),
    LRSchedule("constant", warmup_steps=W),
    LRSchedule("cosine", warmup_steps=W, total_steps=T, min_mult=0.1),
    LRSchedule("cosine", warmup_steps=0, total_steps=T),
    LRSchedule("cosine", warmup_steps=3, total_steps=17, min_mult=0.05),      # nothing a power of two: still the same operations
    LRSchedule("linear", warmup_steps=W, total_steps=T, min_mult=0.25),
    LRSchedule("linear", warmup_steps=0, total_steps=16),
    LRSchedule("multistep", warmup_steps=W, milestones=(6, 7, 12), gamma=0.5),
    LRSchedule("multistep", milestones=(0, 3, 5, 8, 13, 21, 34, 55), gamma=0.5),   # the table full, a milestone at step 0
)


def edges(s: LRSchedule):
    ks = {0, s.warmup_steps - 1, s.warmup_steps, s.warmup_steps + 1}
    if s.kind in ("cosine", "linear"):
        ks |= {s.total_steps - 1, s.total_steps, s.total_steps + 5, (s.warmup_steps + s.total_steps) // 2}
    for m in s.milestones:
        ks |= {m - 1, m, m + 1}
    return sorted(k for k in ks if k >= 0)


def case_multiplier_table(k: K, report=print):
    worst = 0
    for s in TABLE:
        for at in edges(s):
            step, bc, rec = advance(k, s, at)
            twin_step, twin_bc = ec.step_at(k, at), k.t(torch.full((2,), -1.0))
            k.call("dpc_step_advance", twin_step, twin_bc, B1, B2)
            k.sync()
            assert int(step.cpu()) == at + 1 and same(step.cpu(), twin_step.cpu()) and same(bc.cpu(), twin_bc.cpu())
            r = read_record(k, rec)
            want = f32(lr_multiplier(at, s))
            assert r.k == at and tuple(r.reserved) == (0, 0)
            x = (at - s.warmup_steps) / (s.total_steps - s.warmup_steps) if s.kind == "cosine" else None
            if s.kind == "cosine" and at >= s.warmup_steps and 0.0 < x < 1.0:
                d = ulps(r.mult, want)
                worst = max(worst, d)
                assert d <= 1, (s, at, r.mult, want)
            else:
                assert np.float32(r.mult).view(np.int32) == np.float32(want).view(np.int32), (s, at, r.mult, want)
            if s.kind in ("cosine", "linear") and at >= s.total_steps:
                assert r.mult == f32(s.min_mult)
            if s.kind in ("cosine", "linear") and at == s.warmup_steps:
                assert r.mult == f32(s.min_mult + (1.0 - s.min_mult))      # x = 0
    report(f"cosine multipliers: worst distance to the host statement {worst} ulp")
    # the values themselves, from the definition
    assert [f32(lr_multiplier(i, TABLE[1])) for i in range(6)] == [0.25, 0.5, 0.75, 1.0, 1.0, 1.0]
    assert [lr_multiplier(i, TABLE[7]) for i in (5, 6, 7, 11, 12, 500)] == [1.0, 0.5, 0.25, 0.25, 0.125, 0.125]
    assert lr_multiplier(12, TABLE[5]) == 0.25 + 0.75 * 0.5 and lr_multiplier(0, TABLE[8]) == 0.5
    assert abs(lr_multiplier(12, TABLE[2]) - (0.1 + 0.9 * 0.5)) < 1e-15      # cos(pi / 2)
    # with the guard's record: skip = 0 advances as dpc_step_advance_gated does, skip = 1 leaves everything bit-still
    s = TABLE[2]
    go, stop = new_state(k, coef=1.0), new_state(k, coef=0.0, skip=1)
    step, bc, rec = advance(k, s, 7, state=go)
    twin_step, twin_bc = ec.step_at(k, 7), k.t(torch.full((2,), -1.0))
    k.call("dpc_step_advance_gated", twin_step, twin_bc, B1, B2, go)
    k.sync()
    assert same(step.cpu(), twin_step.cpu()) and same(bc.cpu(), twin_bc.cpu()) and read_record(k, rec).k == 7
    step, bc, rec = advance(k, s, 7, state=stop)
    r = read_record(k, rec)
    assert int(step.cpu()) == 7 and same(bc.cpu(), torch.full((2,), -1.0)) and (r.mult, r.k) == (SENTINEL["mult"], SENTINEL["k"])
    assert C.sizeof(L.LrState) == 16 and C.sizeof(L.LrSchedule) == 64


# ------------------------------------------------------------------ cases 2 - 4: the update
def run_plain(k: K, arenas, lr, wd, bc, gscale, rec, state=None, ema=None, step=None, decay=0.0):
    """dpc_adam_dev_sched on device copies; returns the host copies [p, g, m, v(, ema)]"""
    dev = [k.t(t.clone()) for t in arenas] + ([k.t(ema.clone())] if ema is not None else [])
    n = arenas[0].numel()
    k.call("dpc_adam_dev_sched", *dev[:4], n, lr, B1, B2, EPS, wd, bc, gscale, state, dev[4] if ema is not None else None,
           step if ema is not None else None, decay, rec)
    k.sync()
    return [t.cpu() for t in dev]


def run_groups(k: K, arenas, tab, nseg, bc, gscale, rec, state=None, ema=None, step=None, decay=0.0):
    dev = [k.t(t.clone()) for t in arenas] + ([k.t(ema.clone())] if ema is not None else [])
    n = arenas[0].numel()
    k.call("dpc_adam_groups_dev_sched", *dev[:4], n, tab, nseg, B1, B2, EPS, bc, gscale, state, dev[4] if ema is not None else None,
           step if ema is not None else None, decay, rec)
    k.sync()
    return [t.cpu() for t in dev]


def all_same(a, b):
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


TILE_SPLIT = 8192 * 256 * 4 + 8      # a segment boundary inside the second sweep, 16-byte aligned, not on a tile boundary


def case_identity(k: K):
    """mult = 1.0f: the bits of the _ex and _ema entries, plain and groups, over more floats than one sweep of either kernel covers"""
    n = BIG
    p0, g0, m0, v0, e0 = ec.random_arenas(n, seed=41)
    four = (p0, g0, m0, v0)
    bc, step, one = ec.bias_corr(k), ec.step_at(k, 1000), new_record(k, mult=1.0, k=999)
    lr, wd = 1e-2, 1e-5
    assert all_same(run_plain(k, four, lr, wd, bc, 0.5, one), ec.run_plain(k, four, lr, wd, bc, 0.5))
    assert all_same(run_plain(k, four, lr, wd, bc, 0.5, one, None, e0, step, 0.9), ec.run_plain(k, four, lr, wd, bc, 0.5, None, e0, step, 0.9))
    tab = ac.table(k, [(0, TILE_SPLIT, lr, wd, 1), (TILE_SPLIT, n, lr / 8, 0.0, 1)])
    got = run_groups(k, four, tab, 2, bc, 0.5, one)
    assert all_same(got, ec.run_groups(k, four, tab, 2, bc, 0.5)) and not same(got[0][-8:], p0[-8:])
    assert all_same(run_groups(k, four, tab, 2, bc, 0.5, one, None, e0, step, 0.9), ec.run_groups(k, four, tab, 2, bc, 0.5, None, e0, step, 0.9))
    # the guard's record goes through as in the _ex entries
    quarter = new_state(k, coef=0.25)
    assert all_same(run_plain(k, four, lr, wd, bc, 0.5, one, quarter), ec.run_plain(k, four, lr, wd, bc, 0.5, quarter))
    rec = read_record(k, one)
    assert (rec.mult, rec.k) == (1.0, 999)      # the record is only read


def case_scaling_exact(k: K):
    """mult = 0.25: the f32 product lr * 0.25 is exact, so the _ex entry given lr * 0.25 must give the same bits"""
    bc, rec = ec.bias_corr(k), new_record(k, mult=0.25, k=3)
    segs, n, sp = ac.layout()
    p0, g0, m0, v0, e0 = ec.random_arenas(n, seed=42)
    four = (p0, g0, m0, v0)
    lr, wd = 1e-2, 1e-5
    got = run_plain(k, four, lr, wd, bc, 0.5, rec)
    assert all_same(got, ec.run_plain(k, four, f32(lr) * 0.25, wd, bc, 0.5))
    assert not same(got[0], ec.run_plain(k, four, lr, wd, bc, 0.5)[0])          # ... and it did scale
    tab = ac.table(k, segs)
    pre = ac.table(k, [(b, e, f32(s_lr) * 0.25, s_wd, a) for b, e, s_lr, s_wd, a in segs])
    got = run_groups(k, four, tab, len(segs), bc, 0.5, rec)
    assert all_same(got, ec.run_groups(k, four, pre, len(segs), bc, 0.5))
    assert not same(got[0], ec.run_groups(k, four, tab, len(segs), bc, 0.5)[0])
    step = ec.step_at(k, 50)
    assert all_same(run_groups(k, four, tab, len(segs), bc, 0.5, rec, None, e0, step, 0.9),
                    ec.run_groups(k, four, pre, len(segs), bc, 0.5, None, e0, step, 0.9))
    # a length that is no multiple of four: the scalar tail of adam_dev_kernel
    q = [t[:4 * 300 + 3].clone() for t in four]
    assert all_same(run_plain(k, q, lr, wd, bc, 0.5, rec), ec.run_plain(k, q, f32(lr) * 0.25, wd, bc, 0.5))


def case_scaling_rounding(k: K, report=print):
    """mult = 0.3 against the f64 Adam of adam_groups_cases; frozen segment and gap planted with NaN / Inf; the lr = 0 segment"""
    mult = f32(0.3)
    rec = new_record(k, mult=mult, k=9)
    segs, n, sp = ac.layout()
    p0, g0, m0, v0, _ = ec.random_arenas(n, seed=11)
    fb, fe = segs[sp["frozen"]][:2]
    ga, gb = sp["gap"]
    planted = [t.clone() for t in (p0, g0, m0, v0)]
    for t in planted:
        t[fb:fe] = float("nan")
        t[ga:gb] = float("inf")
    step, bc = ec.step_at(k, 2), k.t(torch.ones(2))
    k.call("dpc_step_advance", step, bc, B1, B2)
    k.sync()
    bc_h = bc.cpu()
    gscale = 0.5
    p, g, m, v = run_groups(k, planted, ac.table(k, segs), len(segs), bc, gscale, rec)
    lr_e, wd_e, act = torch.zeros(n), torch.zeros(n), torch.zeros(n, dtype=torch.bool)
    for b, e, lr, wd, a in segs:
        lr_e[b:e], wd_e[b:e], act[b:e] = lr, wd, bool(a)
    zero = torch.zeros(())
    pz, gz, mz, vz = (torch.where(act, t, zero) for t in planted)   # the reference never looks at what a frozen segment or the gap hold
    p2, m2, v2, bm, bv = ac.adam_f64(pz, gz, mz, vz, lr_e.double() * mult, wd_e, bc_h, gscale)
    bp = 1e-7 * max(1.0, p0.abs().max().item()) + 2.0 ** -24 * (p2 - pz.double()).abs()   # one more f32 rounding of the step size
    ep = ((p.double() - p2.float().double()).abs() / bp)[act].max().item()
    em = ((m.double() - m2.float().double()).abs() / bm)[act].max().item()
    ev = ((v.double() - v2.float().double()).abs() / bv)[act].max().item()
    report(f"scheduled groups, mult 0.3, vs f64: p {ep:.3g}, m {em:.3g}, v {ev:.3g} of their bounds")
    assert ep <= 1.0 and em <= 1.0 and ev <= 1.0
    # ... and the bound tells mult = 0.3 from mult = 1: the unscaled reference is far outside it for most live elements
    p_unscaled = ac.adam_f64(pz, gz, mz, vz, lr_e, wd_e, bc_h, gscale)[0]
    live = act & (lr_e > 0)
    assert (((p.double() - p_unscaled).abs() > 2 * bp)[live]).float().mean().item() > 0.9
    for new, old in zip((p, g, m, v), planted):
        assert same(new[~act], old[~act])
    assert torch.isnan(p[fb:fe]).all() and torch.isinf(p[ga:gb]).all() and torch.isfinite(p[act]).all()
    zb, ze = segs[sp["lr0"]][:2]
    assert same(p[zb:ze], p0[zb:ze]) and not same(m[zb:ze], m0[zb:ze]) and not same(v[zb:ze], v0[zb:ze])
    # the one-group entry, same reference
    p, g, m, v = run_plain(k, (p0, g0, m0, v0), 1e-3, 1e-5, bc, gscale, rec)
    lr1 = torch.full((n,), 1e-3)
    p2, m2, v2, bm, bv = ac.adam_f64(p0, g0, m0, v0, lr1.double() * mult, torch.full((n,), 1e-5), bc_h, gscale)
    bp = 1e-7 * max(1.0, p0.abs().max().item()) + 2.0 ** -24 * (p2 - p0.double()).abs()
    ep = ((p.double() - p2.float().double()).abs() / bp).max().item()
    em, ev = ((m.double() - m2.float().double()).abs() / bm).max().item(), ((v.double() - v2.float().double()).abs() / bv).max().item()
    report(f"scheduled one-group, mult 0.3, vs f64: p {ep:.3g}, m {em:.3g}, v {ev:.3g} of their bounds")
    assert ep <= 1.0 and em <= 1.0 and ev <= 1.0


# ------------------------------------------------------------------ case 5
def raw_desc(kind=L.LR_COSINE, warmup=2, total=10, min_mult=0.0, gamma=0.5, milestones=()):
    d = L.LrSchedule(kind=kind, warmup_steps=warmup, total_steps=total, n_milestones=len(milestones), min_mult=min_mult, gamma=gamma)
    for i, m in enumerate(milestones[:L.LR_MAX_MILESTONES]):
        d.milestones[i] = m
    return d


def case_argument_checks(k: K):
    MS = L.LR_MULTISTEP
    nine = raw_desc(MS, milestones=tuple(range(1, 9)))
    nine.n_milestones = 9
    bad_descs = [
        raw_desc(kind=4), raw_desc(kind=-1),
        raw_desc(L.LR_COSINE, warmup=10, total=10), raw_desc(L.LR_LINEAR, warmup=10, total=10), raw_desc(L.LR_COSINE, warmup=10, total=4),
        raw_desc(MS, milestones=(5, 5)), raw_desc(MS, milestones=(7, 3)), raw_desc(MS, milestones=(-1, 3)), nine,
        raw_desc(MS, gamma=0.0, milestones=(3,)), raw_desc(MS, gamma=1.5, milestones=(3,)), raw_desc(MS, gamma=-0.5, milestones=(3,)),
        raw_desc(MS, gamma=float("nan"), milestones=(3,)),
        raw_desc(L.LR_COSINE, min_mult=-0.1), raw_desc(L.LR_LINEAR, min_mult=1.5), raw_desc(L.LR_COSINE, min_mult=float("nan")),
        raw_desc(L.LR_CONSTANT, warmup=-1), raw_desc(L.LR_COSINE, warmup=-1),
    ]
    for d in bad_descs:
        step, bc, rec = ec.step_at(k, 7), k.t(torch.full((2,), -1.0)), new_record(k, **SENTINEL)
        with pytest.raises(L.DpcError, match=f"code {L.ERR_ARG}$"):
            k.call("dpc_step_advance_sched", step, bc, B1, B2, None, C.byref(d), rec)
        k.sync()
        r = read_record(k, rec)
        assert int(step.cpu()) == 7 and same(bc.cpu(), torch.full((2,), -1.0)) and (r.mult, r.k) == (SENTINEL["mult"], SENTINEL["k"])
    good = raw_desc()
    step, bc, rec = ec.step_at(k, 7), k.t(torch.full((2,), -1.0)), new_record(k, **SENTINEL)
    for args in ((step, bc, B1, B2, None, C.byref(good), None), (step, bc, B1, B2, None, None, rec), (None, bc, B1, B2, None, C.byref(good), rec),
                 (step, None, B1, B2, None, C.byref(good), rec)):
        with pytest.raises(L.DpcError, match=f"code {L.ERR_ARG}$"):
            k.call("dpc_step_advance_sched", *args)
    assert int(step.cpu()) == 7
    # the same conditions, refused where the schedule is built
    for kw in (dict(kind="exponential"), dict(kind="cosine", warmup_steps=10, total_steps=10), dict(kind="linear", total_steps=0),
               dict(kind="multistep", milestones=(5, 5)), dict(kind="multistep", milestones=tuple(range(9))),
               dict(kind="multistep", milestones=(3,), gamma=0.0), dict(kind="multistep", milestones=(3,), gamma=1.5),
               dict(kind="cosine", total_steps=10, min_mult=-0.1), dict(kind="cosine", total_steps=10, min_mult=1.5), dict(warmup_steps=-1)):
        with pytest.raises(ValueError):
            LRSchedule(**kw)
    # the two updates: a null record; an average without its counter; the arenas keep every bit
    segs, n, _ = ac.layout()
    tab, S = ac.table(k, segs), len(segs)
    host = ec.random_arenas(n + 4, seed=43)
    dev = [k.t(t.clone()) for t in host]
    four, ema = dev[:4], dev[4]
    bc, st, one = ec.bias_corr(k), ec.step_at(k, 5), new_record(k, mult=1.0, k=4)
    plain = lambda p=four[0], e=None, s=None, d=0.0, r=one: k.call(   # noqa: E731
        "dpc_adam_dev_sched", p, *four[1:], n, 1e-3, B1, B2, EPS, 0.0, bc, 1.0, None, e, s, d, r)
    groups = lambda p=four[0], e=None, s=None, d=0.0, r=one, nn=n, ns=S, tb=tab: k.call(   # noqa: E731
        "dpc_adam_groups_dev_sched", p, *four[1:], nn, tb, ns, B1, B2, EPS, bc, 1.0, None, e, s, d, r)
    bad = [lambda: plain(r=None), lambda: plain(p=None), lambda: plain(e=ema), lambda: plain(s=st), lambda: plain(e=ema, s=st, d=1.0),
           lambda: plain(e=four[0], s=st, d=0.9), lambda: plain(e=ema[1:], s=st, d=0.9),
           lambda: groups(r=None), lambda: groups(e=ema), lambda: groups(s=st), lambda: groups(e=ema, s=st, d=0.0), lambda: groups(nn=n + 2),
           lambda: groups(ns=0), lambda: groups(tb=None), lambda: groups(p=four[0][1:])]
    for f in bad:
        with pytest.raises(L.DpcError, match=f"code {L.ERR_ARG}$"):
            f()
    k.sync()
    assert all_same([t.cpu() for t in dev], list(host))
    plain()
    groups(e=ema, s=st, d=0.9)
    k.sync()
    assert not same(four[0].cpu(), host[0]) and not same(ema.cpu(), host[4])


# ====================================================================== engine, checkpoints, module boundary, entries
Cfg = gc.Cfg
dpc_engine, dpc_input, lc_engine = gc.dpc_engine, gc.dpc_input, gc.lc_engine
arenas, same_bits = gc.arenas, gc.same_bits
SCHED = LRSchedule("cosine", warmup_steps=2, total_steps=5)     # five steps: 1/2, 1, then cos at x = 0, 1/3, 2/3
STEPS = 5
DECAY = 0.9
_RUNS = {}


def host_lr(base: float, k: int, sched: LRSchedule = SCHED) -> float:
    """what a host-driven twin writes before the step after k completed ones: exact in double, rounded where it is stored as f32"""
    return f32(base) * f32(lr_multiplier(k, sched))


def sched_run(cfg: Cfg, dtype, ema: bool = False):
    """STEPS train steps of the one-group DPC engine under SCHED, computed once: after each step the arenas (and flat_ema), lr_now() and
    the launches; after the second the checkpoint dictionary"""
    from dpc_amd import checkpoint as ckpt
    key = ("sched", cfg.device, tuple(cfg.widths), dtype, ema)
    if key not in _RUNS:
        eng, x = dpc_engine(cfg, dtype), dpc_input(cfg)
        if ema:
            eng.set_ema(DECAY)
        eng.set_lr_schedule(SCHED)
        assert eng.lr_now() == {"mult": 1.0, "k": -1, "lr": f32(eng.lr)}
        rec = {"steps": [], "lr": eng.lr}
        for i in range(STEPS):
            n0 = eng._launches
            eng.train_step(x)
            rec["steps"].append({"arenas": arenas(eng), "ema": eng.flat_ema.detach().clone() if ema else None, "now": eng.lr_now(),
                                 "launches": eng._launches - n0, "last": L.last_kernel(eng.lib)})
            if i == 1:
                rec["state2"] = ckpt.build_state(eng, 1, "resnet18", 0.0, 2)
        assert eng.lr == rec["lr"]     # the base value: the schedule never writes it
        _RUNS[key] = rec
    return _RUNS[key]


def host_twin(cfg: Cfg, dtype, ema: bool = False):
    """the same steps with no schedule: the host writes eng.lr before each"""
    key = ("twin", cfg.device, tuple(cfg.widths), dtype, ema)
    if key not in _RUNS:
        eng, x = dpc_engine(cfg, dtype), dpc_input(cfg)
        if ema:
            eng.set_ema(DECAY)
        base, rec = eng.lr, {"steps": []}
        for i in range(STEPS):
            eng.lr = host_lr(base, i)
            n0 = eng._launches
            eng.train_step(x)
            rec["steps"].append({"arenas": arenas(eng), "ema": eng.flat_ema.detach().clone() if ema else None,
                                 "launches": eng._launches - n0, "last": L.last_kernel(eng.lib)})
        assert eng.lr_schedule is None and eng._lr_state is None      # off: nothing allocated
        _RUNS[key] = rec
    return _RUNS[key]


def case_off_is_off(cfg: Cfg, dtype=torch.float32):   # case 6
    x = dpc_input(cfg)
    a, b = dpc_engine(cfg, dtype), dpc_engine(cfg, dtype)
    base = b._baked_scalars()
    b.set_lr_schedule(LRSchedule("constant"))
    assert b._baked_scalars()[:-1] == base and b._baked_scalars()[-1][0] == "lr_schedule" and a._baked_scalars() == base
    for i in range(2):
        na, nb = a._launches, b._launches
        a.train_step(x)
        b.train_step(x)
        assert a._launches - na == b._launches - nb
        assert same_bits(arenas(a), arenas(b))
        assert b.lr_now() == {"mult": 1.0, "k": i, "lr": f32(b.lr)}
    assert not torch.equal(a.flat_p, dpc_engine(cfg, dtype).flat_p)
    # off after having been on: the key and the entry of an engine that never had one
    b.set_lr_schedule(None)
    assert b.lr_schedule is None and b._baked_scalars() == base
    b.adam_step()
    last_b = L.last_kernel(b.lib)
    a.adam_step()
    assert last_b == L.last_kernel(a.lib) and last_b.startswith("adam_dev_kernel<false>")
    assert same_bits(arenas(a), arenas(b)) and b.lr_now()["k"] == 1
    with pytest.raises(RuntimeError, match="never enabled"):
        a.lr_now()


def case_host_driven_twin(cfg: Cfg, dtype=torch.float32, report=print):   # case 7, the one-group DPC engine
    run, ref = sched_run(cfg, dtype), host_twin(cfg, dtype)
    for i, (s, t) in enumerate(zip(run["steps"], ref["steps"])):
        assert same_bits(s["arenas"], t["arenas"]), f"step {i + 1}"
        assert s["launches"] == t["launches"]                                       # no launch of its own
        assert s["last"].startswith("adam_dev_sched_kernel<false>") and t["last"].startswith("adam_dev_kernel<false>"), (s["last"], t["last"])
        want = f32(lr_multiplier(i, SCHED))
        assert s["now"]["k"] == i and ulps(s["now"]["mult"], want) <= (1 if i > 2 else 0)
        assert s["now"]["lr"] == f32(f32(run["lr"]) * s["now"]["mult"])
        assert int(s["arenas"][3].item()) == i + 1
    mults = [s["now"]["mult"] for s in run["steps"]]
    report(f"multipliers of the five steps: {mults}")
    assert mults[:3] == [0.5, 1.0, 1.0] and 0.74 < mults[3] < 0.76 and 0.24 < mults[4] < 0.26
    assert not same_bits(run["steps"][0]["arenas"][:1], run["steps"][1]["arenas"][:1])


def lc_groups(eng, lr_head=1e-3, lr_backbone=1e-4):
    """lc_main --train_what ft: the head at lr, the backbone at a tenth, the aggregator frozen"""
    head = [k for k in eng.offsets if k.startswith(("final_bn.", "final_fc."))]
    backbone = [k for k in eng.offsets if k.startswith("backbone.")]
    return lambda mult=1.0: [{"params": head, "lr": f32(lr_head) * mult, "weight_decay": 1e-3},
                             {"params": backbone, "lr": f32(lr_backbone) * mult, "weight_decay": 1e-3}]


def case_host_driven_twin_groups(cfg: Cfg, num_class: int = 11, dtype=torch.float32):   # case 7, LC with two groups
    x = dpc_input(cfg)
    target = (torch.arange(cfg.B) % num_class).to(cfg.device)

    def make():
        from dpc_amd.lc import LCEngine
        from oracle import dpc_oracle as O
        eng = LCEngine("resnet18", cfg.size, cfg.N, cfg.SL, cfg.B, cfg.device, dtype, cfg.widths, lib=cfg.simulator, num_class=num_class)
        eng.load_params(O.make_lc_params_pcg("resnet18", num_class, cfg.widths))
        return eng

    a, b = make(), make()
    ga, gb = lc_groups(a), lc_groups(b)
    a.set_param_groups(ga())
    a.set_lr_schedule(SCHED)
    frozen = a.offsets["agg.cell_list.0.update_gate.weight"] if "agg.cell_list.0.update_gate.weight" in a.offsets else None
    p0 = a.flat_p.detach().clone()
    for i in range(STEPS):
        b.set_param_groups(gb(f32(lr_multiplier(i, SCHED))))
        na, nb = a._launches, b._launches
        a.train_step(x, target)
        last_a = L.last_kernel(a.lib)      # (the trace belongs to the library, which both engines share)
        b.train_step(x, target)
        assert same_bits(arenas(a), arenas(b)), f"step {i + 1}"
        assert a._launches - na == b._launches - nb
        assert "adam_groups_sched_kernel<false>" in last_a and "adam_groups_kernel<false>" in L.last_kernel(b.lib)
    assert a.seg_uploads == 1 and b.seg_uploads >= 3       # the schedule never touches the table; the host-driven twin re-uploads it
    assert a.param_groups[0]["lr"] == f32(1e-3) and a.lr_now()["k"] == STEPS - 1
    if frozen is not None:
        o, n = frozen
        assert same_bits([a.flat_p[o:o + n]], [p0[o:o + n]])
    o, n = a.offsets["final_fc.1.weight"]
    assert not torch.equal(a.flat_p[o:o + n], p0[o:o + n])


def case_with_the_guard(cfg: Cfg, dtype=torch.float32):   # case 8
    eng, x = dpc_engine(cfg, dtype), dpc_input(cfg)
    eng.set_grad_guard(skip_nonfinite=True)
    eng.set_lr_schedule(SCHED)
    twin = dpc_engine(cfg, dtype)
    twin.set_grad_guard(skip_nonfinite=True)
    eng._forward_loss(x, True)
    eng.backward()
    g = eng.flat_g.detach().clone()
    o, _ = eng.offsets["backbone.layer2.0.conv1.weight"]
    before = arenas(eng) + [eng._lr_state.detach().clone()]
    eng.flat_g[o + 5] = float("nan")
    eng.adam_step()
    assert eng.grad_stats()["skip"] == 1
    assert same_bits(arenas(eng), before[:-1]) and torch.equal(eng._lr_state, before[-1]) and eng.lr_now()["k"] == -1
    assert eng.step_count == 0
    # the next clean step is the step the skipped one would have been: k = 0
    eng.flat_g.copy_(g)
    eng.adam_step()
    assert eng.lr_now() == {"mult": 0.5, "k": 0, "lr": f32(f32(eng.lr) * 0.5)} and eng.step_count == 1
    twin.flat_g.copy_(g)
    twin.lr = host_lr(twin.lr, 0)
    twin.adam_step()
    assert same_bits(arenas(eng), arenas(twin)) and not same_bits(arenas(eng)[:1], before[:1])


def case_with_ema(cfg: Cfg, dtype=torch.float32):   # case 9
    run, ref = sched_run(cfg, dtype, ema=True), host_twin(cfg, dtype, ema=True)
    for i, (s, t) in enumerate(zip(run["steps"], ref["steps"])):
        assert same_bits(s["arenas"] + [s["ema"]], t["arenas"] + [t["ema"]]), f"step {i + 1}"
        assert s["launches"] == t["launches"] and "adam_dev_sched_kernel<true>" in s["last"] and "adam_dev_kernel<true>" in t["last"]
    assert not torch.equal(run["steps"][-1]["ema"], run["steps"][-1]["arenas"][0])


def case_checkpoint(cfg: Cfg, tmp_path, dtype=torch.float32):   # case 10
    from dpc_amd import checkpoint as ckpt
    run = sched_run(cfg, dtype)
    x = dpc_input(cfg)
    state = run["state2"]
    assert state["lr_schedule"] == {"kind": "cosine", "warmup_steps": 2, "total_steps": 5, "min_mult": 0.0}
    assert state["optimizer"]["param_groups"][0]["lr"] == run["lr"]          # the BASE lr: the reference resumes the file as before
    assert "ema" not in state
    fn = str(tmp_path / "epoch1.pth.tar")
    ckpt.save_checkpoint(state, filename=fn)
    b = dpc_engine(cfg, dtype)
    b.set_lr_schedule(SCHED)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        info = ckpt.resume(b, fn)
    assert info["epoch"] == 1 and same_bits(arenas(b)[:4], run["steps"][1]["arenas"][:4]) and b.lr == run["lr"]
    b.train_step(x)
    assert same_bits(arenas(b), run["steps"][2]["arenas"])
    assert b.lr_now() == run["steps"][2]["now"] and b.lr_now()["k"] == 2
    # another schedule at resume: one warning, and the caller's schedule stays
    c = dpc_engine(cfg, dtype)
    other = LRSchedule("linear", warmup_steps=2, total_steps=5)
    c.set_lr_schedule(other)
    with pytest.warns(UserWarning, match="learning-rate schedule") as rec:
        ckpt.resume(c, fn)
    assert len([w for w in rec if "learning-rate schedule" in str(w.message)]) == 1 and c.lr_schedule == other
    d = dpc_engine(cfg, dtype)
    with pytest.warns(UserWarning, match="learning-rate schedule"):
        ckpt.resume(d, fn)
    assert d.lr_schedule is None and "lr_schedule" not in ckpt.build_state(d, 1, "resnet18", 0.0, 2)
    # a file written without the entry: silent, with the schedule on or off
    fn2 = str(tmp_path / "plain.pth.tar")
    ckpt.save_checkpoint({k: v for k, v in state.items() if k != "lr_schedule"}, filename=fn2)
    for e in (b, d):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            ckpt.resume(e, fn2)
    # adopt_optimizer_state carries the schedule and its record
    f = dpc_engine(cfg, dtype)
    f.load_params(b.state_dict())
    f.adopt_optimizer_state(b)
    assert f.lr_schedule == SCHED and f._baked_scalars() == b._baked_scalars() and f._lr_state.data_ptr() != b._lr_state.data_ptr()


def case_captured_step(cfg: Cfg, dtype=torch.float32):   # case 11, HIP device only
    x = dpc_input(cfg)
    sched = LRSchedule("cosine", warmup_steps=4, total_steps=9, min_mult=0.1)     # two eager steps, then four replays: k = 2 .. 5
    a, b = dpc_engine(cfg, dtype), dpc_engine(cfg, dtype)
    plain = dpc_engine(cfg, dtype)
    for e in (a, b):
        e.set_lr_schedule(sched)
    for e in (a, b, plain):
        for _ in range(2):   # eager steps size every lazy buffer
            e.train_step(x)
    block = x.clone()
    replay = a.capture_train_step(block, warmup=0)
    ref = plain.capture_train_step(x.clone(), warmup=0)
    assert replay.kernels == ref.kernels                       # the schedule adds no launch to the captured step
    plain.release_captures()
    for i in range(4):
        replay()
        b.train_step(x)
        assert same_bits(arenas(a), arenas(b)), f"replay {i + 1}"
    now = a.lr_now()
    want = f32(lr_multiplier(5, sched))
    assert now["k"] == 5 and ulps(now["mult"], want) <= 1 and now == b.lr_now() and a.step_count == 6 == int(a.dev_step.item())
    assert 0.1 < now["mult"] < 1.0                              # past the warm-up, on the cosine
    a.set_lr_schedule(LRSchedule("cosine", warmup_steps=4, total_steps=10, min_mult=0.1))
    with pytest.raises(RuntimeError, match="changed since"):
        replay()
    a.set_lr_schedule(None)
    with pytest.raises(RuntimeError, match="changed since"):
        replay()
    a.set_lr_schedule(sched)
    replay()
    b.train_step(x)
    assert same_bits(arenas(a), arenas(b))
    a.release_captures()


def case_module_boundary(cfg: Cfg, num_class: int = 11, report=print):   # case 12
    import lc_loop_cases as lc
    from dpc_amd import optim
    c = lc.Cfg(device=cfg.device, simulator=cfg.simulator, widths=cfg.widths, num_class=num_class, size=cfg.size, B=cfg.B, N=cfg.N, SL=cfg.SL)
    forced, _ = lc.masks(c)
    x = dpc_input(cfg)
    target = (torch.arange(cfg.B) % num_class).to(cfg.device).view(cfg.B, 1)
    crit = torch.nn.CrossEntropyLoss()
    sched = LRSchedule("cosine", warmup_steps=0, total_steps=3, min_mult=0.2)    # two steps: 1, then 0.2 + 0.8 * 0.75 = 0.8
    ma, mb = lc.module(c), lc.module(c)
    for m in (ma, mb):
        m._forced_masks = forced
    oa = optim.Adam(ma.parameters(), lr=1e-3, weight_decay=1e-3, lr_schedule=sched)
    ob = torch.optim.Adam(mb.parameters(), lr=1e-3, weight_decay=1e-3)
    sb = torch.optim.lr_scheduler.LambdaLR(ob, lr_lambda=lambda k: lr_multiplier(k, sched))
    for i in range(2):
        lc.ref_loop_step(ma, oa, x, target, crit)
        lc.ref_loop_step(mb, ob, x, target, crit)
        sb.step()
        lc.assert_params_agree(ma, mb, f"step {i + 1}")
        now = ma.engine.lr_now()
        assert now["k"] == i and ulps(now["mult"], f32(lr_multiplier(i, sched))) <= 1
        lc.same_start(ma, mb)
    assert abs(ob.param_groups[0]["lr"] - 1e-3 * lr_multiplier(2, sched)) < 1e-18 and oa.param_groups[0]["lr"] == 1e-3   # the base stays
    assert ma.engine.lr_schedule == sched and abs(ma.engine.lr_now()["mult"] - 0.8) < 1e-6
    report(f"module boundary: two scheduled steps agree with torch.optim.Adam + LambdaLR; multiplier now {ma.engine.lr_now()['mult']}")
    with pytest.raises(ValueError):
        optim.Adam(ma.parameters(), lr_schedule="cosine")


# ---------------------------------------------------------------------- entries (simulator)
COMMON = ["--net", "resnet18", "--img_dim", "64", "--batch_size", "1", "--gpu", "0", "--print_freq", "1", "--dtype", "bf16", "--num_seq", "4"]
LR_TAIL = re.compile(r" lr (\d\.\d{3}e[-+]\d\d)$")


def printed_lrs(out: str):
    lines = [ln for ln in out.splitlines() if ln.startswith("Epoch: [")]
    tails = [LR_TAIL.search(ln) for ln in lines]
    assert lines and all(tails), out
    return [t.group(1) for t in tails]


def case_entry_main(emu, widths, capsys, tmp_path):   # case 13, dpc_amd.main
    from dpc_amd import main as dpc_main
    d = str(tmp_path / "run")
    argv = COMMON + ["--pred_step", "1", "--synthetic", "2", "--epochs", "2", "--lr", "1e-3", "--save_dir", d]
    dpc_main.main(argv + ["--lr_schedule", "cosine", "--warmup_steps", "2", "--skip_nonfinite"], _simulator=emu, _widths=widths)
    out = capsys.readouterr().out
    sched = LRSchedule("cosine", warmup_steps=2, total_steps=4)     # --total_steps defaults to epochs x steps per epoch
    assert out.count("LR schedule: cosine, warmup_steps 2, total_steps 4, min_mult 0.0\n") == 1, out
    assert printed_lrs(out) == ["{:.3e}".format(f32(f32(1e-3) * f32(lr_multiplier(k, sched)))) for k in range(4)]
    assert all(re.search(r" gnorm \d+\.\d{4} lr ", ln) for ln in out.splitlines() if ln.startswith("Epoch: ["))   # after gnorm
    ck = torch.load(os.path.join(d, "epoch2.pth.tar"), map_location="cpu", weights_only=False)
    assert ck["lr_schedule"] == sched.to_dict() and ck["optimizer"]["param_groups"][0]["lr"] == 1e-3
    # --resume (no epoch left to run): the same flags are silent, another schedule warns once; the run's own schedule stays
    fn = os.path.join(d, "epoch2.pth.tar")
    for flags, n_warn in ((["--lr_schedule", "cosine", "--warmup_steps", "2"], 0), (["--lr_schedule", "linear", "--warmup_steps", "2"], 1), ([], 1)):
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            dpc_main.main(argv + flags + ["--resume", fn], _simulator=emu, _widths=widths)
        assert len([w for w in rec if "learning-rate schedule" in str(w.message)]) == n_warn, [str(w.message) for w in rec]
        assert "=> loaded resumed checkpoint" in capsys.readouterr().out
    # --warmup_steps alone means constant; without the flags: no line, no tail, no key
    d0 = str(tmp_path / "plain")
    dpc_main.main(COMMON + ["--pred_step", "1", "--synthetic", "1", "--epochs", "1", "--warmup_steps", "4"], _simulator=emu, _widths=widths)
    out = capsys.readouterr().out
    assert "LR schedule: constant, warmup_steps 4\n" in out and printed_lrs(out) == ["2.500e-04"]
    dpc_main.main(COMMON + ["--pred_step", "1", "--synthetic", "1", "--epochs", "1", "--save_dir", d0], _simulator=emu, _widths=widths)
    out = capsys.readouterr().out
    assert "LR schedule" not in out and " lr " not in out and "Epoch: [0][0/1]" in out
    assert "lr_schedule" not in torch.load(os.path.join(d0, "epoch1.pth.tar"), map_location="cpu", weights_only=False)


def case_flag_errors(emu, widths):
    from dpc_amd import entry, lc_main, main as dpc_main
    started = []
    real = entry.launch
    for mod in (dpc_main, lc_main):
        mod.launch = lambda *a, **kw: started.append(a)      # a rank that started would show here
    try:
        for mod, extra in ((dpc_main, ["--pred_step", "1"]), (lc_main, ["--train_what", "head"])):
            base = COMMON + extra + ["--synthetic", "1", "--epochs", "1"]
            for bad in (["--lr_schedule", "cosine", "--warmup_steps", "-1"], ["--lr_schedule", "cosine", "--total_steps", "5", "--warmup_steps", "5"],
                        ["--lr_schedule", "linear", "--lr_min_mult", "1.5"], ["--lr_schedule", "multistep", "--lr_milestones", "5,5"],
                        ["--lr_schedule", "multistep", "--lr_milestones", "1,2,3,4,5,6,7,8,9"], ["--lr_schedule", "multistep", "--lr_milestones", "a,b"],
                        ["--lr_schedule", "multistep", "--lr_milestones", "3", "--lr_gamma", "0"], ["--warmup_steps", "-2"],
                        ["--lr_schedule", "linear", "--total_steps", "-4"],
                        ["--lr_schedule", "cosine", "--warmup_steps", "1"],          # the default end, epochs x steps = 1, is not past the warm-up
                        ["--lr_gamma", "0.5"], ["--lr_milestones", "3"], ["--total_steps", "9"], ["--lr_min_mult", "0.1"]):   # parameters of no schedule
                with pytest.raises(ValueError):
                    mod.main(base + bad, _simulator=emu, _widths=widths)
            with pytest.raises(SystemExit):
                mod.main(base + ["--lr_schedule", "exponential"], _simulator=emu, _widths=widths)
        assert not started
    finally:
        for mod in (dpc_main, lc_main):
            mod.launch = real


def case_two_ranks(emu, widths, tmp_path):
    from dpc_amd import main as dpc_main
    pr = str(tmp_path / "probe")
    os.makedirs(pr)
    dpc_main.main(["--net", "resnet18", "--img_dim", "64", "--batch_size", "2", "--gpu", "0,1", "--synthetic", "2", "--print_freq", "1",
                   "--dtype", "bf16", "--num_seq", "4", "--pred_step", "1", "--epochs", "1", "--lr_schedule", "linear", "--warmup_steps", "1"],
                  _simulator=emu, _widths=widths, _probe=pr)
    r = [torch.load(os.path.join(pr, f"rank{i}.pt")) for i in range(2)]
    assert same(r[0]["flat_p"], r[1]["flat_p"]) and same(r[0]["flat_m"], r[1]["flat_m"])
    assert all(x["step"] == 2 for x in r) and torch.isfinite(r[0]["flat_p"]).all()


def case_entry_lc(emu, widths, capsys, tmp_path, graph: bool = False):
    """case 13, dpc_amd.lc_main: epochs 60 and 61 of the ucf101 / 64 px epoch schedule (milestones 60 / 80 / 100) -- the first runs at lr,
    the second at lr / 10; the per-step multiplier applies on top and goes on counting (with --graph: through the re-capture)"""
    from dpc_amd import lc_main
    d = str(tmp_path / "lc")
    n = 3 if graph else 2       # --graph: the first two train steps of the run are the eager warm-up
    argv = COMMON + ["--synthetic", str(n), "--train_what", "head", "--start-epoch", "60", "--epochs", "62", "--lr", "1e-3", "--save_dir", d,
                     "--lr_schedule", "multistep", "--lr_milestones", "1,3", "--lr_gamma", "0.5"] + (["--graph"] if graph else [])
    lc_main.main(argv, _simulator=emu, _widths=widths)
    out = capsys.readouterr().out
    sched = LRSchedule("multistep", milestones=(1, 3), gamma=0.5)
    assert out.count("LR schedule: multistep, warmup_steps 0, milestones [1, 3], gamma 0.5\n") == 1, out
    lines = [ln for ln in out.splitlines() if ln.startswith("Epoch: [")]
    assert len(lines) == 2 * n
    bases = [float(re.search(r"\t lr (\S+) lr ", ln).group(1)) for ln in lines]      # the log's own column: the epoch schedule's lr
    assert bases == [1e-3] * n + [1e-4] * n, lines
    want = ["{:.3e}".format(f32(f32(b) * f32(lr_multiplier(k, sched)))) for k, b in enumerate(bases)]
    assert printed_lrs(out) == want and want[0] == "1.000e-03" and want[-1] == "2.500e-05"
    if graph:
        assert len(re.findall(r"^Graph replay: (\d+) steps", out, re.M)) == 2      # both epochs replayed: the second on a new capture
    ck = torch.load(os.path.join(d, "epoch62.pth.tar"), map_location="cpu", weights_only=False)
    assert ck["lr_schedule"] == sched.to_dict()
    assert abs(ck["optimizer"]["param_groups"][-1]["lr"] - 1e-4) < 1e-12          # the epoch schedule's lr, not multiplied
    lc_main.main(COMMON + ["--synthetic", "1", "--train_what", "head", "--epochs", "1"], _simulator=emu, _widths=widths)
    out = capsys.readouterr().out
    assert "LR schedule" not in out and not LR_TAIL.search([ln for ln in out.splitlines() if ln.startswith("Epoch: [")][0])
