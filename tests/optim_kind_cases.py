"""AdamW and LAMB in the fused step (csrc/optim_kinds.hip: dpc_adamw_dev / dpc_adamw_groups_dev, dpc_lamb_build_chunks / dpc_lamb_moments /
dpc_lamb_ratios / dpc_lamb_apply; BackboneEngine.set_optimizer / lamb_stats; the checkpoint's 'optimizer_kind' entry; optim.AdamW /
optim.LAMB; the entries' --optimizer / --wd_exclude_1d), shared by the CPU tier (host SIMT simulator, tests/test_optim_kind_emu.py)
and the GPU tier (tests/test_optim_kind_gpu.py).

Arena of the kernel cases: adam_groups_cases.layout() plus one active segment of 3 * 4096 + 4 floats, so that three chunk boundaries
of LAMB's work split (chunks of 4096 floats, cut from each segment's start) fall inside a segment and its last chunk holds one unit.
The data are those of a network in training rather than of a fresh one -- gradients and first moments around 1e-3, second moments
around 1e-6 -- because that is where L2 decay and decoupled decay part ways: L2's wd * p reaches p through m / sqrt(v), amplified
by 1 / sqrt(v), so with these data the two differ by ~2e-6 |p| where the bound on p is 1e-7 max|p|.

Bounds, all from the number format (f32, unit roundoff u = 2^-24):
  AdamW p    : 1e-7 * max(1, max|p|), the project's bound for one Adam step.  The kernel rounds p (1 - lr wd) on its own, as
               torch.optim.AdamW's param.mul_ does, and then subtracts the step as Adam does.
  m, v       : adam_groups_cases' bounds with the wd * p terms removed: 8 u (|b1 m| + |(1-b1) s g|), 8 u (|b2 v| + (1-b2) (s g)^2)
  wd = 0     : bit-identical to the Adam entries (the factor is 1.0f; x * 1 - y rounds as x - y)
  LAMB sum p^2 on integer data : exact (every square and every partial sum an integer far below 2^53)
  LAMB sum u^2 : relative 2 K u with K = 13, the roundings on the longest path of u = (m' / bc1) / (sqrt(v') * isb2 + eps) + wd p from the
               f32 state, constants included -- the path through v':  gscale * coef (1), g * gscale (1), the constant 1 - b2 (1),
               (1-b2) * gg (1), ... * gg (1), the sum with b2 v (1), sqrt (1), isb2 = 1 / sqrt(bc2) (2), sqrt(v') * isb2 (1), + eps (1),
               the quotient (1), the sum with wd p (1).  (The path through m' has 8.)  A relative error of K u in u is 2 K u in u^2.
  LAMB ratio : (K + 1) u relative: sqrt halves the 2 K u of sum u^2, sum p^2 is exact to n 2^-53, one rounding to f32
  LAMB p     : per element u |p_ref| + K' u lr r |u_ref|, K' = 2 K + 5 = 31: the subtraction's own rounding, and in the step lr r u the
               errors of u (K), of r (K + 1), of lr as an f32 constant (1), of lr * mult (1), of (lr mult) * r (1) and of ... * u (1).
               The project's 1e-7 * max(1, max|p|) is reported beside it and asserted too.
"""
import ctypes as C
import os
import re
import warnings

import pytest
import torch

import adam_groups_cases as ac
import ema_cases as ec
import grad_guard_cases as gc
import lr_schedule_cases as sc
from dpc_amd import _lib as L
from kcases import K

B1, B2, EPS = ac.B1, ac.B2, ac.EPS
U = 2.0 ** -24
U8 = 8.0 * U
K_U, K_P = 13, 31
CH = L.LAMB_CHUNK
BIG = ec.BIG
same = ec.same
new_state, new_record = gc.new_state, sc.new_record
f32 = sc.f32
all_same = sc.all_same


def layout():
    """adam_groups_cases.layout() plus the long segment; returns segs, n, special"""
    segs, n, sp = ac.layout()
    segs = list(segs) + [(n, n + 3 * CH + 4, 1e-3, 1e-5, 1)]
    sp = dict(sp, long=len(segs) - 1)
    return segs, n + 3 * CH + 4, sp


def trained_arenas(n, seed=51):
    """p, g, m, v, ema of a network in training (see the module docstring)"""
    gen = torch.Generator().manual_seed(seed)
    p0, g0 = torch.randn(n, generator=gen) * 0.5, torch.randn(n, generator=gen) * 2e-3
    m0, v0 = torch.randn(n, generator=gen) * 1e-3, torch.rand(n, generator=gen) * 1e-6 + 1e-8
    e0 = p0 + torch.randn(n, generator=gen) * 0.05
    return p0, g0, m0, v0, e0


def per_element(segs, n):
    lr_e, wd_e, act = torch.zeros(n), torch.zeros(n), torch.zeros(n, dtype=torch.bool)
    for b, e, lr, wd, a in segs:
        lr_e[b:e], wd_e[b:e], act[b:e] = lr, wd, bool(a)
    return lr_e, wd_e, act


def step3(k: K):
    """bias corrections of step 3, as the engine gets them"""
    step, bc = ec.step_at(k, 2), k.t(torch.ones(2))
    k.call("dpc_step_advance", step, bc, B1, B2)
    k.sync()
    return step, bc, bc.cpu()


# ------------------------------------------------------------------ runners
def run_adamw(k: K, arenas, lr, wd, bc, gscale, rec=None, state=None, ema=None, step=None, decay=0.0):
    dev = [k.t(t.clone()) for t in arenas] + ([k.t(ema.clone())] if ema is not None else [])
    k.call("dpc_adamw_dev", *dev[:4], arenas[0].numel(), lr, B1, B2, EPS, wd, bc, gscale, state, dev[4] if ema is not None else None,
           step if ema is not None else None, decay, rec)
    k.sync()
    return [t.cpu() for t in dev]


def run_adamw_groups(k: K, arenas, tab, nseg, bc, gscale, rec=None, state=None, ema=None, step=None, decay=0.0):
    dev = [k.t(t.clone()) for t in arenas] + ([k.t(ema.clone())] if ema is not None else [])
    k.call("dpc_adamw_groups_dev", *dev[:4], arenas[0].numel(), tab, nseg, B1, B2, EPS, bc, gscale, state,
           dev[4] if ema is not None else None, step if ema is not None else None, decay, rec)
    k.sync()
    return [t.cpu() for t in dev]


def u8(k: K, raw: bytes):
    return k.t(torch.frombuffer(bytearray(raw), dtype=torch.uint8).clone())


def lamb_tables(k: K, segs, n, adapt=None):
    """the segment table and its chunk table, built by the library's own host function, uploaded"""
    tab = (L.LambSegment * len(segs))()
    for i, (b, e, lr, wd, a) in enumerate(segs):
        tab[i] = L.LambSegment(b, e, lr, wd, int(a), 1 if adapt is None else int(adapt[i]), 0, 0)
    cap = n // CH + len(segs) + 1
    chunks = (L.LambChunk * cap)()
    nc = k.lib.call("dpc_lamb_build_chunks", tab, len(segs), n, chunks, cap)
    return {"seg": u8(k, bytes(tab)), "nseg": len(segs), "chunks": u8(k, bytes(chunks)[:nc * C.sizeof(L.LambChunk)]), "nc": nc,
            "host": [(c.begin, c.len, c.seg) for c in chunks[:nc]], "tab": tab, "cap": cap}


def read_records(k: K, records, nseg):
    k.sync()
    return list((L.LambRecord * nseg).from_buffer_copy(records.cpu().numpy().tobytes()[:nseg * C.sizeof(L.LambRecord)]))


RECORD_SENTINEL = bytes(L.LambRecord(-1.0, -2.0, -3.0, -4.0, -5.0, 77))


def run_lamb(k: K, arenas, T, bc, gscale, state=None, rec=None, ema=None, step=None, decay=0.0, stages=3):
    """the three launches (or the first `stages`) on device copies; host copies of everything they may write"""
    dev = [k.t(t.clone()) for t in arenas] + ([k.t(ema.clone())] if ema is not None else [])
    n = arenas[0].numel()
    partials = k.t(torch.full((2 * T["nc"],), float("nan"), dtype=torch.float64))
    records = u8(k, RECORD_SENTINEL * T["nseg"])
    k.call("dpc_lamb_moments", *dev[:4], n, T["seg"], T["nseg"], T["chunks"], T["nc"], B1, B2, EPS, bc, gscale, state, partials)
    if stages >= 2:
        k.call("dpc_lamb_ratios", T["seg"], T["nseg"], partials, T["nc"], state, records)
    if stages >= 3:
        k.call("dpc_lamb_apply", dev[0], dev[2], dev[3], n, T["seg"], T["nseg"], T["chunks"], T["nc"], EPS, bc, state, records,
               dev[4] if ema is not None else None, step if ema is not None else None, decay, rec)
    k.sync()
    return {"arenas": [t.cpu() for t in dev], "partials": partials.cpu(), "records": read_records(k, records, T["nseg"]),
            "raw_records": records.cpu()}


# ------------------------------------------------------------------ f64 references
def adamw_f64(p, g, m, v, lr, wd, bc, gscale):
    """one AdamW step in f64 from f32 state (lr, wd per element); new p, m, v and the m / v bounds"""
    p, g, m, v, lr, wd = (t.double() for t in (p, g, m, v, lr, wd))
    bc1, bc2 = float(bc[0]), float(bc[1])
    gg = g * gscale
    m2 = B1 * m + (1 - B1) * gg
    v2 = B2 * v + (1 - B2) * gg * gg
    p2 = p * (1 - lr * wd) - (lr / bc1) * m2 / (v2.sqrt() / bc2 ** 0.5 + EPS)
    return p2, m2, v2, U8 * ((B1 * m).abs() + (1 - B1) * gg.abs()), U8 * ((B2 * v).abs() + (1 - B2) * gg.abs() ** 2)


def lamb_f64(p, g, m, v, segs, bc, gscale, adapt=None, mult=1.0, unit_ratio=False):
    """one LAMB step in f64 from f32 state.  Returns p2, m2, v2, u, the m / v bounds, per segment (sum_p2, sum_u2, ratio) and the
    per-element bound on p.  Inactive segments and gaps keep p, m, v.  unit_ratio: r = 1 everywhere (the mutant of the teeth check)"""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    bc1, bc2 = float(bc[0]), float(bc[1])
    gg = g * gscale
    m2, v2, p2, u = m.clone(), v.clone(), p.clone(), torch.zeros_like(p)
    bm, bv, bp = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    recs = []
    for i, (b, e, lr, wd, a) in enumerate(segs):
        if not a:
            recs.append((0.0, 0.0, 1.0))
            continue
        s = slice(b, e)
        m2[s] = B1 * m[s] + (1 - B1) * gg[s]
        v2[s] = B2 * v[s] + (1 - B2) * gg[s] * gg[s]
        bm[s] = U8 * ((B1 * m[s]).abs() + (1 - B1) * gg[s].abs())
        bv[s] = U8 * ((B2 * v[s]).abs() + (1 - B2) * gg[s].abs() ** 2)
        u[s] = (m2[s] / bc1) / (v2[s].sqrt() / bc2 ** 0.5 + EPS) + f32(wd) * p[s]
        sp, su = float((p[s] ** 2).sum()), float((u[s] ** 2).sum())
        r = 1.0
        if (adapt is None or adapt[i]) and sp > 0 and su > 0 and not unit_ratio:
            r = (sp / su) ** 0.5
        recs.append((sp, su, r))
        lr_eff = f32(lr) * f32(mult)
        p2[s] = p[s] - lr_eff * r * u[s]
        bp[s] = U * p2[s].abs() + K_P * U * lr_eff * r * u[s].abs()
    return p2, m2, v2, u, bm, bv, recs, bp


def lamb_conditioned(p, g, m, v, segs, bc, gscale, recs, u, mult=1.0):
    """The engine cases' bounds.  A network's own gradients cancel in b1 m + (1-b1) g where random data do not (the second step of a
    run: 0.9 * 0.1 g1 against 0.1 g2 of the other sign), so the K roundings act on the summands, not on their sum: with
    u_abs = ((|b1 m| + |(1-b1) gg|) / bc1) / den + |wd p| >= |u|, the error of u is at most K u u_abs.  Per element
    u |p_ref| + K' u lr r u_abs bounds p; per segment K u sum(|u| u_abs) / sum(u^2) + u bounds the ratio's relative error (half of
    that of sum u^2, plus its rounding).  Without cancellation u_abs = |u| and both are the kernel cases' bounds."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    bc1, bc2 = float(bc[0]), float(bc[1])
    gg = g * gscale
    bp, rel = torch.zeros_like(p), []
    for (b, e, lr, wd, a), (sp, su, r) in zip(segs, recs):
        if not a:
            rel.append(0.0)
            continue
        s = slice(b, e)
        den = (B2 * v[s] + (1 - B2) * gg[s] * gg[s]).sqrt() / bc2 ** 0.5 + EPS
        u_abs = (((B1 * m[s]).abs() + ((1 - B1) * gg[s]).abs()) / bc1) / den + (f32(wd) * p[s]).abs()
        lr_eff = f32(lr) * f32(mult)
        bp[s] = U * (p[s] - lr_eff * r * u[s]).abs() + K_P * U * lr_eff * r * u_abs
        rel.append(K_U * U * float((u[s].abs() * u_abs).sum()) / su + U if su > 0 else 0.0)
    return bp, rel


# ------------------------------------------------------------------ case 1
def case_adamw_identity(k: K):
    """wd = 0: the bits of the Adam entries -- without a record those of _ex, with a record at mult = 1 and the average those of _sched;
    over more floats than one sweep of either kernel covers, a segment boundary inside the second sweep, and the scalar tail"""
    n = BIG
    p0, g0, m0, v0, e0 = ec.random_arenas(n, seed=61)
    four = (p0, g0, m0, v0)
    bc, step, one = ec.bias_corr(k), ec.step_at(k, 1000), new_record(k, mult=1.0, k=999)
    lr = 1e-2
    assert all_same(run_adamw(k, four, lr, 0.0, bc, 0.5), ec.run_plain(k, four, lr, 0.0, bc, 0.5))
    assert all_same(run_adamw(k, four, lr, 0.0, bc, 0.5, one, None, e0, step, 0.9), sc.run_plain(k, four, lr, 0.0, bc, 0.5, one, None, e0, step, 0.9))
    tab = ac.table(k, [(0, sc.TILE_SPLIT, lr, 0.0, 1), (sc.TILE_SPLIT, n, lr / 8, 0.0, 1)])
    got = run_adamw_groups(k, four, tab, 2, bc, 0.5)
    assert all_same(got, ec.run_groups(k, four, tab, 2, bc, 0.5)) and not same(got[0][-8:], p0[-8:])
    assert all_same(run_adamw_groups(k, four, tab, 2, bc, 0.5, one, None, e0, step, 0.9),
                    sc.run_groups(k, four, tab, 2, bc, 0.5, one, None, e0, step, 0.9))
    # small: the guard's record goes through as in the _ex entries; a length that is no multiple of four
    segs, n, _ = layout()
    p0, g0, m0, v0, e0 = ec.random_arenas(n, seed=62)
    four = (p0, g0, m0, v0)
    quarter = new_state(k, coef=0.25)
    assert all_same(run_adamw(k, four, lr, 0.0, bc, 0.5, None, quarter), ec.run_plain(k, four, lr, 0.0, bc, 0.5, quarter))
    flat = ac.table(k, [(b, e, s_lr, 0.0, a) for b, e, s_lr, _, a in segs])
    assert all_same(run_adamw_groups(k, four, flat, len(segs), bc, 0.5, None, quarter), ec.run_groups(k, four, flat, len(segs), bc, 0.5, quarter))
    assert all_same(run_adamw_groups(k, four, flat, len(segs), bc, 0.5, one, quarter, e0, step, 0.9),
                    sc.run_groups(k, four, flat, len(segs), bc, 0.5, one, quarter, e0, step, 0.9))
    q = [t[:4 * 300 + 3].clone() for t in four]
    assert all_same(run_adamw(k, q, lr, 0.0, bc, 0.5), ec.run_plain(k, q, lr, 0.0, bc, 0.5))
    rec = sc.read_record(k, one)
    assert (rec.mult, rec.k) == (1.0, 999)      # the record is only read


# ------------------------------------------------------------------ case 2
def case_adamw_f64(k: K, report=print):
    segs, n, sp = layout()
    p0, g0, m0, v0, e0 = trained_arenas(n)
    fb, fe = segs[sp["frozen"]][:2]
    ga, gb = sp["gap"]
    planted = [t.clone() for t in (p0, g0, m0, v0, e0)]
    for t in planted[1:]:      # g, m, v, ema: never read where nothing is updated
        t[fb:fe] = float("nan")
        t[ga:gb] = float("inf")
    step, bc, bc_h = step3(k)
    gscale = 0.5
    lr_e, wd_e, act = per_element(segs, n)
    zero = torch.zeros(())
    pz, gz, mz, vz = (torch.where(act, t, zero) for t in planted[:4])
    p2, m2, v2, bm, bv = adamw_f64(pz, gz, mz, vz, lr_e, wd_e, bc_h, gscale)
    bp = 1e-7 * max(1.0, p0.abs().max().item())
    tab = ac.table(k, segs)
    p, g, m, v, e = run_adamw_groups(k, planted[:4], tab, len(segs), bc, gscale, None, None, planted[4], step, 0.9)
    ep = (p.double() - p2).abs()[act].max().item()
    em = ((m.double() - m2).abs() / bm)[act].max().item()
    ev = ((v.double() - v2).abs() / bv)[act].max().item()
    report(f"adamw groups vs f64: p {ep:.3g} (bound {bp:.3g}), m {em:.3g} of its bound, v {ev:.3g} of its bound")
    assert ep <= bp and em <= 1.0 and ev <= 1.0
    for new, old in zip((p, g, m, v, e), planted):
        assert same(new[~act], old[~act])
    assert torch.isnan(m[fb:fe]).all() and torch.isinf(e[ga:gb]).all() and torch.isfinite(p).all() and torch.isfinite(e[act]).all()
    assert not same(e[act], planted[4][act])
    zb, ze = segs[sp["lr0"]][:2]
    assert same(p[zb:ze], p0[zb:ze]) and not same(m[zb:ze], m0[zb:ze]) and not same(v[zb:ze], v0[zb:ze])
    # teeth: L2 decay on the same data is another update
    l2 = ec.run_groups(k, planted[:4], tab, len(segs), bc, gscale)[0]
    heavy = act & (wd_e == f32(1e-3)) & (lr_e == f32(1e-4))
    miss = ((l2.double() - p2).abs() > bp)[heavy].float().mean().item()
    report(f"the L2 entry misses the bound on {miss:.2f} of the {int(heavy.sum())} elements of the (1e-4, 1e-3) segments")
    assert int(heavy.sum()) >= 200 and miss > 0.5
    # the one-group entry, same reference
    lr, wd = 1e-3, 1e-2
    p, g, m, v = run_adamw(k, (p0, g0, m0, v0), lr, wd, bc, gscale)
    p2, m2, v2, bm, bv = adamw_f64(p0, g0, m0, v0, torch.full((n,), lr), torch.full((n,), wd), bc_h, gscale)
    ep = (p.double() - p2).abs().max().item()
    em, ev = ((m.double() - m2).abs() / bm).max().item(), ((v.double() - v2).abs() / bv).max().item()
    report(f"adamw one-group vs f64: p {ep:.3g} (bound {bp:.3g}), m {em:.3g}, v {ev:.3g} of their bounds")
    assert ep <= bp and em <= 1.0 and ev <= 1.0
    # ... and with a record: the step and the decay both scale with lr * mult
    mult = f32(0.3)
    p = run_adamw(k, (p0, g0, m0, v0), lr, wd, bc, gscale, new_record(k, mult=mult, k=9))[0]
    p2 = adamw_f64(p0, g0, m0, v0, torch.full((n,), lr).double() * mult, torch.full((n,), wd), bc_h, gscale)[0]
    bp3 = bp + U * (p2 - p0.double()).abs()      # one more f32 rounding of the step size
    assert ((p.double() - p2).abs() <= bp3).all()


# ------------------------------------------------------------------ case 3
def case_lamb_sum_p2_exact(k: K):
    segs, n, sp = layout()
    T = lamb_tables(k, segs, n)
    _, _, act = per_element(segs, n)
    # the chunk table itself: chunks of at most CH floats, inside one active segment each, in order, covering exactly the live floats
    cover = torch.zeros(n, dtype=torch.int32)
    for b, ln, s in T["host"]:
        assert 0 < ln <= CH and ln % 4 == 0 and segs[s][0] <= b and b + ln <= segs[s][1] and segs[s][4]
        cover[b:b + ln] += 1
    assert torch.equal(cover == 1, act) and int(cover.max()) == 1
    lb, le = segs[sp["long"]][:2]
    assert [c for c in T["host"] if c[2] == sp["long"]] == [(lb + i * CH, CH, sp["long"]) for i in range(3)] + [(lb + 3 * CH, 4, sp["long"])]
    assert C.sizeof(L.LambSegment) == 48 and C.sizeof(L.LambChunk) == 16 and C.sizeof(L.LambRecord) == 32
    gen = torch.Generator().manual_seed(71)
    p0 = torch.randint(-8, 9, (n,), generator=gen).float()
    _, g0, m0, v0, _ = trained_arenas(n, seed=72)
    fb, fe = segs[sp["frozen"]][:2]
    ga, gb = sp["gap"]
    for t in (p0, g0, m0, v0):
        t[fb:fe] = float("nan")
        t[ga:gb] = float("inf")
    small = next(i for i, s in enumerate(segs) if s[1] - s[0] == 4 and s[4])
    sb, se = segs[small][:2]
    spots = [sb, se - 1, n - 1, ga - 1, gb] + [lb + i * CH + d for i in (1, 2, 3) for d in (-1, 0)]
    assert act[spots].all() and len(set(spots)) == 11
    p0[spots] = 0.0
    _, bc, _ = step3(k)
    base = run_lamb(k, (p0, g0, m0, v0), T, bc, 1.0, stages=2)
    again = run_lamb(k, (p0, g0, m0, v0), T, bc, 1.0, stages=2)
    assert torch.equal(base["partials"].view(torch.int64), again["partials"].view(torch.int64))   # every slot written, the same bits
    assert torch.equal(base["raw_records"], again["raw_records"]) and torch.isfinite(base["partials"]).all()
    assert same(base["arenas"][0], p0)                                      # moments leaves p alone
    for i, (b, e, _, _, a) in enumerate(segs):
        want = float((p0[b:e].double() ** 2).sum()) if a else 0.0
        assert base["records"][i].sum_p2 == want, (i, base["records"][i].sum_p2, want)
        assert base["records"][i].pnorm == f32(want ** 0.5)
    seg_of = lambda pos: next(i for i, s in enumerate(segs) if s[0] <= pos < s[1])   # noqa: E731
    rsz = C.sizeof(L.LambRecord)
    for pos in spots:
        q = p0.clone()
        q[pos] = 4096.0
        out = run_lamb(k, (q, g0, m0, v0), T, bc, 1.0, stages=2)
        hit = seg_of(pos)
        assert out["records"][hit].sum_p2 - base["records"][hit].sum_p2 == 2.0 ** 24, (pos, hit)
        others = torch.ones(len(segs) * rsz, dtype=torch.bool)
        others[hit * rsz:(hit + 1) * rsz] = False
        assert torch.equal(out["raw_records"][others], base["raw_records"][others]), pos


# ------------------------------------------------------------------ case 4
def case_lamb_f64(k: K, report=print):
    segs, n, sp = layout()
    T = lamb_tables(k, segs, n)
    p0, g0, m0, v0, e0 = trained_arenas(n, seed=81)
    fb, fe = segs[sp["frozen"]][:2]
    ga, gb = sp["gap"]
    planted = [t.clone() for t in (p0, g0, m0, v0, e0)]
    for t in planted:
        t[fb:fe] = float("nan")
        t[ga:gb] = float("inf")
    step, bc, bc_h = step3(k)
    gscale = 0.5
    lr_e, _, act = per_element(segs, n)
    zero = torch.zeros(())
    pz, gz, mz, vz = (torch.where(act, t, zero) for t in planted[:4])
    p2, m2, v2, u, bm, bv, recs, bp = lamb_f64(pz, gz, mz, vz, segs, bc_h, gscale)
    out = run_lamb(k, planted[:4], T, bc, gscale, None, None, planted[4], step, 0.9)
    p, g, m, v, e = out["arenas"]
    worst_u = worst_r = 0.0
    for i, (r, (sp2, su2, ratio)) in enumerate(zip(out["records"], recs)):
        if not segs[i][4]:
            assert (r.sum_p2, r.sum_u2, r.pnorm, r.unorm, r.ratio) == (0.0, 0.0, 0.0, 0.0, 1.0)
            continue
        eu, er = abs(r.sum_u2 - su2) / su2, abs(r.ratio - ratio) / ratio
        worst_u, worst_r = max(worst_u, eu / (2 * K_U * U)), max(worst_r, er / ((K_U + 1) * U))
        assert abs(r.sum_p2 - sp2) <= 1e-12 * sp2 and abs(r.unorm - su2 ** 0.5) <= (K_U + 1) * U * su2 ** 0.5
    em = ((m.double() - m2).abs() / bm)[act].max().item()
    ev = ((v.double() - v2).abs() / bv)[act].max().item()
    err = (p.double() - p2).abs()
    ep = (err / bp)[act & (lr_e > 0)].max().item()
    flat = 1e-7 * max(1.0, p0.abs().max().item())
    report(f"lamb vs f64: sum_u2 {worst_u:.3g}, ratio {worst_r:.3g}, m {em:.3g}, v {ev:.3g}, p {ep:.3g} of their bounds; "
           f"p max error {err[act].max().item():.3g} (the project's bound {flat:.3g})")
    assert worst_u <= 1.0 and worst_r <= 1.0 and em <= 1.0 and ev <= 1.0 and ep <= 1.0 and err[act].max().item() <= flat
    for new, old in zip((p, g, m, v, e), planted):
        assert same(new[~act], old[~act])
    zb, ze = segs[sp["lr0"]][:2]
    assert same(p[zb:ze], p0[zb:ze]) and not same(m[zb:ze], m0[zb:ze])
    # the average: the f64 lerp of the p the kernel wrote
    _, w = ec.ema_weight(3, 0.9)
    ref, be = ec.ema_ref(planted[4], p, w)
    assert ((e.double() - ref).abs() <= be)[act].all() and not same(e[act], e0[act])
    # teeth: the same step with r = 1 is far outside the per-element bound wherever the ratio matters
    p1 = lamb_f64(pz, gz, mz, vz, segs, bc_h, gscale, unit_ratio=True)[0]
    matters = torch.zeros(n, dtype=torch.bool)
    for (b, e_, lr, _, a), (_, _, ratio) in zip(segs, recs):
        matters[b:e_] = bool(a) and lr > 0 and abs(ratio - 1.0) > 0.01
    miss = ((p.double() - p1).abs() > bp)[matters].float().mean().item()
    report(f"r = 1 misses the bound on {miss:.3f} of {int(matters.sum())} elements")
    assert int(matters.sum()) > n // 4 and miss > 0.5
    # with the schedule's record: lr * mult, the f32 product first
    mult = f32(0.3)
    out = run_lamb(k, planted[:4], T, bc, gscale, None, new_record(k, mult=mult, k=9))
    p2, _, _, _, _, _, _, bp = lamb_f64(pz, gz, mz, vz, segs, bc_h, gscale, mult=mult)
    assert ((out["arenas"][0].double() - p2).abs() <= bp)[act].all()


# ------------------------------------------------------------------ case 5
def case_lamb_degenerate(k: K):
    n = 16 + CH + 8 + 8
    segs = [(0, 8, 1e-3, 1e-3, 1), (8, 16, 1e-3, 0.0, 1), (16, 16 + CH + 8, 1e-3, 1e-3, 1), (16 + CH + 8, n, 1e-3, 1e-3, 1)]
    adapt = [1, 1, 0, 1]
    T = lamb_tables(k, segs, n, adapt)
    p0, g0, m0, v0, _ = trained_arenas(n, seed=91)
    p0[0:8] = 0.0                       # p = 0, g != 0
    g0[8:16], m0[8:16] = 0.0, 0.0       # nothing to step along, no decay
    _, bc, bc_h = step3(k)
    out = run_lamb(k, (p0, g0, m0, v0), T, bc, 1.0)
    r = out["records"]
    p = out["arenas"][0]
    assert r[0].ratio == 1.0 and r[0].pnorm == 0.0 and r[0].unorm > 0 and not same(p[0:8], p0[0:8])
    assert r[1].ratio == 1.0 and r[1].unorm == 0.0 and r[1].pnorm > 0 and same(p[8:16], p0[8:16])
    _, _, _, _, _, _, recs, bp = lamb_f64(p0, g0, m0, v0, segs, bc_h, 1.0, adapt)
    assert r[2].ratio == 1.0 and abs(r[2].pnorm - recs[2][0] ** 0.5) <= U * 2 * recs[2][0] ** 0.5
    assert abs(r[2].unorm - recs[2][1] ** 0.5) <= (K_U + 1) * U * recs[2][1] ** 0.5 and abs((recs[2][0] / recs[2][1]) ** 0.5 - 1.0) > 0.01
    assert r[3].ratio != 1.0 and abs(r[3].ratio - recs[3][2]) <= (K_U + 1) * U * recs[3][2]
    p2 = lamb_f64(p0, g0, m0, v0, segs, bc_h, 1.0, adapt)[0]
    assert ((p.double() - p2).abs() <= bp).all()


# ------------------------------------------------------------------ case 6
def case_skip_and_coef(k: K):
    segs, n, sp = layout()
    T = lamb_tables(k, segs, n)
    p0, g0, m0, v0, e0 = trained_arenas(n, seed=101)
    host = (p0, g0, m0, v0)
    bad = g0.clone()
    bad[segs[sp["long"]][0] + CH + 1] = float("nan")
    step, bc, _ = step3(k)
    tab = ac.table(k, segs)
    stop = new_state(k, coef=0.0, skip=1)
    one = new_record(k, mult=0.5, k=3)
    still = [p0, bad, m0, v0, e0]
    assert all_same(run_adamw(k, (p0, bad, m0, v0), 1e-3, 1e-2, bc, 1.0, one, stop, e0, step, 0.9), still)
    assert all_same(run_adamw_groups(k, (p0, bad, m0, v0), tab, len(segs), bc, 1.0, one, stop, e0, step, 0.9), still)
    out = run_lamb(k, (p0, bad, m0, v0), T, bc, 1.0, stop, one, e0, step, 0.9)
    assert all_same(out["arenas"], still)
    assert torch.isnan(out["partials"]).all() and out["raw_records"].numpy().tobytes() == RECORD_SENTINEL * len(segs)
    # coef = 0.25: the same call given g * 0.25 (a power of two commutes with every rounding)
    quarter, whole = new_state(k, coef=0.25), new_state(k, coef=1.0)
    gq = g0 * 0.25
    drop_g = lambda a: a[:1] + a[2:]   # noqa: E731
    assert all_same(drop_g(run_adamw(k, host, 1e-3, 1e-2, bc, 1.0, None, quarter)), drop_g(run_adamw(k, (p0, gq, m0, v0), 1e-3, 1e-2, bc, 1.0, None, whole)))
    assert all_same(drop_g(run_adamw_groups(k, host, tab, len(segs), bc, 1.0, None, quarter)),
                    drop_g(run_adamw_groups(k, (p0, gq, m0, v0), tab, len(segs), bc, 1.0, None, whole)))
    a, b = run_lamb(k, host, T, bc, 1.0, quarter), run_lamb(k, (p0, gq, m0, v0), T, bc, 1.0, whole)
    assert all_same(drop_g(a["arenas"]), drop_g(b["arenas"])) and torch.equal(a["raw_records"], b["raw_records"])
    assert torch.equal(a["partials"].view(torch.int64), b["partials"].view(torch.int64)) and not same(a["arenas"][0], p0)


# ------------------------------------------------------------------ case 7
def case_argument_checks(k: K):
    segs, n, _ = layout()
    T = lamb_tables(k, segs, n)
    tab, S = ac.table(k, segs), len(segs)
    host = trained_arenas(n + 4, seed=111)
    dev = [k.t(t.clone()) for t in host]
    four, ema = [t[:n] for t in dev[:4]], dev[4][:n]
    p, g, m, v = four
    bc, st, one = ec.bias_corr(k), ec.step_at(k, 5), new_record(k, mult=1.0, k=4)
    partials = k.t(torch.full((2 * T["nc"],), -1.0, dtype=torch.float64))
    records = u8(k, RECORD_SENTINEL * S)

    def aw(p_=p, g_=g, e=None, s=None, d=0.0, r=None, nn=n):
        k.call("dpc_adamw_dev", p_, g_, m, v, nn, 1e-3, B1, B2, EPS, 1e-2, bc, 1.0, None, e, s, d, r)

    def awg(p_=p, e=None, s=None, d=0.0, r=None, nn=n, ns=S, tb=tab):
        k.call("dpc_adamw_groups_dev", p_, g, m, v, nn, tb, ns, B1, B2, EPS, bc, 1.0, None, e, s, d, r)

    def mo(p_=p, nn=n, sg=T["seg"], ns=S, ch=T["chunks"], nc=T["nc"], pt=partials):
        k.call("dpc_lamb_moments", p_, g, m, v, nn, sg, ns, ch, nc, B1, B2, EPS, bc, 1.0, None, pt)

    def ra(sg=T["seg"], ns=S, pt=partials, nc=T["nc"], rc=records):
        k.call("dpc_lamb_ratios", sg, ns, pt, nc, None, rc)

    def ap(p_=p, nn=n, sg=T["seg"], ns=S, ch=T["chunks"], nc=T["nc"], rc=records, e=None, s=None, d=0.0):
        k.call("dpc_lamb_apply", p_, m, v, nn, sg, ns, ch, nc, EPS, bc, None, rc, e, s, d, None)

    off = dev[0][1:n + 1]       # 4 bytes past a 16-byte boundary
    bad = [lambda: aw(p_=None), lambda: aw(p_=off), lambda: aw(g_=dev[1][1:n + 1]), lambda: aw(e=ema), lambda: aw(s=st),
           lambda: aw(e=p, s=st, d=0.9), lambda: aw(e=ema, s=st, d=1.0), lambda: aw(e=dev[4][1:n + 1], s=st, d=0.9), lambda: aw(nn=0),
           lambda: awg(p_=None), lambda: awg(p_=off), lambda: awg(nn=n + 2), lambda: awg(ns=0), lambda: awg(ns=L.ADAM_MAX_SEGMENTS + 1),
           lambda: awg(tb=None), lambda: awg(e=p, s=st, d=0.9), lambda: awg(e=ema), lambda: awg(e=ema, s=st, d=0.0),
           lambda: mo(p_=None), lambda: mo(p_=off), lambda: mo(nn=n + 2), lambda: mo(sg=None), lambda: mo(ns=L.ADAM_MAX_SEGMENTS + 1),
           lambda: mo(ch=None), lambda: mo(nc=0), lambda: mo(pt=None),
           lambda: ra(sg=None), lambda: ra(ns=0), lambda: ra(ns=L.ADAM_MAX_SEGMENTS + 1), lambda: ra(pt=None), lambda: ra(nc=0), lambda: ra(rc=None),
           lambda: ap(p_=None), lambda: ap(p_=off), lambda: ap(nn=n + 2), lambda: ap(sg=None), lambda: ap(ns=L.ADAM_MAX_SEGMENTS + 1),
           lambda: ap(ch=None), lambda: ap(nc=0), lambda: ap(rc=None), lambda: ap(e=p, s=st, d=0.9), lambda: ap(e=ema), lambda: ap(e=ema, s=st, d=1.0)]
    for i, f in enumerate(bad):
        with pytest.raises(L.DpcError, match=f"code {L.ERR_ARG}$"):
            f()
            pytest.fail(f"call {i} was accepted")
    k.sync()
    assert all_same([t.cpu() for t in dev], list(host))
    assert (partials.cpu() == -1.0).all() and records.cpu().numpy().tobytes() == RECORD_SENTINEL * S
    # the host builder refuses what the kernels rely on
    def build(rows, nn=n, cap=None):
        t = (L.LambSegment * max(len(rows), 1))()
        for i, (b, e, lr, wd, a) in enumerate(rows):
            t[i] = L.LambSegment(b, e, lr, wd, a, 1, 0, 0)
        cap = T["cap"] if cap is None else cap
        return k.lib.call("dpc_lamb_build_chunks", t, len(rows), nn, (L.LambChunk * max(cap, 1))(), cap)
    for rows, kw in (([(0, 8, 1e-3, 0.0, 1), (4, 12, 1e-3, 0.0, 1)], {}), ([(0, 6, 1e-3, 0.0, 1)], {}), ([(2, 8, 1e-3, 0.0, 1)], {}),
                     ([(0, n + 4, 1e-3, 0.0, 1)], {}), ([(8, 8, 1e-3, 0.0, 1)], {}), ([(0, 8, -1.0, 0.0, 1)], {}), ([(0, 8, 1e-3, float("nan"), 1)], {}),
                     ([], {}), (segs, dict(cap=3)), (segs, dict(nn=n + 2)), ([(0, 4, 1e-3, 0.0, 1)] * (L.ADAM_MAX_SEGMENTS + 1), {})):
        with pytest.raises(L.DpcError, match=f"code {L.ERR_ARG}$"):
            build(rows, **kw)
    assert build(segs) == T["nc"] and build([(0, 8, 1e-3, 0.0, 0)]) == 0
    # ... and the calls go through once the arguments are right
    aw(e=ema, s=st, d=0.9, r=one)
    mo()
    ra()
    ap(e=ema, s=st, d=0.9)
    k.sync()
    assert not same(p.cpu(), host[0][:n]) and not same(ema.cpu(), host[4][:n]) and same(dev[0][n:].cpu(), host[0][n:])


# ====================================================================== engine, checkpoints, module boundary, entries
Cfg = gc.Cfg
dpc_engine, dpc_input, lc_engine = gc.dpc_engine, gc.dpc_input, gc.lc_engine
arenas, same_bits = gc.arenas, gc.same_bits
SCHED = sc.SCHED      # warm-up 2, cosine to 5
DECAY = 0.9
KINDS = ("adamw", "lamb")
_RUNS = {}


def eng_segs(eng, groups=None, exclude_1d=False):
    """[(begin, end, lr, wd, active)] per parameter slot, from the engine's layout and the test's own statement of the groups;
    adapt flags; names"""
    per = None if groups is None else {k: (g["lr"], g["weight_decay"]) for g in groups for k in g["params"]}
    segs, adapt, names = [], [], []
    for k, (o, n) in eng.offsets.items():
        one_d = len(eng.shapes[k]) <= 1
        if per is None:
            lr, wd, a = eng.lr, eng.wd, 1
        else:
            lr, wd, a = per[k] + (1,) if k in per else (0.0, 0.0, 0)
        segs.append((o, o + (n + 3) // 4 * 4, lr, 0.0 if (exclude_1d and one_d) else wd, a))
        adapt.append(int(a and not (exclude_1d and one_d)))
        names.append(k)
    return segs, adapt, names


def snapshot(eng):
    """p, m, v as they stand, on the engine's device (the f64 references of the engine cases run there too)"""
    return [t.detach().clone() for t in (eng.flat_p, eng.flat_m, eng.flat_v)]


def check_step(eng, kind, before, segs, adapt, names, mult=1.0, what="", report=print):
    """the step the engine has just taken, against the f64 recurrence from the state before it and the engine's own gradient"""
    p0, m0, v0 = before
    g = eng.flat_g.detach()
    bc = eng.dev_bc.cpu()
    p, m, v = snapshot(eng)
    n = eng.numel
    lr_e, wd_e, act = (t.to(g.device) for t in per_element(segs, n))
    zero = torch.zeros((), device=g.device)
    gz = torch.where(act, g, zero)      # (a frozen parameter's gradient slot may hold anything)
    flat = 1e-7 * max(1.0, p0.abs().max().item())
    if kind == "adamw":
        lr_eff = lr_e.double() * f32(mult)
        p2, m2, v2, bm, bv = adamw_f64(p0, gz, m0, v0, lr_eff, wd_e, bc, 1.0)
        # per element, from the format: the decayed p and the difference are rounded once each (2 u |p|), the factor 1 - lr wd lies in
        # [1/2, 1) and is rounded to u / 2; the step (lr mult / bc1) m' / (sqrt(v') isb2 + eps) has K = 13 roundings on its longest
        # path (the docstring's count for u), acting on the summands of m' where those cancel (see lamb_conditioned)
        den = v2.sqrt() / float(bc[1]) ** 0.5 + EPS
        step_abs = (lr_eff / float(bc[0])) * ((B1 * m0.double()).abs() + ((1 - B1) * gz.double()).abs()) / den
        bp = 2.5 * U * p2.abs() + (K_U + 2) * U * step_abs
    else:
        p2, m2, v2, u, bm, bv, recs, _ = lamb_f64(p0, gz, m0, v0, segs, bc, 1.0, adapt, mult)
        bp, rel = lamb_conditioned(p0, gz, m0, v0, segs, bc, 1.0, recs, u, mult)
        stats = eng.lamb_stats()
        assert list(stats) == [k for k, s in zip(names, segs) if s[4]]
        for k, (sp, su, r), rr in zip(names, recs, rel):
            if k in stats and su > 0:
                assert abs(stats[k][2] - r) <= rr * r, (what, k, stats[k], r, rr)
                assert abs(stats[k][0] - sp ** 0.5) <= 2 * U * sp ** 0.5
    err = (p.double() - p2).abs()
    live = act & (lr_e > 0)
    ep = (err / bp.clamp_min(1e-300))[live].max().item()      # (a slot's padding: p = u = 0, error 0, bound 0)
    tiny = 2.0 ** -126      # below the normal range f32 keeps absolute, not relative, precision: g^2 of a gradient of 1e-25 is no f32
    em = ((m.double() - m2).abs() / (bm + tiny))[act].max().item()
    ev = ((v.double() - v2).abs() / (bv + tiny))[act].max().item()
    report(f"{what} {kind} vs f64: p {ep:.3g}, m {em:.3g}, v {ev:.3g} of their bounds; p max error {err[act].max().item():.3g} (the project's flat bound {flat:.3g})")
    assert ep <= 1.0 and em <= 1.0 and ev <= 1.0, what
    assert kind == "adamw" or err[act].max().item() <= flat, what      # lamb rounds p once: u |p| stays under the flat bound too
    for new, old in ((p, p0), (m, m0), (v, v0)):
        assert same(new[~act], old[~act]), what
    assert not same(p[live], p0[live])
    return p


def kind_run(cfg: Cfg, kind: str, dtype):
    """three train steps of the one-group DPC engine under `kind`, each held to the f64 recurrence; computed once: the arenas after
    each step, the checkpoint dictionary after the second, the launches per step"""
    from dpc_amd import checkpoint as ckpt
    key = (kind, cfg.device, tuple(cfg.widths), dtype)
    if key not in _RUNS:
        eng, x = dpc_engine(cfg, dtype), dpc_input(cfg)
        eng.wd = 1e-2      # a decay that shows: (the engine's default is the reference's 1e-5)
        eng.set_optimizer(kind)
        segs, adapt, names = eng_segs(eng)
        rec = {"steps": [], "launches": []}
        for i in range(3):
            before, n0 = snapshot(eng), eng._launches
            eng.train_step(x)
            rec["launches"].append(eng._launches - n0)
            rec["last"] = L.last_kernel(eng.lib)
            check_step(eng, kind, before, segs, adapt, names, what=f"DPC step {i + 1}")
            rec["steps"].append(arenas(eng))
            if i == 1:
                rec["state2"] = ckpt.build_state(eng, 1, "resnet18", 0.0, 2)
        if kind == "lamb":
            rec["stats"] = eng.lamb_stats()
        _RUNS[key] = rec
    return _RUNS[key]


def case_adam_is_adam(cfg: Cfg, dtype=torch.float32):
    """set_optimizer("adam") changes nothing: bits, launches, baked scalars, the kernel launched"""
    x = dpc_input(cfg)
    ref = gc.twin(cfg, dtype)      # two steps of an engine that never heard of set_optimizer, computed once per session
    a, b = dpc_engine(cfg, dtype), dpc_engine(cfg, dtype)
    base = a._baked_scalars()
    b.set_optimizer("adam")
    assert b._baked_scalars() == base and b.optimizer_kind == "adam" and b._lamb is None
    a.train_step(x)
    first = a._launches
    assert same_bits(arenas(a), ref["steps"][0]["arenas"])
    for i in range(2):
        nb = b._launches
        b.train_step(x)
        assert b._launches - nb == first and L.last_kernel(b.lib).startswith("adam_dev_kernel<false>")
        assert same_bits(arenas(b), ref["steps"][i]["arenas"]), f"step {i + 1}"
    a.train_step(x)
    # on, then off again: the key and the entry of an engine that never had another rule
    b.set_optimizer("lamb")
    assert b._baked_scalars()[:len(base)] == base and b._baked_scalars()[-1][:2] == ("optimizer", "lamb")
    b.set_optimizer("adam")
    assert b._baked_scalars() == base
    a.adam_step()
    b.adam_step()
    assert same_bits(arenas(a), arenas(b)) and L.last_kernel(b.lib).startswith("adam_dev_kernel<false>")
    with pytest.raises(ValueError):
        a.set_optimizer("lars")
    with pytest.raises(ValueError):
        a.set_optimizer("adam", exclude_1d=True)
    with pytest.raises(RuntimeError, match="never enabled"):
        a.lamb_stats()


def case_adamw_without_decay(cfg: Cfg, dtype=torch.float32):
    """adamw with wd = 0 is Adam with wd = 0, bit for bit, launch for launch"""
    x = dpc_input(cfg)
    a, b = dpc_engine(cfg, dtype), dpc_engine(cfg, dtype)
    a.wd = b.wd = 0.0
    b.set_optimizer("adamw")
    for i in range(2):
        na, nb = a._launches, b._launches
        a.train_step(x)
        b.train_step(x)
        assert a._launches - na == b._launches - nb and L.last_kernel(b.lib).startswith("adamw_dev_kernel<false>")
        assert same_bits(arenas(a), arenas(b)), f"step {i + 1}"
    assert not torch.equal(a.flat_p, dpc_engine(cfg, dtype).flat_p)


def case_recurrence(cfg: Cfg, kind: str, dtype=torch.float32):
    """three steps of the one-group engine, each held to the f64 recurrence inside kind_run"""
    run = kind_run(cfg, kind, dtype)
    assert run["last"].startswith("adamw_dev_kernel<false>" if kind == "adamw" else "lamb_apply_kernel<false>"), run["last"]
    assert len(set(run["launches"][1:])) == 1
    if kind == "lamb":
        r = [v[2] for v in run["stats"].values()]
        assert all(x > 0 for x in r) and max(r) / min(r) > 2.0      # layer-wise rates: they differ between tensors


def case_launch_counts(cfg: Cfg, dtype=torch.float32):
    """adamw launches what Adam launches; lamb two more"""
    counts = {}
    for kind in ("adam",) + KINDS:
        eng = dpc_engine(cfg, dtype)
        eng.set_optimizer(kind)
        eng.flat_g.normal_(0.0, 0.01)
        n0 = eng._launches
        eng.adam_step()
        counts[kind] = eng._launches - n0
    assert counts["adamw"] == counts["adam"] and counts["lamb"] == counts["adam"] + 2, counts


def head_groups(eng, lr=1e-3, wd=1e-3):
    head = [k for k in eng.offsets if k.startswith(("final_bn.", "final_fc."))]   # lc_main --train_what head
    return [{"params": head, "lr": lr, "weight_decay": wd}]


def case_recurrence_groups(cfg: Cfg, kind: str, num_class: int = 11):
    """LC with `head` groups: three steps against the recurrence; the frozen backbone bit-still (check_step) and outside
    lamb_stats(); the padding floats inside final_fc.bias' 16-byte slot stay +0 in p, m, v"""
    assert num_class % 4
    eng, x = lc_engine(cfg, num_class), dpc_input(cfg)
    groups = head_groups(eng)
    eng.set_param_groups(groups)
    eng.set_optimizer(kind)
    target = (torch.arange(cfg.B) % num_class).to(cfg.device)
    segs, adapt, names = eng_segs(eng, groups)
    p_start = eng.flat_p.detach().clone()
    for i in range(3):
        before = snapshot(eng)
        eng.train_step(x, target)
        check_step(eng, kind, before, segs, adapt, names, what=f"LC head step {i + 1}")
    assert ("adamw_groups_kernel<false>" if kind == "adamw" else "lamb_apply_kernel<false>") in L.last_kernel(eng.lib)
    frozen = eng.frozen_params()
    assert frozen and any(k.startswith("backbone.") for k in frozen)
    for k in frozen:
        o, n = eng.offsets[k]
        assert same(eng.flat_p[o:o + n], p_start[o:o + n])
    o, n = eng.offsets["final_fc.1.bias"] if "final_fc.1.bias" in eng.offsets else eng.offsets[[k for k in eng.offsets if k.startswith("final_fc.") and k.endswith("bias")][0]]
    assert n == num_class
    pad = slice(o + n, o + (n + 3) // 4 * 4)
    for t in (eng.flat_p, eng.flat_m, eng.flat_v):
        assert (t[pad].cpu().view(torch.int32) == 0).all()      # +0 bits
    assert eng.flat_m[o:o + n].abs().max().item() > 0
    if kind == "lamb":
        assert set(eng.lamb_stats(adaptive_only=True)) == set(groups[0]["params"]) and not set(eng.lamb_stats()) & set(frozen)
        eng.set_optimizer("lamb", exclude_1d=True)
        two_d = {k for k in groups[0]["params"] if len(eng.shapes[k]) > 1}
        assert set(eng.lamb_stats(adaptive_only=True)) == two_d and two_d and two_d != set(groups[0]["params"])
        before = snapshot(eng)
        eng.train_step(x, target)
        segs, adapt, names = eng_segs(eng, groups, exclude_1d=True)
        check_step(eng, kind, before, segs, adapt, names, what="LC head, exclude_1d")
        assert all(v[2] == 1.0 for k, v in eng.lamb_stats().items() if k not in two_d)
    else:
        eng.set_optimizer("adamw", exclude_1d=True)
        before = snapshot(eng)
        eng.train_step(x, target)
        segs, adapt, names = eng_segs(eng, groups, exclude_1d=True)
        check_step(eng, kind, before, segs, adapt, names, what="LC head, exclude_1d")
        assert "adamw_groups_kernel<false>" in L.last_kernel(eng.lib)


def case_combined(cfg: Cfg, kind: str, dtype=torch.float32):
    """guard + average + schedule under `kind`: a NaN gradient leaves everything untouched; then five steps of warm-up 2 + cosine to 5
    against the recurrence stepping with float32(lr) * float32(mult), the average against the f64 lerp of the new p"""
    from dpc_amd.optim import lr_multiplier
    eng, x = dpc_engine(cfg, dtype), dpc_input(cfg)
    eng.wd = 1e-2
    eng.set_grad_guard(max_norm=1e30, skip_nonfinite=True)
    eng.set_ema(DECAY)
    eng.set_lr_schedule(SCHED)
    eng.set_optimizer(kind)
    segs, adapt, names = eng_segs(eng)
    eng._forward_loss(x, True)
    eng.backward()
    o, _ = eng.offsets["backbone.layer2.0.conv1.weight"]
    eng.flat_g[o + 5] = float("nan")
    extra = lambda: [eng.flat_ema.detach().clone(), eng._lr_state.detach().clone()] + ([eng._lamb["records"].detach().clone()] if kind == "lamb" else [])  # noqa: E731
    before, before_x = arenas(eng), extra()
    eng.adam_step()
    assert eng.grad_stats()["skip"] == 1 and same_bits(arenas(eng), before) and all(torch.equal(a, b) for a, b in zip(extra(), before_x))
    assert eng.step_count == 0 and int(eng.dev_step.item()) == 0
    for i in range(sc.STEPS):
        snap, e0 = snapshot(eng), eng.flat_ema.detach().clone()
        eng.train_step(x)
        now = eng.lr_now()
        assert now["k"] == i and sc.ulps(now["mult"], f32(lr_multiplier(i, SCHED))) <= (1 if i > 2 else 0)
        p = check_step(eng, kind, snap, segs, adapt, names, mult=now["mult"], what=f"combined step {i + 1}")
        _, w = ec.ema_weight(i + 1, DECAY)
        ref, be = ec.ema_ref(e0, p, w)
        assert ((eng.flat_ema.double() - ref).abs() <= be).all(), f"average, step {i + 1}"
    assert ("adamw_dev_kernel<true>" if kind == "adamw" else "lamb_apply_kernel<true>") in L.last_kernel(eng.lib)
    assert eng.grad_stats()["n_skipped"] == 1 and eng.step_count == sc.STEPS


def case_checkpoint(cfg: Cfg, kind: str, tmp_path, dtype=torch.float32):
    from dpc_amd import checkpoint as ckpt
    run, x = kind_run(cfg, kind, dtype), dpc_input(cfg)
    state = run["state2"]
    assert state["optimizer_kind"] == kind and list(state)[-1] == "optimizer_kind"
    keys = set(state["optimizer"]["param_groups"][0])
    want = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
    assert keys == set(want([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0])
    fn = str(tmp_path / "epoch1.pth.tar")
    ckpt.save_checkpoint(state, filename=fn)
    b = dpc_engine(cfg, dtype)
    b.set_optimizer(kind)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        info = ckpt.resume(b, fn)
    assert info["epoch"] == 1 and same_bits(arenas(b)[:4], run["steps"][1][:4]) and b.wd == 1e-2
    b.train_step(x)
    assert same_bits(arenas(b), run["steps"][2])
    # another rule at resume: one warning, and the caller's rule stays
    other = "lamb" if kind == "adamw" else "adamw"
    for mine in (other, "adam"):
        c = dpc_engine(cfg, dtype)
        c.set_optimizer(mine)
        with pytest.warns(UserWarning, match="written under the optimizer") as rec:
            ckpt.resume(c, fn)
        assert len([w for w in rec if "written under the optimizer" in str(w.message)]) == 1 and c.optimizer_kind == mine
    # a file without the entry (every Adam run's): silent under any rule; an Adam engine writes none
    fn2 = str(tmp_path / "plain.pth.tar")
    ckpt.save_checkpoint({k: v for k, v in state.items() if k != "optimizer_kind"}, filename=fn2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ckpt.resume(b, fn2)
        ckpt.resume(dpc_engine(cfg, dtype), fn2)
    assert "optimizer_kind" not in ckpt.build_state(dpc_engine(cfg, dtype), 1, "resnet18", 0.0, 2)
    # adopt_optimizer_state carries the rule
    f = dpc_engine(cfg, dtype)
    f.load_params(b.state_dict())
    f.adopt_optimizer_state(b)
    assert f.optimizer_kind == kind and f._baked_scalars() == b._baked_scalars()


def fake_grads(eng, seed):
    g = torch.Generator().manual_seed(seed)
    eng.flat_g.copy_((torch.randn(eng.numel, generator=g) * 0.01).to(eng.device))


def case_torch_adamw_continuation(cfg: Cfg, tmp_path):
    """an adamw file continues in torch.optim.AdamW and a torch.optim.AdamW file continues here, as the Adam round trip does
    (tests/test_checkpoint.py): the next step on both sides, same gradient, to 2e-7"""
    import torch.nn as nn
    from dpc_amd import checkpoint as ckpt
    from dpc_amd.model import DPC_RNN
    lr, wd = 1e-3, 1e-2

    def torch_side():
        m = DPC_RNN(sample_size=cfg.size, num_seq=cfg.N, seq_len=cfg.SL, pred_step=cfg.P, network="resnet18", widths=cfg.widths)
        model = nn.DataParallel(m)
        return model, torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=wd)

    eng = dpc_engine(cfg)
    eng.lr, eng.wd = lr, wd
    eng.set_optimizer("adamw")
    for s in (1, 2):
        fake_grads(eng, s)
        eng.adam_step()
    fn = str(tmp_path / "epoch3.pth.tar")
    ckpt.save_checkpoint(ckpt.build_state(eng, 3, "resnet18", 0.25, 7), filename=fn)
    model, optimizer = torch_side()
    ck = torch.load(fn, map_location="cpu", weights_only=False)
    model.load_state_dict(ck["state_dict"])
    optimizer.load_state_dict(ck["optimizer"])
    named = dict(model.module.named_parameters())
    fake_grads(eng, 3)
    for k in eng.PRM:
        named[k].grad = eng.G[k].detach().clone().to(named[k].device)
    optimizer.step()
    eng.adam_step()
    for k in eng.PRM:
        assert (named[k].detach().cpu() - eng.PRM[k].cpu()).abs().max().item() < 2e-7, k
        assert int(optimizer.state[named[k]]["step"]) == 3
    # ... and the other way
    model, optimizer = torch_side()
    from oracle import dpc_oracle as O
    model.module.load_state_dict(O.make_params_pcg("resnet18", cfg.widths), strict=True)
    g = torch.Generator().manual_seed(11)
    for _ in range(2):
        for p in model.parameters():
            p.grad = (torch.randn(p.shape, generator=g) * 0.01).to(p.device)
        optimizer.step()
    fn2 = str(tmp_path / "torch.pth.tar")
    torch.save({"epoch": 5, "net": "resnet18", "state_dict": model.state_dict(), "best_acc": 0.5, "optimizer": optimizer.state_dict(),
                "iteration": 40}, fn2)
    eng2 = dpc_engine(cfg)
    eng2.set_optimizer("adamw")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        info = ckpt.resume(eng2, fn2)
    assert info["epoch"] == 5 and eng2.step_count == 2 and eng2.lr == lr and eng2.wd == wd
    named = dict(model.module.named_parameters())
    grads = {k: torch.randn(eng2.shapes[k], generator=g) * 0.01 for k in eng2.PRM}
    for k in eng2.PRM:
        named[k].grad = grads[k].clone().to(named[k].device)
        eng2.G[k].copy_(grads[k])
    optimizer.step()
    eng2.adam_step()
    for k in eng2.PRM:
        assert (named[k].detach().cpu() - eng2.PRM[k].cpu()).abs().max().item() < 2e-7, k


def case_captured_step(cfg: Cfg, kind: str, dtype=torch.float32):   # HIP device only
    """a captured step replayed against its eager twin, bit for bit, guard + average + schedule on; the optimizer's share of the graph"""
    from dpc_amd.optim import LRSchedule
    x = dpc_input(cfg)
    sched = LRSchedule("cosine", warmup_steps=4, total_steps=9, min_mult=0.1)

    def make(k_):
        e = dpc_engine(cfg, dtype)
        e.wd = 1e-2
        e.set_grad_guard(max_norm=1e30, skip_nonfinite=True)
        e.set_ema(DECAY)
        e.set_lr_schedule(sched)
        e.set_optimizer(k_)
        for _ in range(2):
            e.train_step(x)
        return e

    a, b, plain = make(kind), make(kind), make("adam")
    replay = a.capture_train_step(x.clone(), warmup=0)
    ref = plain.capture_train_step(x.clone(), warmup=0)
    extra = 2 if kind == "lamb" else 0
    assert sum(replay.kernels) == sum(ref.kernels) + extra and replay.kernels[:-1] == ref.kernels[:-1], (replay.kernels, ref.kernels)
    plain.release_captures()
    for i in range(4):
        replay()
        b.train_step(x)
        assert same_bits(arenas(a) + [a.flat_ema], arenas(b) + [b.flat_ema]), f"replay {i + 1}"
    assert a.lr_now() == b.lr_now() and a.lr_now()["k"] == 5 and a.step_count == 6 == int(a.dev_step.item())
    if kind == "lamb":
        assert a.lamb_stats() == b.lamb_stats() and torch.equal(a._lamb["records"], b._lamb["records"])
    a.wd = 2e-2
    with pytest.raises(RuntimeError, match="changed since"):
        replay()
    a.wd = 1e-2
    a.set_optimizer("adam")
    with pytest.raises(RuntimeError, match="changed since"):
        replay()
    a.set_optimizer(kind)
    replay()
    b.train_step(x)
    assert same_bits(arenas(a), arenas(b))
    a.release_captures()


def case_module_boundary(cfg: Cfg, num_class: int = 11, dtype=torch.float32, report=print):
    """two steps of the reference's loop: optim.AdamW against a torch.optim.AdamW replica; optim.LAMB against the f64 recurrence"""
    import lc_loop_cases as lc
    from dpc_amd import optim
    c = lc.Cfg(device=cfg.device, simulator=cfg.simulator, widths=cfg.widths, num_class=num_class, size=cfg.size, B=cfg.B, N=cfg.N, SL=cfg.SL,
               dtype=dtype)
    forced, _ = lc.masks(c)
    x = dpc_input(cfg)
    target = (torch.arange(cfg.B) % num_class).to(cfg.device).view(cfg.B, 1)
    crit = torch.nn.CrossEntropyLoss()
    ma, mb = lc.module(c), lc.module(c)
    for m in (ma, mb):
        m._forced_masks = forced
    oa = optim.AdamW(ma.parameters(), lr=1e-3, weight_decay=1e-2)
    ob = torch.optim.AdamW(mb.parameters(), lr=1e-3, weight_decay=1e-2)
    for i in range(2):
        lc.ref_loop_step(ma, oa, x, target, crit)
        last_a = L.last_kernel(ma.engine.lib)      # (the trace belongs to the library, which both modules share)
        lc.ref_loop_step(mb, ob, x, target, crit)
        lc.assert_params_agree(ma, mb, f"step {i + 1}")
        lc.same_start(ma, mb)
    assert ma.engine.optimizer_kind == "adamw" and "adamw_" in last_a, last_a
    assert oa.state_dict()["param_groups"][0].keys() == ob.state_dict()["param_groups"][0].keys()
    assert optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).defaults["weight_decay"] == 1e-2
    # LAMB
    ml = lc.module(c)
    ml._forced_masks = forced
    ol = optim.LAMB(ml.parameters(), lr=1e-3, weight_decay=1e-2, exclude_1d=True)
    eng = None
    for i in range(2):
        if eng is not None:
            before = snapshot(eng)
        lc.ref_loop_step(ml, ol, x, target, crit)
        if eng is None:      # the first forward makes the engine: the first step is checked from the module's initial parameters
            eng = ml.engine
            assert eng.optimizer_kind == "lamb" and eng.optimizer_exclude_1d
            continue
        segs, adapt, names = eng_segs(eng, None, exclude_1d=True)
        check_step(eng, "lamb", before, segs, adapt, names, what=f"optim.LAMB step {i + 1}", report=report)
    stats = eng.lamb_stats()
    assert all(v[2] == 1.0 for k, v in stats.items() if len(eng.shapes[k]) <= 1) and any(v[2] != 1.0 for v in stats.values())
    with pytest.raises(TypeError):
        optim.AdamW(ma.parameters(), exclude_1d=True)


# ---------------------------------------------------------------------- entries (simulator)
COMMON = sc.COMMON


def case_entry_main(emu, widths, capsys, tmp_path):
    from dpc_amd import main as dpc_main
    base = COMMON + ["--pred_step", "1", "--synthetic", "2", "--epochs", "1", "--lr", "1e-3", "--wd", "1e-2"]
    outs = {}
    for kind, extra in (("adam", []), ("adamw", ["--optimizer", "adamw"]), ("lamb", ["--optimizer", "lamb", "--wd_exclude_1d"])):
        d = str(tmp_path / kind)
        dpc_main.main(base + extra + ["--save_dir", d], _simulator=emu, _widths=widths)
        outs[kind] = capsys.readouterr().out
        ck = torch.load(os.path.join(d, "epoch1.pth.tar"), map_location="cpu", weights_only=False)
        assert ck.get("optimizer_kind") == (None if kind == "adam" else kind)
    assert "Optimizer" not in outs["adam"] and "LAMB" not in outs["adam"]
    assert outs["adamw"].count("Optimizer: adamw\n") == 1 and "LAMB" not in outs["adamw"]
    assert outs["lamb"].count("Optimizer: lamb, wd_exclude_1d\n") == 1
    assert len(re.findall(r"^LAMB: trust ratio min \S+ median \S+ max \S+$", outs["lamb"], re.M)) == 1, outs["lamb"]
    # the lines every run prints keep their format (the numbers differ with the rule); the first step's loss does not depend on it
    shape = lambda out: [re.sub(r"[-+]?\d+\.\d+(e[-+]\d+)?", "#", ln) for ln in out.splitlines() if not ln.startswith(("Optimizer", "LAMB"))]   # noqa: E731
    assert shape(outs["adamw"]) == shape(outs["adam"]) == shape(outs["lamb"])
    first = lambda out: [ln for ln in out.splitlines() if ln.startswith("Epoch: [0][0/2]")][0].split(" T:")[0]   # noqa: E731
    assert first(outs["adam"]) == first(outs["adamw"]) == first(outs["lamb"])
    # --resume under another rule warns once; under the same rule it is silent
    fn = os.path.join(str(tmp_path / "lamb"), "epoch1.pth.tar")
    for flags, n_warn in ((["--optimizer", "lamb", "--wd_exclude_1d"], 0), (["--optimizer", "adamw"], 1), ([], 1)):
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            dpc_main.main(base + flags + ["--resume", fn], _simulator=emu, _widths=widths)
        assert len([w for w in rec if "written under the optimizer" in str(w.message)]) == n_warn, [str(w.message) for w in rec]
        assert "=> loaded resumed checkpoint" in capsys.readouterr().out


def case_entry_lc(emu, widths, capsys, tmp_path, graph: bool = False):
    """lc_main under lamb: epochs 60 and 61 of the ucf101 / 64 px epoch schedule, the second at lr / 10 (with --graph: on a new capture
    that carries the rule)"""
    from dpc_amd import lc_main
    d = str(tmp_path / "lc")
    n = 3 if graph else 2
    argv = COMMON + ["--synthetic", str(n), "--train_what", "head", "--start-epoch", "60", "--epochs", "62", "--lr", "1e-3", "--save_dir", d,
                     "--optimizer", "lamb", "--wd_exclude_1d"] + (["--graph"] if graph else [])
    lc_main.main(argv, _simulator=emu, _widths=widths)
    out = capsys.readouterr().out
    assert out.count("Optimizer: lamb, wd_exclude_1d\n") == 1, out
    assert len(re.findall(r"^LAMB: trust ratio min \S+ median \S+ max \S+$", out, re.M)) == 2, out
    lines = [ln for ln in out.splitlines() if ln.startswith("Epoch: [")]
    assert [float(re.search(r"\t lr (\S+)$", ln).group(1)) for ln in lines] == [1e-3] * n + [1e-4] * n, lines
    if graph:
        assert len(re.findall(r"^Graph replay: (\d+) steps", out, re.M)) == 2
    ck = torch.load(os.path.join(d, "epoch62.pth.tar"), map_location="cpu", weights_only=False)
    assert ck["optimizer_kind"] == "lamb" and abs(ck["optimizer"]["param_groups"][-1]["lr"] - 1e-4) < 1e-12
    if not graph:
        lc_main.main(COMMON + ["--synthetic", "1", "--train_what", "head", "--epochs", "1", "--optimizer", "adamw"], _simulator=emu, _widths=widths)
        out = capsys.readouterr().out
        assert out.count("Optimizer: adamw\n") == 1 and "LAMB" not in out
        lc_main.main(COMMON + ["--synthetic", "1", "--train_what", "head", "--epochs", "1"], _simulator=emu, _widths=widths)
        out = capsys.readouterr().out
        assert "Optimizer" not in out and "LAMB" not in out


def case_flag_errors(emu, widths):
    from dpc_amd import entry, lc_main, main as dpc_main
    started = []
    real = entry.launch
    for mod in (dpc_main, lc_main):
        mod.launch = lambda *a, **kw: started.append(a)      # a rank that started would show here
    try:
        for mod, extra in ((dpc_main, ["--pred_step", "1"]), (lc_main, ["--train_what", "head"])):
            base = COMMON + extra + ["--synthetic", "1", "--epochs", "1"]
            for bad in (["--wd_exclude_1d"], ["--optimizer", "adam", "--wd_exclude_1d"]):
                with pytest.raises(ValueError, match="wd_exclude_1d"):
                    mod.main(base + bad, _simulator=emu, _widths=widths)
            with pytest.raises(SystemExit):
                mod.main(base + ["--optimizer", "lars"], _simulator=emu, _widths=widths)
        assert not started
    finally:
        for mod in (dpc_main, lc_main):
            mod.launch = real


def case_two_ranks(emu, widths, tmp_path):
    from dpc_amd import main as dpc_main
    pr = str(tmp_path / "probe")
    os.makedirs(pr)
    dpc_main.main(["--net", "resnet18", "--img_dim", "64", "--batch_size", "2", "--gpu", "0,1", "--synthetic", "2", "--print_freq", "1",
                   "--dtype", "bf16", "--num_seq", "4", "--pred_step", "1", "--epochs", "1", "--optimizer", "lamb", "--wd", "1e-2"],
                  _simulator=emu, _widths=widths, _probe=pr)
    r = [torch.load(os.path.join(pr, f"rank{i}.pt")) for i in range(2)]
    assert same(r[0]["flat_p"], r[1]["flat_p"]) and same(r[0]["flat_m"], r[1]["flat_m"])
    assert all(x["step"] == 2 for x in r) and torch.isfinite(r[0]["flat_p"]).all()
