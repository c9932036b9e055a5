"""Negative classes in the loss (csrc/loss_cls.hip: dpc_ce_topk_cls / dpc_ce_topk_bf16_cls; DPCEngine.set_neg_classes; main --neg_weight /
--neg_report), shared by the CPU tier (host SIMT simulator, tests/test_negcls_emu.py) and the GPU tier (tests/test_negcls_gpu.py).

Kernel data is exact by construction, as loss_cases does it: every logit is a multiple of 1/4 in [-2, 2] (a value of f32 and bf16 alike),
so max, rank and every comparison are integer facts and the only rounding left is that of exp, the sums and log.  The class of a column
comes from dpc_mask_gen's own output (1 / -3 / -1 / 0), never from a second closed form.

Bounds (no tolerance constants):
  class map        the non-zero columns of dS under (1,0,0) / (0,1,0) / (0,0,1) are the class's columns and the target (alone in its
                   softmax the target's p - 1 is 0 up to two f32 roundings next to 1)
  loss term        QUARTER (loss_cases) of the smallest change to log Z_r that giving any single column of the row another class's
                   weight makes
  gradient         per element QUARTER of the smallest change such a swap makes to that column's probability, over rows (the target's
                   element: of any single swap in the row, plus 2^-23 / rows for the two f32 roundings of (p - 1) / rows next to 1); a
                   bf16 element 2^-8 of itself more (loss_cases)
  (1, 1, 1)        bit identity to dpc_ce_topk / dpc_ce_topk_bf16 / their _ext forms
  report           counts: equality, and S + T + E = rank; shares: 8 * 2^-24 plus QUARTER of the smallest probability change of the row;
                   their sum within 8 * 2^-24 of 1; the finalised means within rows * 2^-24 of the f64 means of the rows
  bank             the loss bound (bank columns included) for Z and lse_out (plus two f32 spacings); dpc_negq_bwd on that lse_out:
                   negq_cases' backward bound with the kernel's lse as the reference's input (negq_cases.case_bwd), and against the f64
                   weighted share the same bound plus the counted f32 roundings of lse_out (a few 2^-24), which lse_out itself is held to"""
import functools
import re
import warnings
from collections import namedtuple

import numpy as np
import pytest
import torch

import grad_guard_cases as gc
import kcases as kc
import loss_cases as lc
import negq_cases as nq
from dpc_amd import _lib as L
from kcases import K

F32, BF16 = torch.float32, torch.bfloat16
QUARTER, GUARD = lc.QUARTER, lc.GUARD
Cfg = gc.Cfg
bits = lc._bits
_t = lc._t
EPS24 = 2.0 ** -24

# (B, P, SQ): R = 27 the three-sweep kernel; 16 and 96 f32 units; 392 = 4 * 98: windows at 98 / 196 / 294 cut 16-byte units of 4 and of 8;
# (1, 2, 4) has no easy class, (4, 1, 16) no temporal one
GEOMS = ((3, 3, 3), (2, 2, 4), (2, 3, 16), (4, 2, 49), (1, 2, 4), (4, 1, 16))
GEOM_GPU = (11, 3, 256)   # cols 8 448: ce_row_vec<., 16, .> and ce_row_vec16<8>; 800 rows reach past the first window
ROWS_GPU = 800
WEIGHTS = (0.5, 2.0, 0.25)


def rows_of(geom):
    return ROWS_GPU if geom == GEOM_GPU else geom[0] * geom[1] * geom[2]


def desc(geom, w, flags=0, reserved=0.0):
    return L.NegClasses(geom[0], geom[1], geom[2], flags, w[0], w[1], w[2], reserved)


def geometry_of(cols):
    """some (B, P, SQ) with B P SQ = cols for the shapes of loss_cases (at weights (1, 1, 1) any of them gives the same bits)"""
    def factor(n):
        for f in (7, 5, 3, 2):
            if n % f == 0 and n > f:
                return f
        return n
    sq = factor(cols)
    p = factor(cols // sq) if cols // sq > 1 else 1
    return (cols // sq // p, p, sq)


# ---------------------------------------------------------------------------------------------------------------- data and reference
_MASKS = {}


def mask_of(k: K, geom):
    """dpc_mask_gen's output as [R][R] int8 on the host, once per device and geometry"""
    key = (k.dev.type, geom)
    if key not in _MASKS:
        B, P, SQ = geom
        R = B * P * SQ
        m = k.t(torch.full((R * R,), 77, dtype=torch.int8))
        k.call("dpc_mask_gen", m, B, P, SQ)
        k.sync()
        a = m.cpu().numpy().reshape(R, R)
        a.setflags(write=False)
        _MASKS[key] = a
    return _MASKS[key]


@functools.lru_cache(maxsize=None)
def logits(geom, hot=None):
    """[rows][R] multiples of 1/4 in [-2, 2]; in every row one column of each class present is set to the target's value (a tie is never
    counted) and one to 1/4 above it.  hot = "S" / "T": one column of that class per row holds 62, 60 above every other logit."""
    B, P, SQ = geom
    R, W, rows = B * P * SQ, P * SQ, rows_of(geom)
    rng = np.random.Generator(np.random.PCG64(31 * R + SQ))
    S = rng.integers(-8, 9, (rows, R)) / 4.0
    for r in range(rows):
        w0, s = r // W * W, r % SQ
        own = np.arange(w0, w0 + W)
        cands = {"T": [c for c in own if c % SQ == s and c != r], "S": [c for c in own if c % SQ != s],
                 "E": [c for c in (w0 - 1, w0 + W, (r + R // 2) % R) if 0 <= c < R and not (w0 <= c < w0 + W)]}
        for name, cs in cands.items():
            if cs:
                S[r, cs[0]] = S[r, r]
                if len(cs) > 1 and S[r, r] < 2.0:
                    S[r, cs[-1]] = S[r, r] + 0.25
        if hot is not None:
            S[r, cands[hot][len(cands[hot]) // 2]] = 62.0
    S.setflags(write=False)
    return S


Ref = namedtuple("Ref", "term lbound rank grad gbound pbound share count Z mx allS allW")


def reference(S, cls, w, rows_div, Sq=None):
    """f64 of the weighted loss: S [rows][R], cls the rows of dpc_mask_gen's output, w = (w_S, w_T, w_E), Sq [rows][Q] the bank's logits
    (easy).  rows_div: the gradient's 1 / rows."""
    rows, R = S.shape
    wS, wT, wE = w
    Wm = np.select([cls == 1, cls == -3, cls == -1], [1.0, wS, wT], wE)
    kind = np.select([cls == 1, cls == -3, cls == -1], [0, 1, 2], 3)   # 0 positive, 1 spatial, 2 temporal, 3 easy
    if Sq is not None and Sq.shape[1]:
        allS, allW = np.concatenate([S, Sq], 1), np.concatenate([Wm, np.full(Sq.shape, wE)], 1)
        kind = np.concatenate([kind, np.full(Sq.shape, 3)], 1)
    else:
        allS, allW = S, Wm
    idx = np.arange(rows)
    assert (cls[idx, idx] == 1).all() and (cls == 1).sum() == rows
    tgt = S[idx, idx]
    mx = np.where(allW > 0, allS, -np.inf).max(1)
    e = np.exp(allS - mx[:, None])
    we = allW * e
    Z = we.sum(1)
    p = we / Z[:, None]
    term = np.log(Z) + mx - tgt
    above = allS > tgt[:, None]
    rank = above.sum(1)
    grad = p[:, :R].copy()
    grad[idx, idx] -= 1.0
    grad /= rows_div
    share = np.stack([np.where(kind == j, p, 0.0).sum(1) for j in range(4)], 1)
    count = np.stack([(above & (kind == j)).sum(1) for j in (1, 2, 3)], 1).astype(np.float64)
    # what one column under another class's weight changes
    nontgt = np.ones(allS.shape, bool)
    nontgt[idx, idx] = False
    dl = np.full(rows, np.inf)
    dp = np.full(allS.shape, np.inf)
    dt = np.full(rows, np.inf)
    for a in sorted(set(w)):
        ok = nontgt & (allW != a)
        delta = (a - allW) * e
        Zp = Z[:, None] + delta
        dl = np.minimum(dl, np.where(ok, np.abs(np.log1p(delta / Z[:, None])), np.inf).min(1))
        dp = np.minimum(dp, np.where(ok, np.abs(a * e / Zp - p), np.inf))
        dt = np.minimum(dt, np.where(ok, np.abs(p[idx, idx][:, None] * (Z[:, None] / Zp - 1.0)), np.inf).min(1))
    pbound = QUARTER * dp.min(1)
    gbound = QUARTER * dp[:, :R] / rows_div
    # the target's element is p - 1, formed in f32 next to 1 (spacing 2^-24 below it) and scaled by 1 / rows: two roundings at that size,
    # whatever the swap does to p (negq_cases.hand_reference's diagonal term)
    gbound[idx, idx] = QUARTER * dt / rows_div + 2.0 ** -23 / rows_div
    return Ref(term, QUARTER * dl, rank, grad, gbound, pbound, share, count, Z, mx, allS, allW)


Run = namedtuple("Run", "out lse rrows rep")


def run_cls(k: K, S, sdt, gdt, geom, w, qs=None, report=True, with_grad=True):
    """one call of the entry the logits' dtype selects; every output poisoned, guard bands behind dscore, lse_out and the report"""
    rows, R = S.shape
    E = 8 if (gdt == BF16 or sdt == BF16) else 4
    ld_d = (R + E - 1) // E * E
    out = lc.Out(k, rows, ld_d, gdt if with_grad else None)
    lse = k.poison(rows + GUARD) if qs is not None else None
    rrows, rep = (k.poison(rows * 8 + GUARD), k.poison(8 + GUARD)) if report else (None, None)
    sdev = k.t(_t(S), sdt)
    if sdt == BF16:
        k.call("dpc_ce_topk_bf16_cls", sdev, rows, R, R, out.ws, out.res, out.d, ld_d, qs, lse, desc(geom, w), rrows, rep)
    else:
        k.call("dpc_ce_topk_cls", sdev, rows, R, R, out.ws, out.res, out.d, L.dtype_code(gdt), ld_d, qs, lse, desc(geom, w), rrows, rep)
    k.sync()
    out.guard_untouched()
    if report:
        assert bool(torch.isnan(rrows[rows * 8:]).all()) and bool(torch.isnan(rep[8:]).all()), "written past the report"
    if lse is not None:
        assert bool(torch.isnan(lse[rows:]).all())
    return Run(out, lse, None if rrows is None else rrows[:rows * 8].view(rows, 8), None if rep is None else rep[:8])


def arms_of(geom):
    """(logits dtype, gradient dtype): f32 logits with either gradient everywhere, bf16 logits where the entry serves the width"""
    R = geom[0] * geom[1] * geom[2]
    return [(F32, F32), (F32, BF16)] + ([(BF16, BF16)] if R % 8 == 0 else [])


def check_loss_grad(tag, run, ref, gdt, report=print):
    rows, R = ref.grad.shape
    kc.all_finite(run.out.ws, run.out.res)
    w = run.out.ws.cpu().numpy().astype(np.float64)
    assert np.array_equal(w[:, 1], ref.rank.astype(np.float64)), f"{tag}: rank differs on rows {np.nonzero(w[:, 1] != ref.rank)[0][:8].tolist()}"
    et = np.abs(w[:, 0] - ref.term)
    g = run.out.d[:, :R].float().cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all()
    gb = ref.gbound + (2.0 ** -8 * np.abs(ref.grad) if gdt == BF16 else 0.0)
    eg = np.abs(g - ref.grad)
    report(f"[negcls] {tag}: loss {float((et / ref.lbound).max()):.3g}, gradient {float((eg / gb).max()):.3g} of their bounds "
           f"(smallest loss bound {float(ref.lbound.min()):.3g})")
    assert (et < ref.lbound).all(), f"{tag}: loss term of rows {np.nonzero(~(et < ref.lbound))[0][:8].tolist()}, worst {float((et / ref.lbound).max()):.3g} of the bound"
    assert (eg <= gb).all(), f"{tag}: {int((~(eg <= gb)).sum())} gradient elements outside the bound, worst {float((eg / gb).max()):.3g}"
    assert (g[ref.allW[:, :R] == 0] == 0).all(), f"{tag}: a column of weight 0 has a gradient"
    if run.out.d.shape[1] > R:
        assert float(run.out.d[:, R:].float().abs().max()) == 0.0
    r = run.out.res.cpu().numpy()
    for i, kk in enumerate((1, 3, 5)):
        assert r[1 + i] == np.float32(int((ref.rank < kk).sum())) / np.float32(rows)
    assert abs(float(r[0]) - ref.term.mean()) < ref.lbound.max() + rows * EPS24 * np.abs(ref.term).mean()


# ---------------------------------------------------------------------------------------------------------------- K1 class map
def case_class_map(k: K, geom):
    S, cls = logits(geom), mask_of(k, geom)[:rows_of(geom)]
    rows, R = S.shape
    for w, value in (((1.0, 0.0, 0.0), -3), ((0.0, 1.0, 0.0), -1), ((0.0, 0.0, 1.0), 0)):
        want = cls == value
        some = want.any(1)
        idx = np.arange(rows)
        for sdt, gdt in arms_of(geom):
            run = run_cls(k, S, sdt, gdt, geom, w, report=False)
            d = run.out.d[:, :R].float().cpu().numpy()
            got = d != 0
            # the target's own element is p - 1: not 0 where the class has a column in the row; alone in its softmax p is 1 up to the
            # two roundings of e / sum(e) (the v_exp_f32 form does not give exp(0) = 1 exactly)
            assert got[idx, idx][some].all() and (np.abs(d[idx, idx][~some]) <= 2.0 ** -22 / rows).all(), f"{geom} {w}: the target's element"
            got[idx, idx] = False
            assert np.array_equal(got, want), f"{geom} {w} {sdt} {gdt}: rows {np.nonzero((got != want).any(1))[0][:8].tolist()}"


# ---------------------------------------------------------------------------------------------------------------- K2 loss and gradient
def case_weighted(k: K, geom, report=print):
    S, cls = logits(geom), mask_of(k, geom)[:rows_of(geom)]
    rows, R = S.shape
    ref = reference(S, cls, WEIGHTS, rows)
    # the same reference with one column of every row under another class's weight misses the row
    rng = np.random.Generator(np.random.PCG64(R))
    cols = (np.arange(rows) + 1 + rng.integers(0, R - 1, rows)) % R
    wrong = np.array(cls)
    wrong[np.arange(rows), cols] = np.where(cls[np.arange(rows), cols] == 0, -3, np.where(cls[np.arange(rows), cols] == -3, -1, 0))
    wrong[np.arange(rows), np.arange(rows)] = 1
    Wm = np.select([wrong == 1, wrong == -3, wrong == -1], [1.0, WEIGHTS[0], WEIGHTS[1]], WEIGHTS[2])
    mis = np.log((Wm * np.exp(S - ref.mx[:, None])).sum(1)) + ref.mx - S[np.arange(rows), np.arange(rows)]
    assert (np.abs(mis - ref.term) > ref.lbound).all(), "a mis-classed column stays inside the bound"
    for sdt, gdt in arms_of(geom):
        run = run_cls(k, S, sdt, gdt, geom, WEIGHTS, report=False)
        check_loss_grad(f"{geom} {'bf16' if sdt == BF16 else 'f32'} logits, {'bf16' if gdt == BF16 else 'f32'} gradient", run, ref, gdt, report)


# ---------------------------------------------------------------------------------------------------------------- K3 (1, 1, 1)
@functools.lru_cache(maxsize=None)
def bank_stats(rows):
    """per-row statistics of a real bank (negq_cases.bank_data, every slot live), repeated down the rows"""
    bank = nq.bank_data(24, 32, 3)
    r = nq.queue_ref(bank, [0, 1, 2])
    i = np.arange(rows) % 24
    return torch.from_numpy(np.stack([r.m[i], r.l[i], r.rk[i], np.zeros(rows)], 1).astype(np.float32))


def case_ones_is_the_old_entry(k: K, entry, name, mode, bank):
    """one shape of loss_cases.CE_SHAPES / CE16_SHAPES: weights (1, 1, 1) against the older entry (its _ext form with a bank), bit for
    bit, report written or not.  Modes as negq_cases.case_ext_empty."""
    bf_logits = entry == "dpc_ce_topk_bf16"
    cols, ld, ld_d, off = (lc.CE16_SHAPES if bf_logits else lc.CE_SHAPES)[name]
    rc = lc.row_case(cols, 8 if bf_logits else 4, square="square" in name)
    rows = rc.s.shape[0]
    ld, ld_d = ld or cols, ld_d or cols
    keep, sview = lc._strided(k, rc.s, ld, BF16 if bf_logits else F32, off)
    gdt = {"f32": F32, "bf16": BF16}.get(mode)
    code = L.dtype_code(F32 if mode in ("f32", "null") else BF16)
    geom = geometry_of(cols)
    d = desc(geom, (1.0, 1.0, 1.0))
    qs = k.t(bank_stats(rows)) if bank else None
    old = lc.Out(k, rows, ld_d, gdt)
    old_lse = k.poison(rows + GUARD) if bank else None
    if bank:
        if bf_logits:
            k.call(entry + "_ext", sview, rows, cols, ld, old.ws, old.res, old.d, ld_d, qs, old_lse)
        else:
            k.call(entry + "_ext", sview, rows, cols, ld, old.ws, old.res, old.d, code, ld_d, qs, old_lse)
        k.sync()
    else:
        lc._launch(k, entry, sview, rows, cols, ld, old, code)
    for report in (False, True):
        new = lc.Out(k, rows, ld_d, gdt)
        lse = k.poison(rows + GUARD) if bank else None
        rrows, rep = (k.poison(rows * 8), k.poison(8)) if report else (None, None)
        if bf_logits:
            k.call(entry + "_cls", sview, rows, cols, ld, new.ws, new.res, new.d, ld_d, qs, lse, d, rrows, rep)
        else:
            k.call(entry + "_cls", sview, rows, cols, ld, new.ws, new.res, new.d, code, ld_d, qs, lse, d, rrows, rep)
        k.sync()
        tag = f"{entry}_cls {name} {mode} bank={bank} report={report}"
        assert torch.equal(bits(new.ws), bits(old.ws)) and torch.equal(bits(new.res), bits(old.res)), f"{tag}: other bits"
        if gdt is not None:
            assert torch.equal(bits(new.dbuf), bits(old.dbuf)), f"{tag}: other gradient bits"
        if bank:
            assert torch.equal(bits(lse), bits(old_lse)), f"{tag}: other lse_out bits"
        if report:
            kc.all_finite(rrows, rep)
            rr = rrows.view(rows, 8).cpu().numpy().astype(np.float64)
            assert np.array_equal(rr[:, 4:7].sum(1), new.ws[:, 1].cpu().numpy().astype(np.float64)) and (rr[:, 7] == 0).all()
            assert (np.abs(rr[:, :4].sum(1) - 1.0) <= 8 * EPS24).all(), float(np.abs(rr[:, :4].sum(1) - 1.0).max())
    del keep


# ---------------------------------------------------------------------------------------------------------------- K4 a hot column of weight 0
def case_hot_zero(k: K, geom, report=print):
    which = "T" if geom[1] > 1 else "S"
    w = (0.5, 0.0, 0.25) if which == "T" else (0.0, 2.0, 0.25)
    S, cls = logits(geom, which), mask_of(k, geom)[:rows_of(geom)]
    rows, R = S.shape
    ref = reference(S, cls, w, rows)
    assert (ref.mx <= 2.0).all() and (S.max(1) == 62.0).all() and (ref.rank >= 1).all()
    for sdt, gdt in arms_of(geom):
        run = run_cls(k, S, sdt, gdt, geom, w, report=False)
        check_loss_grad(f"{geom} hot {which} {'bf16' if sdt == BF16 else 'f32'} logits, {'bf16' if gdt == BF16 else 'f32'} gradient", run, ref, gdt, report)
        g = run.out.d[:, :R].float().cpu().numpy()
        assert (g[S == 62.0] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- K5 report
def check_report(tag, run, ref, report=print):
    rows = ref.term.shape[0]
    kc.all_finite(run.rrows, run.rep)
    rr = run.rrows.cpu().numpy().astype(np.float64)
    assert np.array_equal(rr[:, 4:7], ref.count), f"{tag}: counts differ on rows {np.nonzero((rr[:, 4:7] != ref.count).any(1))[0][:8].tolist()}"
    assert np.array_equal(rr[:, 4:7].sum(1), run.out.ws[:, 1].cpu().numpy().astype(np.float64)) and (rr[:, 7] == 0).all()
    got = rr[:, [0, 1, 2, 3]]
    want = ref.share[:, [0, 1, 2, 3]]   # positive, spatial, temporal, easy
    e = np.abs(got - want)
    b = (8 * EPS24 + ref.pbound)[:, None]
    report(f"[negcls] {tag}: shares {float((e / b).max()):.3g} of their bound, sum off by {float(np.abs(got.sum(1) - 1).max()):.3g}")
    assert (e <= b).all(), f"{tag}: shares of rows {np.nonzero((e > b).any(1))[0][:8].tolist()}"
    assert (np.abs(got.sum(1) - 1.0) <= 8 * EPS24).all()
    m = run.rep.cpu().numpy().astype(np.float64)
    means = np.concatenate([rr[:, :4].mean(0), (rr[:, 4:7] > 0).mean(0)])
    assert (np.abs(m[:7] - means) <= rows * EPS24).all() and m[7] == 0, (m.tolist(), means.tolist())
    # ... and of the f64 reference's: the mean of the rows' share bounds more
    assert (np.abs(m[:4] - ref.share.mean(0)) <= rows * EPS24 + float(b.mean())).all(), (m[:4].tolist(), ref.share.mean(0).tolist())
    for j in range(3):   # the fractions are quotients of small integers
        assert np.float32(m[4 + j]) == np.float32(int((ref.count[:, j] > 0).sum())) / np.float32(rows)


def case_report(k: K, geom, report=print):
    S, cls = logits(geom), mask_of(k, geom)[:rows_of(geom)]
    rows = S.shape[0]
    ref = reference(S, cls, WEIGHTS, rows)
    for sdt, gdt in arms_of(geom):
        run = run_cls(k, S, sdt, gdt, geom, WEIGHTS, report=True)
        check_report(f"{geom} {'bf16' if sdt == BF16 else 'f32'} logits", run, ref, report)
        plain = run_cls(k, S, sdt, gdt, geom, WEIGHTS, report=False)   # the report changes no other output
        assert torch.equal(bits(plain.out.ws), bits(run.out.ws)) and torch.equal(bits(plain.out.dbuf), bits(run.out.dbuf))
        rows_only = k.poison(rows * 8)   # report_rows without the means
        out = lc.Out(k, rows, run.out.ld_d, gdt)
        if sdt == BF16:
            k.call("dpc_ce_topk_bf16_cls", k.t(_t(S), sdt), rows, S.shape[1], S.shape[1], out.ws, out.res, out.d, out.ld_d, None, None,
                   desc(geom, WEIGHTS), rows_only, None)
        else:
            k.call("dpc_ce_topk_cls", k.t(_t(S), sdt), rows, S.shape[1], S.shape[1], out.ws, out.res, out.d, L.dtype_code(gdt), out.ld_d, None,
                   None, desc(geom, WEIGHTS), rows_only, None)
        k.sync()
        assert torch.equal(bits(rows_only.view(rows, 8)), bits(run.rrows))


# ---------------------------------------------------------------------------------------------------------------- K6 bank
BANK_SHAPES = (((2, 3, 4), 32, 3), ((2, 4, 25), 32, 2))   # R = 24 and 200 of negq_cases.KERNEL_SHAPES, as geometries


def case_bank(k: K, geom, D, Kk, report=print):
    R = geom[0] * geom[1] * geom[2]
    bank = nq.bank_data(R, D, Kk)
    sd = bank.sd
    live = list(range(Kk))
    qref = nq.queue_ref(bank, live)
    ring, ringT = nq.make_ring(k, bank, live)
    st = nq.make_state(k, Kk, Kk)
    qs = nq.run_fwd(k, bank, ring, st, nq.target_of(k, bank, F32), F32).contiguous()
    cls = mask_of(k, geom)
    Q = np.concatenate([bank.keys[s] for s in live], 0)
    _, _, nslab = nq.ws_sizes(k, R, D, Kk)
    for wE in (0.25, 2.0):
        w = (0.5, 2.0, wE)
        ref = reference(sd.S, cls, w, R, qref.Sq)
        lse_want = np.log(ref.Z) + ref.mx - np.log(wE)
        for sdt, gdt in arms_of(geom):
            run = run_cls(k, sd.S, sdt, gdt, geom, w, qs=qs, report=True)
            tag = f"bank {geom} w_E {wE} {'bf16' if sdt == BF16 else 'f32'} logits, {'bf16' if gdt == BF16 else 'f32'} gradient"
            check_loss_grad(tag, run, ref, gdt, report)
            check_report(tag, run, ref, report)
            lse32 = run.lse[:R].cpu()
            el = np.abs(lse32.numpy().astype(np.float64) - lse_want)
            lb = ref.lbound + 2 * np.spacing(np.abs(lse_want).astype(np.float32) + np.float32(2.0))
            assert (el < lb).all(), f"{tag}: lse_out of rows {np.nonzero(~(el < lb))[0][:8].tolist()}"
            got, n = nq.run_bwd(k, bank, ring, ringT, st, lse32)
            kc.all_finite(got)
            g = got.cpu().numpy().astype(np.float64)
            N = len(live) * nq.pitch_of(R) + nslab
            # as negq_cases.case_bwd holds it: the kernel's input as it is, negq_cases' bound and nothing else
            dS_in = np.exp(qref.Sq - lse32.numpy().astype(np.float64)[:, None]) / R
            e_in, b_in = np.abs(g - dS_in @ Q), (2.0 ** -8 + N * EPS24) * (np.abs(dS_in) @ np.abs(Q))
            assert (e_in <= b_in).all(), f"{tag}: {int((~(e_in <= b_in)).sum())} elements of the bank's d_pred outside negq_cases' bound"
            # ... and against the f64 weighted share: the same bound, plus what an lse_out formed in f32 moves exp(s - lse) by -- its
            # roundings, counted from the row kernel: the sum-exp (per thread at most cols / 256 + 1 adds, 6 shuffle steps, 3 adds over
            # the waves, 1 for the bank: each 2^-24 of the sum at most, so of lse absolutely), the exponentials (v_exp_f32 / expf: 2^-23
            # relative), logf (one spacing of its result) and the two additions behind it (+ mx, - log w_E: one spacing each at the
            # size of |lse| + |log w_E|)
            adds = -(-R // 256) + 1 + 6 + 3 + 1
            slack = (adds + 2) * EPS24 + 3 * np.spacing((np.abs(lse_want) + abs(np.log(wE))).astype(np.float32)).astype(np.float64)
            assert (el <= slack).all(), f"{tag}: lse_out is further from f64 than its f32 roundings: {float((el / slack).max()):.3g}"
            dS = wE * np.exp(qref.Sq - ref.mx[:, None]) / ref.Z[:, None] / R          # the f64 weighted share of every bank column
            want, mag = dS @ Q, np.abs(dS) @ np.abs(Q)
            bound = (2.0 ** -8 + N * EPS24 + 2 * slack[:, None]) * mag
            e = np.abs(g - want)
            assert (e <= bound).all(), f"{tag}: {int((~(e <= bound)).sum())} elements of the bank's d_pred outside the bound"
            unweighted = np.abs(g - want / wE) > bound                                # the share without the weight misses it
            report(f"[negcls] {tag}: bank d_pred {float((e[mag > 0] / bound[mag > 0]).max()):.3g} of its bound; unweighted misses "
                   f"{unweighted[mag > 0].mean():.3f} of the elements")
            assert unweighted[mag > 0].mean() > 0.5


# ---------------------------------------------------------------------------------------------------------------- K7 refused calls
def case_refused(k: K):
    geom = (2, 3, 4)
    R = 24
    arg, uns = f"code {L.ERR_ARG}$", f"code {L.ERR_UNSUPPORTED}$"
    s32, s16 = k.zeros(R * R), k.zeros(R * R + 8, dtype=BF16)
    qs = k.t(bank_stats(R))
    outs = dict(ws=k.poison(R * 2 + GUARD), res=k.poison(4 + GUARD), d=k.poison(R * R + GUARD), d16=k.poison(R * R + GUARD, dtype=BF16),
                lse=k.poison(R + GUARD), rr=k.poison(R * 8 + GUARD), rep=k.poison(8 + GUARD))
    before = {n: bits(t) for n, t in outs.items()}
    ws, res, d, d16, lse, rr, rep = (outs[n] for n in ("ws", "res", "d", "d16", "lse", "rr", "rep"))
    ok = (1.0, 1.0, 1.0)

    def c32(desc_, score=s32, ws_=ws, res_=res, qs_=None, lse_=None, rr_=rr, rep_=rep, rows=R, cols=R):
        return lambda: k.call("dpc_ce_topk_cls", score, rows, cols, cols, ws_, res_, d, L.F32, R, qs_, lse_, desc_, rr_, rep_)

    def c16(desc_, score=s16, qs_=None, lse_=None, rr_=rr, rep_=rep, ld=R):
        return lambda: k.call("dpc_ce_topk_bf16_cls", score, R, R, ld, ws, res, d16, R, qs_, lse_, desc_, rr_, rep_)
    bad = [
        (arg, c32(desc((2, 3, 5), ok))),                       # cols != B P SQ
        (arg, c32(desc((0, 3, 8), ok))),
        (arg, c32(desc((-2, -3, 4), ok))),
        (arg, c32(desc(geom, (float("nan"), 1.0, 1.0)))),
        (arg, c32(desc(geom, (1.0, float("inf"), 1.0)))),
        (arg, c32(desc(geom, (1.0, 1.0, -0.5)))),
        (arg, c32(desc(geom, (65537.0, 1.0, 1.0)))),
        (arg, c32(desc(geom, ok, flags=1))),
        (arg, c32(desc(geom, (1.0, 1.0, 0.0)), qs_=qs, lse_=lse)),   # the bank's keys are easy
        (arg, c32(desc(geom, ok), qs_=qs)),                    # qstats / lse_out go together
        (arg, c32(desc(geom, ok), lse_=lse)),
        (arg, c32(desc(geom, ok), rr_=None)),                  # the means need the rows
        (arg, c32(desc(geom, ok), score=None)),
        (arg, c32(desc(geom, ok), ws_=None)),
        (arg, c32(desc(geom, ok), res_=None)),
        (arg, c32(desc(geom, ok), rows=R + 1)),                # cols < rows
        (arg, c16(desc((2, 3, 5), ok))),
        (arg, c16(desc(geom, (1.0, -1.0, 1.0)))),
        (arg, c16(desc(geom, (1.0, 1.0, 0.0)), qs_=qs, lse_=lse)),
        (arg, c16(desc(geom, ok), qs_=qs)),
        (arg, c16(desc(geom, ok), rr_=None)),
        (arg, c16(desc(geom, ok), score=None)),
        (uns, c16(desc(geom, ok), score=s16[4:])),             # 8 bytes off a 16-byte boundary
        (arg, c16(desc((2, 3, 5), ok), score=s16[4:])),        # argument errors come first
    ]
    for code, f in bad:
        with pytest.raises(L.DpcError, match=code):
            f()
    k.sync()
    for n, t in outs.items():
        assert torch.equal(bits(t), before[n]), f"a refused call wrote {n}"
    # the same calls go through once they are right
    c32(desc(geom, ok), qs_=qs, lse_=lse)()
    c16(desc(geom, (0.0, 0.0, 65536.0)))()
    k.sync()
    kc.all_finite(ws[:R * 2], res[:4], rep[:8])
    for n, t in outs.items():
        assert torch.equal(bits(t)[-GUARD:], before[n][-GUARD:]), f"{n}: the guard band was written"


# ================================================================================================================ engine
# r18, num_seq 4, pred_step 2, so that all three classes exist: R = B P SQ = 16 at 64 px (f32 logits) and 64 at 128 px (bf16 logits)
ARMS = {"f32 logits": dict(size=64, B=2), "bf16 logits": dict(size=128, B=2)}
REPORT_CALLS = 0   # C-ABI calls per training step the weights or the report add (the engine's launch count, replay.kernels of a capture):
                   # the _cls entry takes the place of dpc_ce_topk[_bf16][_ext] and launches the report's means (one single-workgroup
                   # kernel) itself


def arm_cfg(cfg: Cfg, arm: str) -> Cfg:
    return Cfg(device=cfg.device, simulator=cfg.simulator, widths=cfg.widths, P=2, **ARMS[arm])


def inputs(cfg: Cfg, count: int):
    shape = gc.dpc_input(cfg).shape
    return [torch.randn(shape, generator=torch.Generator().manual_seed(800 + j)).to(cfg.device) for j in range(count)]


def engine(cfg: Cfg, weights=None, report=False, k_slots=0):
    eng = gc.dpc_engine(cfg, BF16)
    if k_slots:
        eng.set_neg_queue(k_slots)
    if weights is not None or report:
        eng.set_neg_classes(weights or (1, 1, 1), report=report)
    return eng


all_arenas, same = nq.all_arenas, nq.same


def case_off_is_off(cfg: Cfg, arm: str):
    c = arm_cfg(cfg, arm)
    a, b = engine(c), engine(c)
    b.set_neg_classes((0.5, 2, 0.25), report=True)
    assert b.neg_classes == ((0.5, 2.0, 0.25), True) and ("neg_cls", 0.5, 2.0, 0.25, True) in b._baked_scalars()
    b.set_neg_classes()   # the defaults: off
    assert b.neg_classes == ((1.0, 1.0, 1.0), False) == a.neg_classes and b._baked_scalars() == a._baked_scalars()
    with pytest.raises(L.DpcError, match="report is off"):
        b.neg_class_stats()
    la, lb = a._launches, b._launches
    for x in inputs(c, 2):
        ra, rb = a.train_step(x).clone(), b.train_step(x).clone()
        assert torch.equal(bits(ra), bits(rb)) and torch.equal(bits(a.flat_g), bits(b.flat_g)) and same(all_arenas(a), all_arenas(b))
    assert a._launches - la == b._launches - lb


def case_report_only(cfg: Cfg, arm: str):
    c = arm_cfg(cfg, arm)
    a, b = engine(c), engine(c, report=True)
    assert b.neg_classes == ((1.0, 1.0, 1.0), True) and b._baked_scalars() == a._baked_scalars() + (("neg_cls", 1.0, 1.0, 1.0, True),)
    la, lb = a._launches, b._launches
    for x in inputs(c, 2):
        ra, rb = a.train_step(x).clone(), b.train_step(x).clone()
        assert torch.equal(bits(ra), bits(rb)) and torch.equal(bits(a.flat_g), bits(b.flat_g)) and same(all_arenas(a), all_arenas(b))
        assert torch.equal(bits(a.row_ws), bits(b.row_ws)) and torch.equal(bits(a.dscore), bits(b.dscore))
    assert (b._launches - lb) - (a._launches - la) == 2 * REPORT_CALLS
    s = b.neg_class_stats()
    assert list(s) == list(b.NEG_CLASS_KEYS) and abs(sum(s[n] for n in ("mass_pos", "mass_S", "mass_T", "mass_E")) - 1.0) <= 8 * EPS24
    rk = b.row_ws.view(b.R, 2)[:, 1].cpu().numpy()
    rr = b._ncls_rows.cpu().numpy()
    assert np.array_equal(rr[:, 4:7].sum(1), rk)


def hand_reference(eng, pred, finf, s_in, bank_keys, w, bf16_logits):
    """negq_cases.hand_reference with a weight per class: f64 loss terms, ranks, d_pred, d_finf and the report of one training step from
    the step's own score operands, its in-batch logits as the loss kernel read them and the keys the bank held; the same bounds, the
    probabilities being the weighted ones"""
    P, F = pred.double().numpy(), finf.double().numpy()
    R = P.shape[0]
    S = s_in.double().numpy()
    exact = P @ F.T
    tol = (np.abs(P) @ np.abs(F).T) * (2.0 ** -8 if bf16_logits else P.shape[1] * 2.0 ** -23) + 1e-30
    assert (np.abs(S - exact) <= tol).all(), "the in-batch logits are not pred @ finf^T"
    Q = np.concatenate([q.double().numpy() for q in bank_keys], 0) if bank_keys else np.zeros((0, P.shape[1]))
    cls = eng.get_mask().reshape(R, R).cpu().numpy()
    ref = reference(S, cls, w, R, P @ Q.T)
    tgt = np.diagonal(S)
    p = ref.allW * np.exp(ref.allS - ref.mx[:, None]) / ref.Z[:, None]
    dS = p.copy()
    dS[np.arange(R), np.arange(R)] -= 1.0
    dS /= R
    keys = np.concatenate([F, Q], 0)
    N = keys.shape[0] + 64 + 32
    f = 2.0 ** -8 + N * 2.0 ** -24
    lse = np.log(ref.Z) + ref.mx
    big = np.maximum(np.maximum(np.abs(ref.mx), np.abs(tgt)), np.maximum(np.abs(lse), np.abs(ref.term)))
    acc = P.shape[1] * 2.0 ** -24 * (np.abs(P) @ np.abs(Q).T).max(1) if Q.shape[0] else np.zeros(R)
    pmin = np.where(ref.allW > 0, p, np.inf).min(1)
    rbound = QUARTER * -np.log1p(-pmin) + 2.0 ** -24 * 4 * big + acc
    lbound = float(rbound.max()) + 2.0 ** -24 * (-(-R // 256) + 10) * float(np.abs(ref.term).mean())
    diag = 2.0 ** -23 / R
    return dict(ref=ref, loss=float(ref.term.mean()), lbound=lbound, term=ref.term, rbound=rbound, rank=ref.rank,
                d_pred=dS @ keys, b_pred=f * (np.abs(dS) @ np.abs(keys)) + diag * np.abs(F),
                d_finf=dS[:, :R].T @ P, b_finf=f * (np.abs(dS[:, :R]).T @ np.abs(P)) + diag * np.abs(P))


def hand_step(eng, x, bank_keys, w, report, tag, grads=True):
    """one training step taken apart (negq_cases.hand_step) under the class weights, the report included"""
    R, D = eng.R, eng.D
    eng._forward_loss(x, True)
    sp, sf = eng._score_operands()
    pred, finf = sp.detach().reshape(R, D).cpu().clone(), sf.detach().reshape(R, D).cpu().clone()
    s_in = (eng.score16 if eng._score16_live else eng.score).detach().cpu().clone()
    res = eng.result.detach().cpu().clone()
    rows = eng.row_ws.detach().cpu().double().numpy().reshape(R, 2).copy()
    rr = eng._ncls_rows.detach().cpu().double().numpy().copy()
    stats = eng.neg_class_stats()
    ref = hand_reference(eng, pred, finf, s_in, bank_keys, w, eng._score16_live)
    er = np.abs(rows[:, 0] - ref["term"])
    assert (er < ref["rbound"]).all(), (tag, np.nonzero(~(er < ref["rbound"]))[0][:8].tolist(), float((er / ref["rbound"]).max()))
    assert np.array_equal(rows[:, 1], ref["rank"].astype(np.float64)), (tag, np.nonzero(rows[:, 1] != ref["rank"])[0][:8].tolist())
    assert abs(float(res[0]) - ref["loss"]) < ref["lbound"], (tag, float(res[0]), ref["loss"], ref["lbound"])
    for i, kk in enumerate((1, 3, 5)):
        assert float(res[1 + i]) == float(np.float32(int((ref["rank"] < kk).sum())) / np.float32(R)), (tag, kk)
    r = ref["ref"]
    # the report: counts exactly; a share is a quotient of two of the row's sums, each off by at most the row's bound relative to Z
    assert np.array_equal(rr[:, 4:7], r.count) and np.array_equal(rr[:, 4:7].sum(1), rows[:, 1]), tag
    es = np.abs(rr[:, :4] - r.share)
    bs = (8 * EPS24 + 2 * ref["rbound"])[:, None]
    assert (es <= bs).all() and (np.abs(rr[:, :4].sum(1) - 1.0) <= 8 * EPS24).all(), (tag, float((es / bs).max()))
    want = np.concatenate([r.share.mean(0), (r.count > 0).mean(0)])
    got = np.array([stats[n] for n in eng.NEG_CLASS_KEYS])
    assert (np.abs(got[:4] - want[:4]) <= float(bs.max()) + R * EPS24).all() and (np.abs(got[4:] - want[4:]) <= EPS24).all(), (tag, got, want)
    line = f"[negcls-engine] {tag}: {len(bank_keys)} slots live, loss {float(res[0]):.5f} (f64 {ref['loss']:.5f}), rows {float((er / ref['rbound']).max()):.3g}"
    if grads:
        eng.backward()
        d_pred, d_finf = eng.d_pred.detach().reshape(R, D).cpu().double().numpy(), eng.d_finf.detach().reshape(R, D).cpu().double().numpy()
        ep, ef = np.abs(d_pred - ref["d_pred"]), np.abs(d_finf - ref["d_finf"])
        assert (ep <= ref["b_pred"]).all() and (ef <= ref["b_finf"]).all(), (tag, float((ep / ref["b_pred"]).max()), float((ef / ref["b_finf"]).max()))
        line += f", d_pred {float((ep / ref['b_pred']).max()):.3g}, d_finf {float((ef / ref['b_finf']).max()):.3g}"
    report(line + " of their bounds; shares " + "/".join(f"{v:.3f}" for v in got[:4]))
    return finf, ref


def case_by_hand(cfg: Cfg, arm: str, k_slots: int, report=print):
    c = arm_cfg(cfg, arm)
    eng = engine(c, WEIGHTS, report=True, k_slots=k_slots)
    batches = []
    for j, x in enumerate(inputs(c, 4 if k_slots else 2)):
        finf, ref = hand_step(eng, x, nq.live_keys(batches, k_slots) if k_slots else [], WEIGHTS, report, f"{arm} bank {k_slots} step {j}")
        eng.adam_step()
        batches.append(finf)
        if k_slots:
            nq.check_ring(eng, batches)   # the wrap: step 2 overwrites slot 0, step 3 slot 1
    # the same step with the unweighted reference misses its rows
    plain = hand_reference(eng, *[t for t in (eng._score_operands()[0].reshape(eng.R, eng.D).cpu(), eng._score_operands()[1].reshape(eng.R, eng.D).cpu())],
                           (eng.score16 if eng._score16_live else eng.score).cpu(), [], (1.0, 1.0, 1.0), eng._score16_live)
    rows = eng.row_ws.cpu().double().numpy().reshape(eng.R, 2)
    if not k_slots:
        assert (np.abs(rows[:, 0] - plain["term"]) > plain["rbound"]).mean() > 0.5


def case_temporal_off(cfg: Cfg, arm: str):
    c = arm_cfg(cfg, arm)
    eng = engine(c, (1, 0, 1))
    x = inputs(c, 1)[0]
    eng._forward_loss(x, True)
    R = eng.R
    cls = eng.get_mask().reshape(R, R).cpu().numpy()
    d = eng.dscore[:, :R].float().cpu().numpy()
    assert (cls == -1).sum() == R * (c.P - 1) and (d[cls == -1] == 0).all() and (d[cls == 1] != 0).all()
    eng.backward()
    eng.adam_step()
    kc.all_finite(eng.flat_p)


def case_eval_between(cfg: Cfg, arm: str):
    c = arm_cfg(cfg, arm)
    eng, plain = engine(c, WEIGHTS, report=True), engine(c)
    xs = inputs(c, 2)
    eng.train_step(xs[0])
    plain.flat_p.copy_(eng.flat_p)
    plain.packed_for_step = -1
    rep = eng._ncls_report.clone()
    la, lb = eng._launches, plain._launches
    for e in (eng, plain):
        e.forward(xs[1], train=False, materialise=False)
        e.loss_topk(with_grad=False)
    assert torch.equal(bits(eng.result), bits(plain.result)) and torch.equal(bits(eng.row_ws), bits(plain.row_ws))
    assert eng._launches - la == plain._launches - lb and torch.equal(bits(rep), bits(eng._ncls_report))
    sa, sb = eng.forward(xs[1], train=False), plain.forward(xs[1], train=False)   # forward(materialise=True) and its loss
    assert sa is not None and torch.equal(bits(sa), bits(sb)) and not eng._ncls_live
    assert eng.forward(xs[1], train=True) is not None and not eng._ncls_live       # the module boundary's training forward
    eng.forward(xs[1], train=False)
    eng.loss_topk(with_grad=True)
    plain.loss_topk(with_grad=True)
    assert torch.equal(bits(eng.dscore), bits(plain.dscore)) and torch.equal(bits(eng.result), bits(plain.result))


def case_combined(cfg: Cfg, report=print):
    """the cosine score, accumulation 2 and a NaN micro-batch under skip_nonfinite, with the weights and the report on"""
    c = arm_cfg(cfg, "f32 logits")
    xs = inputs(c, 4)

    def make(weights, rep):
        e = engine(c, weights, report=rep)
        e.set_score_norm("cosine", 0.25)
        e.set_grad_accum(2)
        e.set_grad_guard(skip_nonfinite=True)
        return e
    eng = make(WEIGHTS, True)
    eng.train_step(xs[0])
    with pytest.raises(RuntimeError, match="accumulation cycle is open"):
        eng.set_neg_classes((1, 1, 1))
    hand_step(eng, xs[1], [], WEIGHTS, report, "cosine, accumulation, micro-batch 1", grads=False)
    eng._accum_finish_and_exchange()
    eng._accum_pos = 0
    eng.adam_step()
    assert eng.step_count == 1
    before = all_arenas(eng)
    bad = xs[2].clone()
    bad.view(-1)[7] = float("nan")
    eng.train_step(bad)
    eng.train_step(xs[3])
    assert eng.grad_stats()["skip"] == 1 and same(all_arenas(eng), before)
    eng.train_step(xs[0])   # the next cycle is a cycle like any other
    eng.train_step(xs[1])
    kc.all_finite(eng.flat_p, eng._ncls_report)
    assert eng.step_count == 2
    s = eng.neg_class_stats()
    assert abs(s["mass_pos"] + s["mass_S"] + s["mass_T"] + s["mass_E"] - 1.0) <= 8 * EPS24


def case_checkpoint(cfg: Cfg, tmp_path):
    from dpc_amd import checkpoint as ckpt
    c = arm_cfg(cfg, "f32 logits")
    a, b, plain, rep = engine(c, WEIGHTS), engine(c, WEIGHTS), engine(c), engine(c, report=True)
    a.train_step(inputs(c, 1)[0])
    state = ckpt.build_state(a, 1, "resnet18", 0.0, 1)
    assert state["neg_weight"] == {"spatial": 0.5, "temporal": 2.0, "easy": 0.25}
    assert "neg_weight" not in ckpt.build_state(plain, 1, "resnet18", 0.0, 1) and "neg_weight" not in ckpt.build_state(rep, 1, "resnet18", 0.0, 1)
    path = str(tmp_path / "epoch1.pth.tar")
    ckpt.save_checkpoint(state, filename=path)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ckpt.resume(b, path)            # the same weights: silent
    assert b.neg_classes == (WEIGHTS, False)
    for other in (plain, rep):
        with pytest.warns(UserWarning, match="negative-class weights spatial 0.5 temporal 2 easy 0.25") as rec:
            ckpt.resume(other, path)
        assert sum("negative-class weights" in str(w.message) for w in rec) == 1 and other.neg_classes[0] == (1.0, 1.0, 1.0)
    ppath = str(tmp_path / "plain.pth.tar")
    ckpt.save_checkpoint(ckpt.build_state(plain, 1, "resnet18", 0.0, 1), filename=ppath)
    with pytest.warns(UserWarning, match="this run continues with spatial 0.5 temporal 2 easy 0.25"):
        ckpt.resume(b, ppath)


def case_refusals(cfg: Cfg):
    from dpc_amd.engine import DPCEngine
    c = arm_cfg(cfg, "f32 logits")
    eng = engine(c)
    for bad in ((1, 1), (1, 1, 1, 1), "abc", (float("nan"), 1, 1), (1, -0.5, 1), (1, 1, 65537), (float("inf"), 1, 1), None):
        with pytest.raises(ValueError, match="negative-class weights"):
            eng.set_neg_classes(bad)
    assert eng.neg_classes == ((1.0, 1.0, 1.0), False)
    fused = DPCEngine("resnet18", c.size, c.N, c.SL, c.P, c.B, c.device, BF16, c.widths, lib=c.simulator, score_path="fused")
    with pytest.raises(L.DpcError, match="fused"):
        fused.set_neg_classes((0.5, 1, 1))
    with pytest.raises(L.DpcError, match="fused"):
        fused.set_neg_classes(report=True)
    fused.set_neg_classes()   # off is never refused
    eng.set_neg_queue(2)
    with pytest.raises(L.DpcError, match="easy"):
        eng.set_neg_classes((1, 1, 0))
    eng.set_neg_classes((0, 0, 1))
    eng.set_neg_queue(0)
    eng.set_neg_classes((1, 1, 0))
    with pytest.raises(L.DpcError, match="easy"):   # ... and the other order
        eng.set_neg_queue(2)
    assert eng.neg_queue == 0
    eng.set_neg_classes()
    eng.set_grad_accum(2)
    eng.train_step(inputs(c, 1)[0])
    with pytest.raises(RuntimeError, match="accumulation cycle is open"):
        eng.set_neg_classes((0.5, 1, 1))
    eng.reset_accum()
    eng.set_neg_classes((0.5, 1, 1))
    assert eng.neg_classes == ((0.5, 1.0, 1.0), False)
    if c.device != "cpu":
        t = torch.zeros(8, device=c.device)
        torch.cuda.synchronize()
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            t.add_(1.0)
            with pytest.raises(L.DpcError, match="captured"):
                eng.set_neg_classes((1, 1, 1))
        assert eng.neg_classes == ((0.5, 1.0, 1.0), False)


# ---------------------------------------------------------------------- the entry (simulator)
def case_entry(emu, widths, capsys, tmp_path):
    from dpc_amd import main as dpc_main
    common = ["--net", "resnet18", "--img_dim", "64", "--batch_size", "2", "--gpu", "0", "--print_freq", "1", "--num_seq", "4", "--epochs", "1",
              "--pred_step", "2", "--synthetic", "1"]
    run = lambda flags: (dpc_main.main(common + flags, _simulator=emu, _widths=widths), capsys.readouterr().out)[1]   # noqa: E731
    strip = lambda s: re.sub(r"T:\d+\.\d+", "T:", s)   # noqa: E731
    off = run(["--neg_weight", "1,1,1"])   # the defaults, spelled out
    assert "Negative classes" not in off and " neg P/S/T/E" not in off
    on = run(["--neg_weight", "0.5,2,0.25", "--neg_report"])
    assert on.splitlines().count("Negative classes: spatial 0.5 temporal 2 easy 0.25") == 1, on
    tail = re.compile(r" neg P/S/T/E (\d\.\d{3})/(\d\.\d{3})/(\d\.\d{3})/(\d\.\d{3}) above S/T/E (\d\.\d{3})/(\d\.\d{3})/(\d\.\d{3})$")
    lines = [ln for ln in on.splitlines() if ln.startswith("Epoch: [")]
    assert len(lines) == 1
    for ln in lines:
        m = tail.search(ln)
        assert m, ln
        assert abs(sum(float(v) for v in m.groups()[:4]) - 1.0) <= 0.002
    rep = run(["--neg_report"])   # the report alone: the default run's numbers, every training line with the tail
    assert "Negative classes" not in rep
    cut = lambda s: [tail.sub("", ln) for ln in strip(s).splitlines()]   # noqa: E731
    assert cut(rep) == cut(off) and all(tail.search(ln) for ln in rep.splitlines() if ln.startswith("Epoch: ["))
    assert cut(on) != cut(off)   # the weights change the loss
    for flags in (["--neg_weight", "1,1"], ["--neg_weight", "1,x,1"], ["--neg_weight", "1,-1,1"], ["--neg_weight", "nan,1,1"],
                  ["--neg_weight", "1,1,70000"], ["--neg_weight", "1,1,0", "--neg_queue", "2"]):
        with pytest.raises(ValueError, match="--neg_weight"):   # before a rank starts: nothing is printed
            dpc_main.main(common + flags, _simulator=emu, _widths=widths)
        assert capsys.readouterr().out == ""


# ---------------------------------------------------------------------- captured steps (HIP device only)
def case_captured(cfg: Cfg, arm: str, k_slots: int = 0, accum: int = 1):
    """a captured step under the weights and the report replayed five times against an eager twin, bit for bit (with a bank: across the
    fill boundary and the wrap); the capture holds the plain capture's launches plus REPORT_CALLS per step; a replay after
    set_neg_classes raises"""
    c = arm_cfg(cfg, arm)
    xs = inputs(c, 6 * accum)
    a, b = engine(c, WEIGHTS, True, k_slots), engine(c, WEIGHTS, True, k_slots)
    plain = engine(c, k_slots=k_slots)
    for e in (a, b, plain):
        if accum > 1:
            e.set_grad_accum(accum)
        for x in xs[:accum]:   # an eager step (cycle) sizes every lazy buffer
            e.train_step(x)
    block = xs[0].clone()
    ref = plain.capture_train_step(block, warmup=0)
    replay = a.capture_train_step(block, warmup=0)
    if accum > 1:
        assert replay.micro.kernels == [ref.micro.kernels[0] + REPORT_CALLS] and replay.last.kernels == [ref.last.kernels[0] + REPORT_CALLS]
    else:
        assert replay.kernels == [ref.kernels[0] + REPORT_CALLS]
    for j, x in enumerate(xs[accum:6 * accum]):
        block.copy_(x)
        ra = replay().clone()
        rb = b.train_step(x).clone()
        assert torch.equal(bits(ra), bits(rb)), j
        assert torch.equal(bits(a.flat_p), bits(b.flat_p)) and torch.equal(bits(a._ncls_report), bits(b._ncls_report)), j
        if k_slots:
            assert same(nq.ring_state(a), nq.ring_state(b)), j
    assert a.step_count == b.step_count == 6
    a.set_neg_classes((0.5, 2, 0.5), report=True)
    with pytest.raises(RuntimeError):
        replay()
    a.release_captures()
    plain.release_captures()
