"""Symmetric InfoNCE (csrc/loss_sym.hip: dpc_ce_colpass, dpc_ce_topk_sym / dpc_ce_topk_bf16_sym; DPCEngine.set_loss_sym; main --loss_sym),
shared by the CPU tier (host SIMT simulator, tests/test_sym_emu.py) and the GPU tier (tests/test_sym_gpu.py).

The reference of every case is the f64 statement of the loss: over the square logits S (as the loss reads them), with a = 1 - W, b = W,
    Lr_i = logsumexp([S[i, :], bank]) - S[i, i]          Lc_j = logsumexp(S[:, j]) - S[j, j]          loss = a mean Lr + b mean Lc
    rank_r[i] = #{j : S[i, j] > S[i, i]} + the bank's    rank_c[j] = #{i : S[i, j] > S[j, j]}
    dS[i, j] = (a (pr[i, j] - [i == j]) + b (pc[i, j] - [i == j])) / R,  pr the row softmax (bank in its denominator), pc the column softmax.

Kernel data is exact by construction, as loss_cases does it: every logit is a value of f32 and of bf16, so ranks are integer facts.
  column pass   loss_cases.row_case(n, U, square=True), transposed: its four row kinds (flat, ties with planted ranks, sentinel, hot +-100)
                sit on the columns, and the expectations per column are row_case's own per row
  W > 0         multiples of 1/4 in [-1, 1], so every column and every row carries at least e^-2 / n of its sum's mass and "the lightest
                contribution" is a number f32 can see
  hot cross     -60 everywhere, one +60 per row, all in the first 8 columns

Bounds carry no tolerance constant (QUARTER is loss_cases'):
  loss term     QUARTER * -log1p(-p_min): a quarter of what dropping the lightest contribution of the row (column) changes; the column
                pass alone on row_case data takes row_case's own bound, which is that with the sentinel / hot rows' J
  bf16 gradient within 2^-8 of the element's reference, relative (loss_cases: one bf16 rounding and an f32 value across a rounding boundary)
  f32 gradient  QUARTER * min(a |t_row| drop_row[i], b |t_col| drop_col[j]) / R, t_row = pr - [i == j], t_col = pc - [i == j], drop_row[i] the
                lightest probability of row i (what removing that column changes every probability of the row by, relatively), drop_col[j]
                likewise.  Two readings the formula needs, both from the number formats: a term of weight 0 (a at W = 1) is not in the
                loss and not in the minimum; a term whose f64 size a |t_row| / R is below the smallest normal f32 cannot be carried
                by an f32 at all (the hot cross: e^-120) and is not in the minimum either -- the element is then held by the other term.
                Both terms of an element have the same sign, so there is no cancellation to excuse; a reference that drops the lightest
                row from a column's sum, or the lightest column from a row's, moves every off-diagonal element by four times its
                bound (held on the reference in case_weighted).
  means         the largest term bound plus n 2^-24 of the mean term (ce_finalize's f32 sum)

Engine cases: negq_cases.hand_reference's widened bounds for a network's logits, with the column direction beside the row direction."""
import ctypes as C
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
import negcls_cases as nc
import negq_cases as nq
from dpc_amd import _lib as L
from kcases import K

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
QUARTER, GUARD, TINY = lc.QUARTER, lc.GUARD, lc.TINY
Cfg = gc.Cfg
bits = lc._bits
_t = lc._t
EPS24 = 2.0 ** -24
WEIGHTS = (0.25, 0.5, 1.0)

# the base sizes, and one unit past every seam of the column pass (csrc/loss_sym.hip):
#   17   row slabs are multiples of 16 rows: the second slab holds one row (scalar form)
#   20   ... the f32 16-byte form: 16 rows and one unit of 4
#   24   ... the bf16 16-byte form: 16 rows and one unit of 8
#   65   the scalar form's column strips are 64 wide: one column into the second strip
#   260  the f32 form's strips are 256 columns: one unit into the second strip
#   520  the bf16 form's strips are 512 columns: one unit into the second strip (also a base size)
KERNEL_N = (1, 8, 17, 20, 24, 37, 40, 65, 136, 260, 520, 1030)
KERNEL_N_GPU = KERNEL_N + (1100, 2056, 8200)   # 2 056: second register trip of the bf16 row form; 8 200: its NV = 8 form


def unit_of(sdt):
    return 8 if sdt == BF16 else 4


def arms_of(n):
    """(logits dtype, gradient dtype): f32 logits with either gradient, bf16 logits where the entry serves the width"""
    return [(F32, F32), (F32, BF16)] + ([(BF16, BF16)] if n % 8 == 0 else [])


def ws_floats(k: K, n, slabs=0):
    nf = C.c_int64(0)
    count = k.lib.call("dpc_ce_sym_ws_floats", n, slabs, C.byref(nf))
    assert count >= 1 and nf.value == count * 3 * n
    return nf.value, count


# ---------------------------------------------------------------------------------------------------------------- data and reference
@functools.lru_cache(maxsize=None)
def grid_logits(n):
    """[n][n] multiples of 1/4 in [-1, 1] (int8 numerators); on the diagonal's row and column a tie with the target and a logit 1/4 above"""
    g = torch.Generator().manual_seed(9000 + n)
    q = torch.randint(-4, 5, (n, n), generator=g, dtype=torch.int8)
    if n >= 4:
        i = torch.arange(n)
        d = q[i, i].clone()
        q[i, (i + 1) % n] = d                                   # a tie in the row, never counted
        q[(i + 2) % n, i] = d                                   # ... and in the column
        q[i, (i + 3) % n] = torch.clamp(d + 1, max=4)
    return q


@functools.lru_cache(maxsize=None)
def cross_logits(n):
    q = torch.full((n, n), -60.0)
    i = torch.arange(n)
    q[i, i % min(8, n)] = 60.0
    return q


Ref = namedtuple("Ref", "term_r term_c rank_r rank_c bound_r bound_c pr pc drop_r drop_c")


def reference(S, qstats=None):
    """f64 on S's device: S [n][n] f64, qstats [n][4] (m, l, rk, -) or None"""
    n = S.shape[0]
    diag = S.diagonal()
    mx = S.max(1).values
    if qstats is not None:
        q = qstats.to(S.device, F64)
        mx = torch.maximum(mx, q[:, 0])
    e = torch.exp(S - mx[:, None])
    Z = e.sum(1)
    if qstats is not None:
        Z = Z + q[:, 1] * torch.exp(q[:, 0] - mx)
    pr = e / Z[:, None]
    term_r = torch.log(Z) + mx - diag
    rank_r = (S > diag[:, None]).sum(1).double() + (q[:, 2] if qstats is not None else 0.0)
    mc = S.max(0).values
    ec = torch.exp(S - mc[None, :])
    Zc = ec.sum(0)
    pc = ec / Zc[None, :]
    term_c = torch.log(Zc) + mc - diag
    rank_c = (S > diag[None, :]).sum(0).double()
    drop_r, drop_c = pr.min(1).values, pc.min(0).values
    return Ref(term_r, term_c, rank_r, rank_c, QUARTER * -torch.log1p(-drop_r), QUARTER * -torch.log1p(-drop_c), pr, pc, drop_r, drop_c)


def grad_of(ref: Ref, W, swap=False):
    """(gradient, f32 bound) at weight W; swap: rows and columns exchanged (the wrong reference)"""
    n = ref.pr.shape[0]
    a, b = (W, 1.0 - W) if swap else (1.0 - W, W)
    eye = torch.eye(n, dtype=F64, device=ref.pr.device)
    tr, tc = ref.pr - eye, ref.pc - eye
    g = (a * tr + b * tc) / n
    inf = torch.full_like(g, float("inf"))
    br = torch.where((a * tr.abs() / n >= TINY) & (a > 0), a * tr.abs() * ref.drop_r[:, None], inf)
    bc = torch.where((b * tc.abs() / n >= TINY) & (b > 0), b * tc.abs() * ref.drop_c[None, :], inf)
    bound = QUARTER * torch.minimum(br, bc) / n
    bound = torch.where(torch.isinf(bound), torch.zeros_like(bound), bound)   # neither term is an f32: the element is below TINY
    return g, bound


Sym = namedtuple("Sym", "out lse col_lse col_ws sym")


def run_sym(k: K, sdev, sdt, gdt, n, W, qs=None, slabs=0, ld=None, with_grad=True):
    """one call of the entry the logits' dtype selects; every output poisoned, guard bands behind each"""
    E = 8 if (gdt == BF16 or sdt == BF16) else 4
    ld_d = (n + E - 1) // E * E
    out = lc.Out(k, n, ld_d, gdt if with_grad else None)
    lse = k.poison(n + GUARD) if qs is not None else None
    nf, _ = ws_floats(k, n, slabs)
    cl, cw, ws, sr = k.poison(n + GUARD), k.poison(2 * n + GUARD), k.poison(nf + GUARD), k.poison(8 + GUARD)
    tail = (qs, lse, W, slabs, cl, cw, ws, sr)
    if sdt == BF16:
        k.call("dpc_ce_topk_bf16_sym", sdev, n, n, ld or n, out.ws, out.res, out.d, ld_d, *tail)
    else:
        k.call("dpc_ce_topk_sym", sdev, n, n, ld or n, out.ws, out.res, out.d, L.dtype_code(gdt or F32), ld_d, *tail)
    k.sync()
    out.guard_untouched()
    for t, m in ((cl, n), (cw, 2 * n), (ws, nf), (sr, 8)) + (((lse, n),) if lse is not None else ()):
        assert bool(torch.isnan(t[m:]).all()), "written past an output"
    kc.all_finite(cl[:n], cw[:2 * n], sr[:8])
    return Sym(out, lse, cl[:n], cw[:2 * n].view(n, 2), sr[:8])


def run_colpass(k: K, sdev, sdt, n, ld, fast, slabs=0):
    nf, count = ws_floats(k, n, slabs)
    cl, cw, ws = k.poison(n + GUARD), k.poison(2 * n + GUARD), k.poison(nf + GUARD)
    k.call("dpc_ce_colpass", sdev, L.dtype_code(sdt), n, ld, int(fast), slabs, cl, cw, ws)
    k.sync()
    for t, m in ((cl, n), (cw, 2 * n), (ws, nf)):
        assert bool(torch.isnan(t[m:]).all()), "written past an output"
    kc.all_finite(cl[:n], cw[:2 * n])
    return cl[:n], cw[:2 * n].view(n, 2)


# ---------------------------------------------------------------------------------------------------------------- K1 column pass alone
def case_colpass(k: K, n, report=print):
    for sdt in (F32, BF16):
        if n == 1:   # (row_case plants its kinds in two columns or more) the one logit is its own target: term log 1 = 0 whatever is dropped
            rc = lc.RowCase(np.array([[0.25]]), ("flat",), 0, np.array([0]), np.array([0.0]), np.array([np.inf]), None, None, True, (0,))
        else:
            rc = lc.row_case(n, unit_of(sdt), square=True)
        S = np.ascontiguousarray(rc.s.T)         # row_case's rows are the columns; the target of column j is still S[j][j]
        clean = k.t(_t(S), sdt)
        for fast in (False, True):
            cl, cw = run_colpass(k, clean, sdt, n, n, fast)
            w = cw.cpu().numpy().astype(np.float64)
            assert np.array_equal(w[:, 1], rc.rank.astype(np.float64)), f"n {n}: column rank differs on {np.nonzero(w[:, 1] != rc.rank)[0][:8].tolist()}"
            e = np.abs(w[:, 0] - rc.term)
            worst = int(np.argmax(e / rc.loss_bound))
            report(f"[sym-col] n {n} {'bf16' if sdt == BF16 else 'f32'} fast {int(fast)}: term {e[worst] / rc.loss_bound[worst]:.3g} of its bound "
                   f"(column {worst}, {rc.kinds[worst]})")
            assert (e < rc.loss_bound).all(), f"n {n}: column terms {np.nonzero(~(e < rc.loss_bound))[0][:8].tolist()}"
            lse_want = rc.term + np.diagonal(rc.s)
            el = np.abs(cl.cpu().numpy().astype(np.float64) - lse_want)
            assert (el < rc.loss_bound + np.spacing(np.abs(lse_want).astype(np.float32))).all(), f"n {n}: col_lse"
            again = run_colpass(k, clean, sdt, n, n, fast)                     # two runs: the same bits
            assert torch.equal(bits(again[0]), bits(cl)) and torch.equal(bits(again[1]), bits(cw))
            # another slab count: the same ranks, terms within the bound (the order of the sums differs)
            if n > 16:
                other = run_colpass(k, clean, sdt, n, n, fast, slabs=2)
                wo = other[1].cpu().numpy().astype(np.float64)
                assert np.array_equal(wo[:, 1], w[:, 1]) and (np.abs(wo[:, 0] - rc.term) < rc.loss_bound).all(), f"n {n}: two slabs"
        # ld > n with NaN in [n, ld), NaN rows behind row n: the 16-byte form again (ld a multiple of the unit) and the scalar form;
        # a pointer 4 bytes off a 16-byte boundary: the scalar form.  Bit-identical to the clean copy through the same form.
        U = unit_of(sdt)
        off_el = 4 // clean.element_size()
        for ld, off in ((n + U, 0), (n + 1, 0), (n, off_el)):
            buf = torch.full((off + (n + 2) * ld,), float("nan"), dtype=sdt)
            buf[off:off + n * ld].view(n, ld)[:, :n] = _t(S).to(sdt)
            dev = buf.to(k.dev)
            view = dev[off:]
            assert dev.data_ptr() % 16 == 0
            got = run_colpass(k, view, sdt, n, ld, True)
            # the clean copy through the same form: tight with the same alignment class
            vec = n % U == 0 and ld % U == 0 and off == 0
            if vec:
                want = run_colpass(k, clean, sdt, n, n, True)
            else:   # the scalar form on a clean matrix: one element off alignment, rows tight
                cbuf = torch.zeros(1 + n * n + 1, dtype=sdt)
                cbuf[1:1 + n * n] = _t(S).to(sdt).reshape(-1)
                cdev = cbuf.to(k.dev)
                want = run_colpass(k, cdev[1:], sdt, n, n, True)
            assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1])), f"n {n} ld {ld} off {off}: padding was read"
            wg = got[1].cpu().numpy().astype(np.float64)
            assert np.array_equal(wg[:, 1], rc.rank.astype(np.float64)) and (np.abs(wg[:, 0] - rc.term) < rc.loss_bound).all()


# ---------------------------------------------------------------------------------------------------------------- K2 W = 0 is the old entry
def square_shapes(table, limit):
    """the names of loss_cases.CE_SHAPES / CE16_SHAPES whose matrix can be square: rows = cols up to `limit` columns"""
    return [name for name, (cols, _, _, _) in table.items() if cols <= limit]


def case_zero_is_the_old_entry(k: K, entry, name, mode, bank):
    """one shape of loss_cases.CE_SHAPES / CE16_SHAPES as a square matrix: W = 0 against the older entry (its _ext form with a bank's
    statistics), bit for bit.  Modes as negq_cases.case_ext_empty."""
    bf_logits = entry == "dpc_ce_topk_bf16"
    cols, ld, ld_d, off = (lc.CE16_SHAPES if bf_logits else lc.CE_SHAPES)[name]
    rc = lc.row_case(cols, 8 if bf_logits else 4, square=True)
    rows = cols
    ld, ld_d = ld or cols, ld_d or cols
    keep, sview = lc._strided(k, rc.s, ld, BF16 if bf_logits else F32, off)
    gdt = {"f32": F32, "bf16": BF16}.get(mode)
    code = L.dtype_code(F32 if mode in ("f32", "null") else BF16)
    qs = k.t(nc.bank_stats(rows)) if bank else None
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
    new = lc.Out(k, rows, ld_d, gdt)
    lse = k.poison(rows + GUARD) if bank else None
    nf, _ = ws_floats(k, rows)
    cl, cw, ws, sr = k.poison(rows), k.poison(2 * rows), k.poison(nf), k.poison(8)
    tail = (qs, lse, 0.0, 0, cl, cw, ws, sr)
    if bf_logits:
        k.call(entry + "_sym", sview, rows, cols, ld, new.ws, new.res, new.d, ld_d, *tail)
    else:
        k.call(entry + "_sym", sview, rows, cols, ld, new.ws, new.res, new.d, code, ld_d, *tail)
    k.sync()
    tag = f"{entry}_sym {name} {mode} bank={bank}"
    kc.all_finite(cl, cw, sr)
    assert torch.equal(bits(new.ws), bits(old.ws)) and torch.equal(bits(new.res), bits(old.res)), f"{tag}: other bits"
    if gdt is not None:
        assert torch.equal(bits(new.dbuf), bits(old.dbuf)), f"{tag}: other gradient bits"
    if bank:
        assert torch.equal(bits(lse), bits(old_lse)), f"{tag}: other lse_out bits"
    assert torch.equal(bits(sr[:1]), bits(old.res[:1])), f"{tag}: sym_result[0] is not the row mean"
    del keep


def case_zero_big(k: K, entry, cols, gdt):
    """the forms past 8 192 columns (ce_row_vec<., 16, .>, ce_row_vec16<8>) as a square matrix, GPU tier: grid logits drawn on the device,
    W = 0 against the older entry bit for bit"""
    bf_logits = entry == "dpc_ce_topk_bf16"
    g = torch.Generator(device=k.dev).manual_seed(cols)
    s = (torch.randint(-4, 5, (cols, cols), generator=g, device=k.dev, dtype=torch.int8).float() / 4.0).to(BF16 if bf_logits else F32)
    old, new = lc.Out(k, cols, cols, gdt), lc.Out(k, cols, cols, gdt)
    lc._launch(k, entry, s, cols, cols, cols, old, L.dtype_code(gdt))
    nf, _ = ws_floats(k, cols)
    cl, cw, ws, sr = k.poison(cols), k.poison(2 * cols), k.poison(nf), k.poison(8)
    tail = (None, None, 0.0, 0, cl, cw, ws, sr)
    if bf_logits:
        k.call(entry + "_sym", s, cols, cols, cols, new.ws, new.res, new.d, cols, *tail)
    else:
        k.call(entry + "_sym", s, cols, cols, cols, new.ws, new.res, new.d, L.dtype_code(gdt), cols, *tail)
    k.sync()
    kc.all_finite(cl, cw, sr)
    assert torch.equal(bits(new.ws), bits(old.ws)) and torch.equal(bits(new.res), bits(old.res)) and torch.equal(bits(new.dbuf), bits(old.dbuf))


# ---------------------------------------------------------------------------------------------------------------- K3 W > 0
def check_sym(tag, run: Sym, ref: Ref, W, gdt, n, report=print, grad_where=None):
    a, b = 1.0 - W, W
    dev = ref.pr.device
    rw, cw = run.out.ws.to(dev, F64), run.col_ws.to(dev, F64)
    assert torch.equal(rw[:, 1], ref.rank_r), f"{tag}: row ranks differ on {torch.nonzero(rw[:, 1] != ref.rank_r)[:8, 0].tolist()}"
    assert torch.equal(cw[:, 1], ref.rank_c), f"{tag}: column ranks differ on {torch.nonzero(cw[:, 1] != ref.rank_c)[:8, 0].tolist()}"
    er, ec = (rw[:, 0] - ref.term_r).abs(), (cw[:, 0] - ref.term_c).abs()
    assert bool((er < ref.bound_r).all()) and bool((ec < ref.bound_c).all()), f"{tag}: terms {float((er / ref.bound_r).max()):.3g} / {float((ec / ref.bound_c).max()):.3g}"
    res, sym = run.out.res.cpu().double().numpy(), run.sym.cpu().double().numpy()
    Lr, Lc = float(ref.term_r.mean()), float(ref.term_c.mean())
    mr = float(ref.bound_r.max()) + n * EPS24 * abs(Lr)
    mc = float(ref.bound_c.max()) + n * EPS24 * abs(Lc)
    assert abs(sym[0] - Lr) < mr and abs(sym[1] - Lc) < mc, f"{tag}: means {sym[:2].tolist()} against {Lr}, {Lc}"
    mixed = (a * mr if a else 0.0) + (b * mc if b else 0.0)   # (n = 1: the bounds are infinite, and 0 * inf is no bound)
    assert abs(res[0] - (a * Lr + b * Lc)) < mixed + EPS24 * abs(a * Lr + b * Lc), f"{tag}: loss {res[0]}"
    for i, kk in enumerate((1, 3, 5)):
        assert res[1 + i] == float(np.float32(int((ref.rank_r < kk).sum())) / np.float32(n)), f"{tag}: row top-{kk}"
        assert sym[2 + i] == float(np.float32(int((ref.rank_c < kk).sum())) / np.float32(n)), f"{tag}: column top-{kk}"
    assert (sym[5:] == 0).all()
    line = f"[sym] {tag}: terms {float((er / ref.bound_r).max()):.3g} / {float((ec / ref.bound_c).max()):.3g}"
    if gdt is not None:
        g = run.out.d[:, :n].to(dev, F64)
        assert bool(torch.isfinite(g).all()), f"{tag}: a gradient element is not finite"
        want, fb = grad_of(ref, W)
        tiny = want.abs() < TINY
        assert bool((g[tiny].abs() < TINY).all()), f"{tag}: an element whose reference underflows is not below the smallest normal number"
        bound = 2.0 ** -8 * want.abs() if gdt == BF16 else fb
        ok = ((g - want).abs() <= bound) | tiny
        if grad_where is not None:
            ok = ok | ~grad_where
        ratio = torch.where(tiny | (bound == 0), torch.zeros_like(g), (g - want).abs() / bound.clamp_min(1e-300))
        if grad_where is not None:
            ratio = torch.where(grad_where, ratio, torch.zeros_like(ratio))
        line += f", gradient {float(ratio.max()):.3g} of its bound"
        assert bool(ok.all()), f"{tag}: {int((~ok).sum())} gradient elements outside the bound, worst {float(ratio.max()):.3g}"
        if run.out.d.shape[1] > n:
            assert float(run.out.d[:, n:].float().abs().max()) == 0.0
        # the wrong references: the row direction alone, and rows and columns exchanged
        shares = []
        for name, (wg, _) in (("W = 0", grad_of(ref, 0.0)), ("exchanged", grad_of(ref, W, swap=True))):
            miss = float((((g - wg).abs() > bound) & ~tiny).double().mean())
            shares.append(f"{name} misses {miss:.3f}")
            if gdt == F32 and n >= 8 and grad_where is None and not (name == "exchanged" and W == 0.5):   # (at W = 1/2 exchanged is the same loss)
                assert miss > 0.75, f"{tag}: the reference with {name} stays inside the bound on {1 - miss:.3f} of the elements"
        line += "; " + ", ".join(shares)
    report(line)


def case_weighted(k: K, n, W, report=print):
    q = grid_logits(n)
    S = k.t(q, F64) / 4.0
    for bank in (False, True):
        qs = k.t(nc.bank_stats(n)) if bank else None
        ref = reference(S, qs)
        if not bank and n >= 8:   # on the reference: without its lightest row (column) a column's (row's) off-diagonal elements move by 4 bounds
            _, fb = grad_of(ref, W)
            eye = torch.eye(n, dtype=torch.bool, device=S.device)
            moved_c = W * ref.pc * (ref.drop_c / (1 - ref.drop_c))[None, :] / n
            moved_r = (1 - W) * ref.pr * (ref.drop_r / (1 - ref.drop_r))[:, None] / n
            assert bool((moved_c[~eye] >= 4 * fb[~eye]).all()) and (W == 1.0 or bool((moved_r[~eye] >= 4 * fb[~eye]).all()))
        for sdt, gdt in arms_of(n):
            sdev = k.t(q.float() / 4.0, sdt)
            run = run_sym(k, sdev, sdt, gdt, n, W, qs=qs)
            tag = f"n {n} W {W:g} {'bf16' if sdt == BF16 else 'f32'} logits, {'bf16' if gdt == BF16 else 'f32'} gradient, bank {int(bank)}"
            check_sym(tag, run, ref, W, gdt, n, report)
            if bank and W < 1:   # lse_out = lse - log a (dpc_negq_bwd then yields a x the bank's share): two f32 roundings at that size more
                el = (run.lse[:n].to(S.device, F64) - (ref.term_r + S.diagonal() - np.log(1.0 - W))).abs()
                assert bool((el < ref.bound_r + 2 * EPS24 * 8).all()), f"{tag}: lse_out"
            elif bank:           # a = 0: no share at all
                assert bool((run.lse[:n] > 1e37).all()) and bool(torch.isfinite(run.lse[:n]).all()), f"{tag}: lse_out at W = 1"
            if gdt == F32 and not bank:   # without a gradient: the same row_ws / result bits
                null = run_sym(k, sdev, sdt, None, n, W, with_grad=False)
                assert torch.equal(bits(null.out.ws), bits(run.out.ws)) and torch.equal(bits(null.out.res), bits(run.out.res))
                assert torch.equal(bits(null.col_ws), bits(run.col_ws)) and torch.equal(bits(null.sym), bits(run.sym))


# ---------------------------------------------------------------------------------------------------------------- K4 hot cross
def case_hot_cross(k: K, n, report=print):
    q = cross_logits(n)
    S = k.t(q, F64)
    ref = reference(S)
    hot = min(8, n)
    outside = torch.zeros((n, n), dtype=torch.bool, device=S.device)
    outside[:, hot:] = True
    outside.fill_diagonal_(False)   # (a target's element is p - 1 in both directions: held with the hot columns below)
    for W in (0.5, 1.0):
        want, _ = grad_of(ref, W)
        if n > hot:   # outside the hot columns pc is 1 / n and the row's own exponentials have underflowed
            assert bool(((want[outside] - W / (n * n)).abs() <= 1e-12 * W / (n * n)).all()) and bool((ref.pr[outside] < 1e-50).all())
        for sdt, gdt in arms_of(n):
            run = run_sym(k, k.t(q, sdt), sdt, gdt, n, W)
            tag = f"hot cross n {n} W {W:g} {'bf16' if sdt == BF16 else 'f32'} logits, {'bf16' if gdt == BF16 else 'f32'} gradient"
            g = run.out.d[:, :n].to(S.device, F64)
            assert bool(torch.isfinite(g).all()), f"{tag}: not finite"
            assert torch.equal(run.col_ws.to(S.device, F64)[:, 1], ref.rank_c) and torch.equal(run.out.ws.to(S.device, F64)[:, 1], ref.rank_r)
            if n > hot:
                _, fb = grad_of(ref, W)
                bound = 2.0 ** -8 * want.abs() if gdt == BF16 else fb
                e = (g - want).abs()
                assert bool((bound[outside] > 0).all())
                report(f"[sym] {tag}: outside the hot columns {float((e[outside] / bound[outside]).max()):.3g} of the bound")
                assert bool((e[outside] <= bound[outside]).all()), f"{tag}: W / (n R) is missed outside the hot columns"
            # inside them: every element that an f32 can carry within 2^-8 of its reference (they are not the case's subject)
            big = want.abs() >= TINY
            assert bool((((g - want).abs() <= 2.0 ** -8 * want.abs()) | ~big | outside).all()), f"{tag}: inside the hot columns"


# ---------------------------------------------------------------------------------------------------------------- K5 refused calls
def case_refused(k: K):
    R = 24
    arg, uns = f"code {L.ERR_ARG}$", f"code {L.ERR_UNSUPPORTED}$"
    s32, s16 = k.zeros(R * R + 8), k.zeros(R * R + 16, dtype=BF16)
    qs = k.t(nc.bank_stats(R))
    nf, _ = ws_floats(k, R)
    outs = dict(ws=k.poison(R * 2 + GUARD), res=k.poison(4 + GUARD), d=k.poison(R * R + GUARD), d16=k.poison(R * R + GUARD, dtype=BF16),
                lse=k.poison(R + GUARD), cl=k.poison(R + GUARD), cw=k.poison(2 * R + GUARD), wk=k.poison(nf + GUARD), sr=k.poison(8 + GUARD))
    before = {n: bits(t) for n, t in outs.items()}
    o = outs

    def c32(w=0.5, score=s32, rows=R, cols=R, ld=R, qs_=None, lse_=None, cl=o["cl"], cw=o["cw"], wk=o["wk"], sr=o["sr"], ws_=o["ws"], res_=o["res"],
            code=L.F32, slabs=0):
        return lambda: k.call("dpc_ce_topk_sym", score, rows, cols, ld, ws_, res_, o["d"], code, R, qs_, lse_, w, slabs, cl, cw, wk, sr)

    def c16(w=0.5, score=s16, rows=R, cols=R, ld=R, qs_=None, lse_=None, cl=o["cl"], wk=o["wk"], sr=o["sr"]):
        return lambda: k.call("dpc_ce_topk_bf16_sym", score, rows, cols, ld, o["ws"], o["res"], o["d16"], R, qs_, lse_, w, 0, cl, o["cw"], wk, sr)
    bad = [
        (arg, c32(rows=R - 8)),                                 # rows != cols
        (arg, c32(rows=R, cols=R + 8, ld=R + 8)),
        (arg, c32(w=-0.25)), (arg, c32(w=1.5)), (arg, c32(w=float("nan"))), (arg, c32(w=float("inf"))),
        (arg, c32(wk=None)), (arg, c32(cl=None)), (arg, c32(cw=None)), (arg, c32(sr=None)),
        (arg, c32(cl=o["cl"][1:])),                             # col_lse off a 16-byte boundary
        (arg, c32(slabs=-1)),
        (arg, c32(qs_=qs)), (arg, c32(lse_=o["lse"])),          # qstats / lse_out go together
        (arg, c32(score=None)), (arg, c32(ws_=None)), (arg, c32(res_=None)),
        (arg, c32(ld=R - 1)),
        (arg, c32(code=77)),
        (arg, c16(rows=R - 8)), (arg, c16(w=2.0)), (arg, c16(w=float("nan"))), (arg, c16(wk=None)), (arg, c16(sr=None)),
        (arg, c16(qs_=qs)), (arg, c16(score=None)),
        (uns, c16(score=s16[4:])),                              # 8 bytes off a 16-byte boundary
        (uns, c16(ld=R + 4)),                                   # ld % 8 != 0
        (arg, c16(w=2.0, score=s16[4:])),                       # argument errors come first
        (arg, lambda: k.call("dpc_ce_colpass", s32, L.F32, R, R - 1, 0, 0, o["cl"], o["cw"], o["wk"])),
        (arg, lambda: k.call("dpc_ce_colpass", s32, 77, R, R, 0, 0, o["cl"], o["cw"], o["wk"])),
        (arg, lambda: k.call("dpc_ce_colpass", s32, L.F32, R, R, 2, 0, o["cl"], o["cw"], o["wk"])),
        (arg, lambda: k.call("dpc_ce_colpass", s32, L.F32, R, R, 0, 0, o["cl"], o["cw"], None)),
    ]
    for code, f in bad:
        with pytest.raises(L.DpcError, match=code):
            f()
    with pytest.raises(L.DpcError, match=arg):
        k.lib.call("dpc_ce_sym_ws_floats", 0, 0, C.byref(C.c_int64(0)))
    k.sync()
    for n, t in outs.items():
        assert torch.equal(bits(t), before[n]), f"a refused call wrote {n}"
    # the same calls go through once they are right: W = 0 and W = 1 are both accepted at this level
    c32(w=0.0, qs_=qs, lse_=o["lse"])()
    c16(w=1.0)()
    k.sync()
    kc.all_finite(o["ws"][:R * 2], o["res"][:4], o["cl"][:R], o["cw"][:2 * R], o["sr"][:8])
    for n, t in outs.items():
        assert torch.equal(bits(t)[-GUARD:], before[n][-GUARD:]), f"{n}: the guard band was written"


# ================================================================================================================ engine
# r18, num_seq 4, pred_step 2: R = B P SQ = 16 at 64 px (f32 logits) and 64 at 128 px (bf16 logits)
ARMS = nc.ARMS
SYM_CALLS = 0   # C-ABI calls per training step the symmetric loss adds (the engine's launch count, replay.kernels of a capture): the _sym
                # entry takes the place of dpc_ce_topk[_bf16][_ext] and launches the column pass (two kernels) itself
arm_cfg, inputs = nc.arm_cfg, nc.inputs
all_arenas, same = nq.all_arenas, nq.same


def engine(cfg: Cfg, w=0.0, k_slots=0):
    eng = gc.dpc_engine(cfg, BF16)
    if k_slots:
        eng.set_neg_queue(k_slots)
    if w:
        eng.set_loss_sym(w)
    return eng


def case_off_is_off(cfg: Cfg, arm: str):
    c = arm_cfg(cfg, arm)
    a, b = engine(c), engine(c)
    b.set_loss_sym(0.5)
    assert b.loss_sym == 0.5 and b._baked_scalars() == a._baked_scalars() + (("loss_sym", 0.5),)
    b.set_loss_sym()   # the default: off
    assert b.loss_sym == 0.0 == a.loss_sym and b._baked_scalars() == a._baked_scalars() and b._sym_col_lse is None
    with pytest.raises(L.DpcError, match="symmetric loss is off"):
        b.loss_sym_stats()
    la, lb = a._launches, b._launches
    for x in inputs(c, 2):
        ra, rb = a.train_step(x).clone(), b.train_step(x).clone()
        assert torch.equal(bits(ra), bits(rb)) and torch.equal(bits(a.flat_g), bits(b.flat_g)) and same(all_arenas(a), all_arenas(b))
    assert a._launches - la == b._launches - lb


def hand_reference(pred, finf, s_in, bank_keys, W, bf16_logits):
    """negq_cases.hand_reference with the column direction: f64 terms, ranks, d_pred, d_finf of one training step from the step's own
    score operands, its in-batch logits as the loss kernels read them and the keys the bank held; the same widened bounds (what f32
    itself adds on a network's logits), the columns' like the rows'"""
    P, F = pred.double().numpy(), finf.double().numpy()
    R = P.shape[0]
    a, b = 1.0 - W, W
    S = s_in.double().numpy()
    exact = P @ F.T
    tol = (np.abs(P) @ np.abs(F).T) * (2.0 ** -8 if bf16_logits else P.shape[1] * 2.0 ** -23) + 1e-30
    assert (np.abs(S - exact) <= tol).all(), "the in-batch logits are not pred @ finf^T"
    Q = np.concatenate([q.double().numpy() for q in bank_keys], 0) if bank_keys else np.zeros((0, P.shape[1]))
    allS = np.concatenate([S, P @ Q.T], 1)
    tgt = np.diagonal(S)
    idx = np.arange(R)
    mx = allS.max(1)
    e = np.exp(allS - mx[:, None])
    lse = np.log(e.sum(1)) + mx
    pr = e / e.sum(1)[:, None]
    term_r = lse - tgt
    mc = S.max(0)
    ec = np.exp(S - mc[None, :])
    lse_c = np.log(ec.sum(0)) + mc
    pc = ec / ec.sum(0)[None, :]
    term_c = lse_c - tgt
    dS = a * pr
    dS[:, :R] += b * pc
    dS[idx, idx] -= 1.0
    dS /= R
    keys = np.concatenate([F, Q], 0)
    N = keys.shape[0] + 64 + 32
    f = 2.0 ** -8 + N * 2.0 ** -24
    big_r = np.maximum(np.maximum(np.abs(mx), np.abs(tgt)), np.maximum(np.abs(lse), np.abs(term_r)))
    big_c = np.maximum(np.maximum(np.abs(mc), np.abs(tgt)), np.maximum(np.abs(lse_c), np.abs(term_c)))
    acc = P.shape[1] * 2.0 ** -24 * (np.abs(P) @ np.abs(Q).T).max(1) if Q.shape[0] else np.zeros(R)
    rbound = QUARTER * -np.log1p(-pr.min(1)) + 2.0 ** -24 * 4 * big_r + acc
    # the column pass rescales its running sum whenever the column's maximum moves, once more per slab and wave it merges: each a rounding
    # of the sum (2^-24 of it, so of the term absolutely); at most R of them
    cbound = QUARTER * -np.log1p(-pc.min(0)) + 2.0 ** -24 * (4 * big_c + R)
    mean = 2.0 ** -24 * (-(-R // 256) + 10)
    diag = 2.0 ** -23 / R
    return dict(term_r=term_r, term_c=term_c, rbound=rbound, cbound=cbound, rank_r=(allS > tgt[:, None]).sum(1), rank_c=(S > tgt[None, :]).sum(0),
                Lr=float(term_r.mean()), Lc=float(term_c.mean()), loss=float(a * term_r.mean() + b * term_c.mean()),
                lr_bound=float(rbound.max()) + mean * float(np.abs(term_r).mean()), lc_bound=float(cbound.max()) + mean * float(np.abs(term_c).mean()),
                d_pred=dS @ keys, b_pred=f * (np.abs(dS) @ np.abs(keys)) + diag * np.abs(F),
                d_finf=dS[:, :R].T @ P, b_finf=f * (np.abs(dS[:, :R]).T @ np.abs(P)) + diag * np.abs(P))


def through_norm(g, b, x, rn, scale):
    """dpc_rownorm_bwd in f64 (include/dpc_hip.h): g [R][D] the gradient at the normalised operand and b its bound, x the raw operand, rn
    the rows' 1 / norm as the forward kept them (f32 values), scale 1 / T or 1:  u = x rn, t = sum g u, out = (scale rn)(g - u t).  The
    bound carries b through the same expression and adds the kernel's own f32 roundings, counted: u, scale rn, the difference and the
    product (4 at the size of the terms) and the D products and D - 1 sums of t (D + 2 at the size of sum |g||u|)."""
    u, c = x * rn[:, None], (scale * rn)[:, None]
    D = x.shape[1]
    t, tabs = (g * u).sum(1, keepdims=True), (np.abs(g) * np.abs(u)).sum(1, keepdims=True)
    out = c * (g - u * t)
    bound = c * (b + np.abs(u) * (b * np.abs(u)).sum(1, keepdims=True)) + c * EPS24 * (4 * (np.abs(g) + np.abs(u) * tabs) + np.abs(u) * (D + 2) * tabs)
    return out, bound


def hand_step(eng, x, bank_keys, W, report, tag, grads=True):
    """one training step taken apart (negq_cases.hand_step) under the symmetric loss; under the cosine score the reference's gradients at
    the normalised operands go through the normalisation's backward in f64 (through_norm) before they are compared"""
    R, D = eng.R, eng.D
    a, b = 1.0 - W, W
    eng._forward_loss(x, True)
    sp, sf = eng._score_operands()
    pred, finf = sp.detach().reshape(R, D).cpu().clone(), sf.detach().reshape(R, D).cpu().clone()
    s_in = (eng.score16 if eng._score16_live else eng.score).detach().cpu().clone()
    res = eng.result.detach().cpu().clone()
    rows = eng.row_ws.detach().cpu().double().numpy().reshape(R, 2).copy()
    cols = eng._sym_col_ws.detach().cpu().double().numpy().reshape(R, 2).copy()
    stats = eng.loss_sym_stats()
    ref = hand_reference(pred, finf, s_in, bank_keys, W, eng._score16_live)
    er, ec = np.abs(rows[:, 0] - ref["term_r"]), np.abs(cols[:, 0] - ref["term_c"])
    assert (er < ref["rbound"]).all() and (ec < ref["cbound"]).all(), (tag, float((er / ref["rbound"]).max()), float((ec / ref["cbound"]).max()))
    assert np.array_equal(rows[:, 1], ref["rank_r"].astype(np.float64)) and np.array_equal(cols[:, 1], ref["rank_c"].astype(np.float64)), tag
    assert abs(stats["loss_row"] - ref["Lr"]) < ref["lr_bound"] and abs(stats["loss_col"] - ref["Lc"]) < ref["lc_bound"], (tag, stats, ref["Lr"], ref["Lc"])
    assert abs(float(res[0]) - ref["loss"]) < a * ref["lr_bound"] + b * ref["lc_bound"] + EPS24 * abs(ref["loss"]), (tag, float(res[0]), ref["loss"])
    for i, kk in enumerate((1, 3, 5)):
        assert float(res[1 + i]) == float(np.float32(int((ref["rank_r"] < kk).sum())) / np.float32(R)), (tag, kk)
    assert stats["col_top1"] == float(np.float32(int((ref["rank_c"] < 1).sum())) / np.float32(R)), tag
    line = (f"[sym-engine] {tag}: {len(bank_keys)} slots live, loss {float(res[0]):.5f} (f64 {ref['loss']:.5f}), Lr {stats['loss_row']:.5f} Lc "
            f"{stats['loss_col']:.5f}, rows {float((er / ref['rbound']).max()):.3g}, columns {float((ec / ref['cbound']).max()):.3g}")
    if grads:
        eng.backward()
        d_pred, d_finf = eng.d_pred.detach().reshape(R, D).cpu().double().numpy(), eng.d_finf.detach().reshape(R, D).cpu().double().numpy()
        plain = hand_reference(pred, finf, s_in, bank_keys, 0.0, eng._score16_live)
        if eng._snorm is not None:
            xp, xf = eng.pred.detach().reshape(R, D).cpu().double().numpy(), eng.feat_inf.detach().reshape(R, D).cpu().double().numpy()
            rn = eng.rnorm.detach().cpu().double().numpy()
            for r in (ref, plain):
                r["d_pred"], r["b_pred"] = through_norm(r["d_pred"], r["b_pred"], xp, rn[:R], float(eng._snorm[1]))
                r["d_finf"], r["b_finf"] = through_norm(r["d_finf"], r["b_finf"], xf, rn[R:], 1.0)
        ep, ef = np.abs(d_pred - ref["d_pred"]), np.abs(d_finf - ref["d_finf"])
        assert (ep <= ref["b_pred"]).all() and (ef <= ref["b_finf"]).all(), (tag, float((ep / ref["b_pred"]).max()), float((ef / ref["b_finf"]).max()))
        line += f", d_pred {float((ep / ref['b_pred']).max()):.3g}, d_finf {float((ef / ref['b_finf']).max()):.3g}"
        # the row direction alone misses d_finf: the keys' gradient is where the column softmax goes
        miss = float((np.abs(d_finf - plain["d_finf"]) > plain["b_finf"]).mean())
        line += f"; W = 0 misses {miss:.3f} of d_finf"
        assert miss > 0.5, (tag, miss)
    report(line + " of their bounds")
    return finf, ref


def case_by_hand(cfg: Cfg, arm: str, k_slots: int, cosine: bool = False, report=print):
    c = arm_cfg(cfg, arm)
    W = 0.5
    eng = engine(c, W, k_slots)
    if cosine:
        eng.set_score_norm("cosine", 0.25)
    batches = []
    for j, x in enumerate(inputs(c, 4 if k_slots else 2)):
        finf, _ = hand_step(eng, x, nq.live_keys(batches, k_slots) if k_slots else [], W, report,
                            f"{arm} bank {k_slots}{' cosine' if cosine else ''} step {j}")
        eng.adam_step()
        batches.append(finf)
        if k_slots:
            nq.check_ring(eng, batches)
    kc.all_finite(eng.flat_p)


def case_eval_between(cfg: Cfg, arm: str):
    c = arm_cfg(cfg, arm)
    eng, plain = engine(c, 0.5), engine(c)
    xs = inputs(c, 2)
    eng.train_step(xs[0])
    plain.flat_p.copy_(eng.flat_p)
    plain.packed_for_step = -1
    sr = eng._sym_result.clone()
    la, lb = eng._launches, plain._launches
    for e in (eng, plain):
        e.forward(xs[1], train=False, materialise=False)
        e.loss_topk(with_grad=False)
    assert torch.equal(bits(eng.result), bits(plain.result)) and torch.equal(bits(eng.row_ws), bits(plain.row_ws))
    assert eng._launches - la == plain._launches - lb and torch.equal(bits(sr), bits(eng._sym_result))
    sa, sb = eng.forward(xs[1], train=False), plain.forward(xs[1], train=False)   # forward(materialise=True) and its loss
    assert sa is not None and torch.equal(bits(sa), bits(sb)) and not eng._sym_live
    assert eng.forward(xs[1], train=True) is not None and not eng._sym_live       # the module boundary's training forward
    eng.forward(xs[1], train=False)
    eng.loss_topk(with_grad=True)
    plain.loss_topk(with_grad=True)
    assert torch.equal(bits(eng.dscore), bits(plain.dscore)) and torch.equal(bits(eng.result), bits(plain.result))


def case_accum_and_guard(cfg: Cfg, report=print):
    """accumulation 2 with the loss held by hand on the second micro-batch, then a NaN micro-batch under skip_nonfinite: arenas still"""
    c = arm_cfg(cfg, "f32 logits")
    xs = inputs(c, 4)
    eng = engine(c, 0.5)
    eng.set_grad_accum(2)
    eng.set_grad_guard(skip_nonfinite=True)
    eng.train_step(xs[0])
    with pytest.raises(RuntimeError, match="accumulation cycle is open"):
        eng.set_loss_sym(0.25)
    hand_step(eng, xs[1], [], 0.5, report, "accumulation, micro-batch 1", grads=False)
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
    kc.all_finite(eng.flat_p, eng._sym_result)
    assert eng.step_count == 2


def case_checkpoint(cfg: Cfg, tmp_path):
    from dpc_amd import checkpoint as ckpt
    c = arm_cfg(cfg, "f32 logits")
    a, b, plain = engine(c, 0.5), engine(c, 0.5), engine(c)
    a.train_step(inputs(c, 1)[0])
    state = ckpt.build_state(a, 1, "resnet18", 0.0, 1)
    assert state["loss_sym"] == 0.5 and "loss_sym" not in ckpt.build_state(plain, 1, "resnet18", 0.0, 1)
    path = str(tmp_path / "epoch1.pth.tar")
    ckpt.save_checkpoint(state, filename=path)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ckpt.resume(b, path)            # the same weight: silent
    assert b.loss_sym == 0.5 and torch.equal(bits(b.flat_p), bits(a.flat_p))
    with pytest.warns(UserWarning, match="written with the symmetric-loss weight 0.5, this run continues with 0") as rec:
        ckpt.resume(plain, path)
    assert sum("symmetric-loss" in str(w.message) for w in rec) == 1 and plain.loss_sym == 0.0
    ppath = str(tmp_path / "plain.pth.tar")
    ckpt.save_checkpoint(ckpt.build_state(plain, 1, "resnet18", 0.0, 1), filename=ppath)
    with pytest.warns(UserWarning, match="symmetric-loss weight 0, this run continues with 0.5"):
        ckpt.resume(b, ppath)
    # the file is the reference's dictionary plus one top-level float: the keys the reference reads are all there
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert {"epoch", "net", "state_dict", "best_acc", "optimizer", "iteration"} <= set(ck) and isinstance(ck["loss_sym"], float)


def case_refusals(cfg: Cfg):
    from dpc_amd.engine import DPCEngine
    c = arm_cfg(cfg, "f32 logits")
    eng = engine(c)
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "abc", None):
        with pytest.raises(ValueError, match="set_loss_sym"):
            eng.set_loss_sym(bad)
    assert eng.loss_sym == 0.0
    fused = DPCEngine("resnet18", c.size, c.N, c.SL, c.P, c.B, c.device, BF16, c.widths, lib=c.simulator, score_path="fused")
    with pytest.raises(L.DpcError, match="fused"):
        fused.set_loss_sym(0.5)
    fused.set_loss_sym(0)   # off is never refused
    eng.set_neg_classes((0.5, 1, 1))
    with pytest.raises(L.DpcError, match="set_neg_classes"):
        eng.set_loss_sym(0.5)
    eng.set_neg_classes(report=True)
    with pytest.raises(L.DpcError, match="set_neg_classes"):
        eng.set_loss_sym(0.5)
    eng.set_neg_classes()
    eng.set_loss_sym(0.5)
    with pytest.raises(L.DpcError, match="symmetric loss"):   # ... and the other order
        eng.set_neg_classes((0.5, 1, 1))
    with pytest.raises(L.DpcError, match="symmetric loss"):
        eng.set_neg_classes(report=True)
    eng.set_neg_classes()   # off is never refused
    assert eng.loss_sym == 0.5 and eng.neg_classes == ((1.0, 1.0, 1.0), False)
    eng.set_loss_sym(0)
    eng.set_grad_accum(2)
    eng.train_step(inputs(c, 1)[0])
    with pytest.raises(RuntimeError, match="accumulation cycle is open"):
        eng.set_loss_sym(0.5)
    eng.reset_accum()
    eng.set_loss_sym(1.0)
    assert eng.loss_sym == 1.0
    if c.device != "cpu":
        t = torch.zeros(8, device=c.device)
        torch.cuda.synchronize()
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            t.add_(1.0)
            with pytest.raises(L.DpcError, match="captured"):
                eng.set_loss_sym(0.5)
        assert eng.loss_sym == 1.0


# ---------------------------------------------------------------------- the entry (simulator)
def case_entry(emu, widths, capsys, tmp_path):
    from dpc_amd import main as dpc_main
    common = ["--net", "resnet18", "--img_dim", "64", "--batch_size", "2", "--gpu", "0", "--print_freq", "1", "--num_seq", "4", "--epochs", "1",
              "--pred_step", "2", "--synthetic", "2"]
    run = lambda flags: (dpc_main.main(common + flags, _simulator=emu, _widths=widths), capsys.readouterr().out)[1]   # noqa: E731
    strip = lambda s: re.sub(r"T:\d+\.\d+", "T:", s)   # noqa: E731
    plain = run([])
    off = run(["--loss_sym", "0"])   # the default, spelled out
    assert strip(off) == strip(plain) and "Loss: symmetric" not in off and " Lr " not in off
    on = run(["--loss_sym", "0.5"])
    assert on.splitlines().count("Loss: symmetric, key-to-prediction weight 0.5") == 1, on
    tail = re.compile(r" Lr (\d+\.\d{4}) Lc (\d+\.\d{4}) c@1 (\d\.\d{4})$")
    lines = [ln for ln in on.splitlines() if ln.startswith("Epoch: [")]
    assert len(lines) == 2
    for ln in lines:
        m = tail.search(ln)
        assert m, ln
        loss = float(re.search(r"Loss (\d+\.\d+)", ln).group(1))
        assert abs(loss - 0.5 * (float(m.group(1)) + float(m.group(2)))) <= 2e-4, ln   # four printed decimals of each term
    cut = lambda s: [tail.sub("", ln) for ln in strip(s).splitlines() if ln.startswith("Epoch: [")]   # noqa: E731
    assert cut(on) != cut(off)   # the column direction changes the loss
    assert [ln for ln in strip(on).splitlines() if ln.startswith("[0/1]")] != []   # validation ran, without a tail
    assert not any(tail.search(ln) for ln in on.splitlines() if not ln.startswith("Epoch: ["))
    for flags in (["--loss_sym", "-0.5"], ["--loss_sym", "1.5"], ["--loss_sym", "nan"], ["--loss_sym", "0.5", "--neg_weight", "0.5,1,1"],
                  ["--loss_sym", "0.5", "--neg_report"]):
        with pytest.raises(ValueError, match="--loss_sym"):   # before a rank starts: nothing is printed
            dpc_main.main(common + flags, _simulator=emu, _widths=widths)
        assert capsys.readouterr().out == ""


# ---------------------------------------------------------------------- captured steps (HIP device only)
def case_captured(cfg: Cfg, arm: str, k_slots: int = 0, accum: int = 1):
    """a captured step under the symmetric loss replayed five times against an eager twin, bit for bit (with a bank: across the fill
    boundary and the wrap); the capture holds the plain capture's launches plus SYM_CALLS per step -- the same number on every route;
    a replay after set_loss_sym raises"""
    c = arm_cfg(cfg, arm)
    xs = inputs(c, 6 * accum)
    a, b = engine(c, 0.5, k_slots), engine(c, 0.5, k_slots)
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
        assert replay.micro.kernels == [ref.micro.kernels[0] + SYM_CALLS] and replay.last.kernels == [ref.last.kernels[0] + SYM_CALLS]
    else:
        assert replay.kernels == [ref.kernels[0] + SYM_CALLS]
    for j, x in enumerate(xs[accum:6 * accum]):
        block.copy_(x)
        ra = replay().clone()
        rb = b.train_step(x).clone()
        assert torch.equal(bits(ra), bits(rb)), j
        assert torch.equal(bits(a.flat_p), bits(b.flat_p)) and torch.equal(bits(a._sym_result), bits(b._sym_result)), j
        if k_slots:
            assert same(nq.ring_state(a), nq.ring_state(b)), j
    assert a.step_count == b.step_count == 6
    a.set_loss_sym(0.25)
    with pytest.raises(RuntimeError):
        replay()
    a.release_captures()
    plain.release_captures()
