"""The cosine score (csrc/score_norm.hip: dpc_rownorm_fwd / dpc_rownorm_bwd; DPCEngine.set_score_norm; DPC_RNN(score_norm=, temperature=);
main --score_norm cosine --temperature T), shared by the CPU tier (host SIMT simulator, tests/test_score_norm_emu.py) and the GPU tier
(tests/test_score_norm_gpu.py).

Bounds (no tolerance constants; u = 2^-24, h = 2^-8 for bf16 outputs -- half an ulp, and the same again for a value on the other side of a
rounding boundary -- and 0 for f32):
  forward y        |y - ref| <= (h + (D + 8) u) |ref| against F.normalize(x.double(), dim=1) * scale: D roundings of the sum of squares
                   in any order, and sqrt, the division, scale * rn, x * k and spare
  forward rnorm    relative (D + 8) u
  exact data       rows of m in {4, 16, 64, 256} entries +-2^e, scale 8: the sum of squares is a power of four, everything behind it a
                   power of two -- bit identity of y and rnorm
  backward         per element (D + 8) u scale rn (|g_d| + |u_d| sum |g u|) against the f64 autograd of the same expression; the same
                   reference without the projection term, and with scale = 1, must miss on >= 99 % of the elements
  clamped rows     x scale / eps and g scale / eps, three f32 roundings (1 / eps, scale * rn, the product): (1 + u)^3 - 1 (+ h), in f64
Engine cases: by_hand's docstring counts what it adds."""
import functools
import math
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grad_guard_cases as gc
import kcases as kc
import loss_cases as lc
import negq_cases as nq
from dpc_amd import _lib as L
from kcases import K

F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24
GUARD = lc.GUARD
EPS = 1e-12
EPS32 = float(np.float32(EPS))
RN_MAX = float(np.float32(1.0) / np.float32(EPS))   # rnorm of a clamped row
R3 = (1 + U) ** 3 - 1                               # three f32 roundings in a row
Cfg = gc.Cfg
bits = lc._bits

KERNEL_SHAPES = tuple((R, D) for R in (1, 5, 24, 130) for D in (32, 256))   # 5, 130: a partly filled last workgroup / lane group
KERNEL_SHAPES_GPU = KERNEL_SHAPES + ((1100, 256),)
DTYPES = (F32, BF16)
T_KERNEL = 0.07


def f32(v):
    return float(np.float32(v))


def half_ulp(dt):
    return 2.0 ** -8 if dt == BF16 else 0.0


def fwd_bound(D, dt):
    return half_ulp(dt) + (D + 8) * U


# ---------------------------------------------------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def rows_data(R, D, seed=0):
    """two operands [R][D] with row magnitudes spread over 0.01 .. 30, and gradients of mixed row scales; row R // 2 of the gradients is
    nearly parallel to its x (g = 0.37 x + 1e-3 noise), the cancellation case.  f64, computed once, never written to."""
    rng = np.random.Generator(np.random.PCG64(1000 * R + D + seed))
    out = []
    for _ in range(2):
        mag = 0.01 * 3000.0 ** rng.random(R)
        x = rng.standard_normal((R, D)) * mag[:, None] / math.sqrt(D)
        g = rng.standard_normal((R, D)) * (10.0 ** rng.uniform(-3, 1, R))[:, None]
        out += [x, g]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def quantised(a, dt):
    return torch.from_numpy(np.array(a)).to(torch.float32).to(dt)


class Buf:
    """a device buffer of n elements with GUARD poisoned elements in front of and behind it"""

    def __init__(self, k: K, n, dt, init=None):
        self.all = k.poison(n + 2 * GUARD, dtype=dt)
        self.v = self.all[GUARD:GUARD + n]
        if init is not None:
            self.v.copy_(init.reshape(-1).to(self.all.device))
        self.edge = self.edges()

    def edges(self):
        return torch.cat([bits(self.all[:GUARD]), bits(self.all[-GUARD:])])

    def guards_still(self):
        return torch.equal(self.edges(), self.edge)


def run_fwd(k: K, xa, xb, dt, sa, sb, eps=EPS):
    """one launch; xb may be None.  Returns (ya, yb, rnorm) as CPU tensors; the guard bands are held here"""
    R, D = xa.shape
    ya, yb = Buf(k, R * D, dt), (Buf(k, R * D, dt) if xb is not None else None)
    rn = Buf(k, 2 * R, F32)
    k.call("dpc_rownorm_fwd", k.t(xa), k.t(xb) if xb is not None else None, ya.v, yb.v if yb else None, rn.v, R, D, L.dtype_code(dt), sa, sb, eps)
    k.sync()
    assert ya.guards_still() and rn.guards_still() and (yb is None or yb.guards_still()), "written outside an output"
    if xb is None:
        assert bool(torch.isnan(rn.v[R:]).all()), "operand b's 1 / norm written without an operand b"
    return ya.v.cpu().view(R, D), (yb.v.cpu().view(R, D) if yb else None), rn.v.cpu()


def run_bwd(k: K, xa, xb, rn, ga, gb, dt, sa, sb, eps=EPS):
    """in place on guarded copies of ga / gb (f32).  Returns the two results as CPU tensors"""
    R, D = xa.shape
    a, b = Buf(k, R * D, F32, ga), (Buf(k, R * D, F32, gb) if xb is not None else None)
    k.call("dpc_rownorm_bwd", k.t(xa), k.t(xb) if xb is not None else None, k.t(rn), a.v, b.v if b else None, R, D, L.dtype_code(dt), sa, sb, eps)
    k.sync()
    assert a.guards_still() and (b is None or b.guards_still()), "written outside a gradient"
    return a.v.cpu().view(R, D), (b.v.cpu().view(R, D) if b else None)


# ---------------------------------------------------------------------------------------------------------------- K1 forward vs f64
def case_fwd(k: K, R, D, dt, report=print):
    xa64, _, xb64, _ = rows_data(R, D)
    xa, xb = quantised(xa64, dt), quantised(xb64, dt)
    sa = f32(1.0 / T_KERNEL)
    ya, yb, rn = run_fwd(k, xa, xb, dt, sa, 1.0)
    worst = 0.0
    for x, y, s, r in ((xa, ya, sa, rn[:R]), (xb, yb, 1.0, rn[R:])):
        ref = F.normalize(x.double(), dim=1) * s
        e, b = (y.double() - ref).abs(), fwd_bound(D, dt) * ref.abs()
        assert bool((e <= b).all()), f"({R}, {D}) {dt}: {int((~(e <= b)).sum())} elements outside the bound"
        want = 1.0 / x.double().norm(dim=1)
        er = (r.double() - want).abs() / want
        assert bool((er <= (D + 8) * U).all()), f"({R}, {D}) {dt}: rnorm {float(er.max()):.3g}"
        worst = max(worst, float((e[b > 0] / b[b > 0]).max()), float(er.max() / ((D + 8) * U)))
    again = run_fwd(k, xa, xb, dt, sa, 1.0)
    assert all(torch.equal(bits(p), bits(q)) for p, q in zip((ya, yb, rn), again)), "two runs differ"
    alone, none, rn1 = run_fwd(k, xa, None, dt, sa, 1.0)   # a NULL second operand
    assert none is None and torch.equal(bits(alone), bits(ya)) and torch.equal(bits(rn1[:R]), bits(rn[:R]))
    report(f"[rownorm-fwd] ({R}, {D}) {dt}: at most {worst:.3g} of the bound")
    return worst


# ---------------------------------------------------------------------------------------------------------------- K2 exact data
def case_exact(k: K, R, D, dt):
    rng = np.random.Generator(np.random.PCG64(7 * R + D))
    ms = (4, 16) if D == 32 else (4, 16, 64, 256)
    ops, refs = [], []
    for _ in range(2):
        x, y, r = np.zeros((R, D)), np.zeros((R, D)), np.zeros(R)
        for i in range(R):
            m = ms[(i + len(ops)) % len(ms)]
            a = 2.0 ** int(rng.integers(-6, 7))
            cols = rng.choice(D, m, replace=False)
            sg = rng.choice([-1.0, 1.0], m)
            x[i, cols] = sg * a
            y[i, cols] = sg * 8.0 / math.sqrt(m)
            r[i] = 1.0 / (math.sqrt(m) * a)
        ops.append(quantised(x, dt))
        refs.append((quantised(y, dt), torch.from_numpy(r).to(F32)))
    ya, yb, rn = run_fwd(k, ops[0], ops[1], dt, 8.0, 8.0)
    assert torch.equal(bits(ya), bits(refs[0][0])) and torch.equal(bits(yb), bits(refs[1][0])), f"({R}, {D}) {dt}: y is not exact"
    assert torch.equal(bits(rn), bits(torch.cat([refs[0][1], refs[1][1]]))), f"({R}, {D}) {dt}: rnorm is not exact"


# ---------------------------------------------------------------------------------------------------------------- K3 edges
def case_edges(k: K, R, D, dt):
    xa64, _, xb64, _ = rows_data(R, D)
    xa, xb = quantised(xa64, dt), quantised(xb64, dt)
    sa = f32(1.0 / T_KERNEL)
    zero, tiny = 0, R - 1                      # rows of operand a (the same row at R = 1: the tiny row then)
    xa[zero] = 0.0
    t64 = torch.from_numpy(np.array(xa64[tiny])).double()
    xa[tiny] = (t64 / t64.norm() * 1e-20).to(F32).to(dt)
    ya, yb, rn = run_fwd(k, xa, xb, dt, sa, 1.0)
    if R > 1:
        assert not bits(ya[zero]).any() and float(rn[zero]) == RN_MAX, "a zero row must give +0 and 1 / eps"
    assert float(rn[tiny]) == RN_MAX
    ref = xa[tiny].double() * sa / EPS32
    assert float(ref.abs().max()) > 0
    e = (ya[tiny].double() - ref).abs()
    assert bool((e <= (half_ulp(dt) + R3) * (1 + half_ulp(dt)) * ref.abs()).all()), "a row below eps must give x scale / eps"
    # a NaN row leaves every other row as it was
    xn = xb.clone()
    xn[R // 2] = float("nan")
    ya2, yb2, rn2 = run_fwd(k, xa, xn, dt, sa, 1.0)
    keep = torch.arange(R) != R // 2
    assert torch.equal(bits(ya2), bits(ya)) and torch.equal(bits(yb2[keep]), bits(yb[keep]))
    assert torch.equal(bits(rn2[:R]), bits(rn[:R])) and torch.equal(bits(rn2[R:][keep]), bits(rn[R:][keep]))
    assert bool(torch.isnan(yb2[R // 2].float()).all()) and bool(torch.isnan(rn2[R + R // 2]))
    # the backward's clamped arm: g scale / eps
    _, ga64, _, gb64 = rows_data(R, D)
    ga, gb = quantised(ga64, F32), quantised(gb64, F32)
    da, _ = run_bwd(k, xa, xb, rn, ga, gb, dt, sa, 1.0)
    for row in {zero, tiny}:
        want = ga[row].double() * sa / EPS32
        assert bool(((da[row].double() - want).abs() <= R3 * want.abs()).all()), f"clamped row {row}: not g scale / eps"


# ---------------------------------------------------------------------------------------------------------------- K4 backward vs f64
def bwd_reference(x, g, scale, project=True):
    """f64: the autograd of F.normalize(x) * scale (project) or the same without the projection term; and the bound's magnitude"""
    x64, g64 = x.double(), g.double()
    rn = 1.0 / x64.norm(dim=1, keepdim=True)
    u = x64 * rn
    if project:
        leaf = x64.clone().requires_grad_()
        (F.normalize(leaf, dim=1, eps=EPS) * scale * g64).sum().backward()
        ref = leaf.grad
    else:
        ref = scale * rn * g64
    mag = scale * rn * (g64.abs() + u.abs() * (g64 * u).abs().sum(1, keepdim=True))
    return ref, mag


def case_bwd(k: K, R, D, dt, report=print):
    xa64, ga64, xb64, gb64 = rows_data(R, D)
    xa, xb = quantised(xa64, dt), quantised(xb64, dt)
    ga, gb = quantised(ga64, F32), quantised(gb64, F32)
    c = R // 2    # the cancellation row: g nearly parallel to x
    noise = torch.from_numpy(np.random.Generator(np.random.PCG64(R + D)).standard_normal(D)).to(F32)
    ga[c] = (0.37 * xa[c].float() + 1e-3 * xa[c].float().abs().max() * noise)
    sa = f32(1.0 / T_KERNEL)
    _, _, rn = run_fwd(k, xa, xb, dt, sa, 1.0)
    da, db = run_bwd(k, xa, xb, rn, ga, gb, dt, sa, 1.0)
    worst, missed = 0.0, []
    for x, g, s, d in ((xa, ga, sa, da), (xb, gb, 1.0, db)):
        ref, mag = bwd_reference(x, g, s)
        bound = (D + 8) * U * mag
        e = (d.double() - ref).abs()
        assert bool((e <= bound).all()), f"({R}, {D}) {dt}: {int((~(e <= bound)).sum())} elements outside the bound, worst {float((e / bound).max()):.3g}"
        worst = max(worst, float((e / bound).max()))
        flat, _ = bwd_reference(x, g, s, project=False)
        missed.append(float(((d.double() - flat).abs() > bound).double().mean()))
        if s != 1.0:
            one, _ = bwd_reference(x, g, 1.0)
            missed.append(float(((d.double() - one).abs() > bound).double().mean()))
    report(f"[rownorm-bwd] ({R}, {D}) {dt}: at most {worst:.3g} of the bound; the mutated references miss on {min(missed):.4f} of the elements at least")
    assert min(missed) >= 0.99, missed
    # in place == a copy-out twin: every row on its own, in a buffer of its own, gives the bits the whole pass gave
    for row in sorted({0, c, R - 1} | set(range(0, R, max(1, R // 8)))):
        one, _ = run_bwd(k, xa[row:row + 1], None, rn[row:row + 1], ga[row:row + 1], None, dt, sa, 1.0)
        assert torch.equal(bits(one), bits(da[row:row + 1])), f"row {row}: in place differs from the row alone"
        two, _ = run_bwd(k, xb[row:row + 1], None, rn[R + row:R + row + 1], gb[row:row + 1], None, dt, 1.0, 1.0)
        assert torch.equal(bits(two), bits(db[row:row + 1])), f"row {row} of operand b"
    again = run_bwd(k, xa, xb, rn, ga, gb, dt, sa, 1.0)
    assert torch.equal(bits(again[0]), bits(da)) and torch.equal(bits(again[1]), bits(db)), "two runs differ"
    return worst


# ---------------------------------------------------------------------------------------------------------------- K5 refused calls
def case_refused(k: K):
    R, D = 24, 32
    x0 = torch.randn((R, D), generator=torch.Generator().manual_seed(1))
    for dt in DTYPES:
        x, y, rn, g = k.t(x0, dt), k.poison(R * D, dtype=dt), k.poison(2 * R), k.t(x0)
        g0 = g.clone()
        off = k.t(torch.randn(R * D + 8).to(dt))[1:]   # one element off a 16-byte boundary
        goff = k.t(torch.randn(R * D + 8))[1:]
        dc = L.dtype_code(dt)
        arg, uns = f"code {L.ERR_ARG}$", f"code {L.ERR_UNSUPPORTED}$"
        fw, bw = (lambda *a: k.call("dpc_rownorm_fwd", *a)), (lambda *a: k.call("dpc_rownorm_bwd", *a))
        inf, nan = float("inf"), float("nan")
        bad = [
            (arg, lambda: fw(None, None, y, None, rn, R, D, dc, 1.0, 1.0, EPS)),
            (arg, lambda: fw(x, None, None, None, rn, R, D, dc, 1.0, 1.0, EPS)),
            (arg, lambda: fw(x, None, y, None, None, R, D, dc, 1.0, 1.0, EPS)),
            (arg, lambda: fw(x, x, y, None, rn, R, D, dc, 1.0, 1.0, EPS)),       # an operand b without its output
            (arg, lambda: fw(x, None, y, y, rn, R, D, dc, 1.0, 1.0, EPS)),       # ... and the other way round
            (arg, lambda: fw(off, None, y, None, rn, R, D, dc, 1.0, 1.0, EPS)),
            (arg, lambda: fw(x, None, off, None, rn, R, D, dc, 1.0, 1.0, EPS)),
            (arg, lambda: fw(x, None, y, None, rn, 0, D, dc, 1.0, 1.0, EPS)),
            (arg, lambda: fw(x, None, y, None, rn, -3, D, dc, 1.0, 1.0, EPS)),
            (arg, lambda: fw(x, None, y, None, rn, R, D, 7, 1.0, 1.0, EPS)),
            (uns, lambda: fw(x, None, y, None, rn, R, 64, dc, 1.0, 1.0, EPS)),
            (uns, lambda: fw(x, None, y, None, rn, R, 0, dc, 1.0, 1.0, EPS)),
            (arg, lambda: bw(None, None, rn, g, None, R, D, dc, 1.0, 1.0, EPS)),
            (arg, lambda: bw(x, None, None, g, None, R, D, dc, 1.0, 1.0, EPS)),
            (arg, lambda: bw(x, None, rn, None, None, R, D, dc, 1.0, 1.0, EPS)),
            (arg, lambda: bw(x, x, rn, g, None, R, D, dc, 1.0, 1.0, EPS)),
            (arg, lambda: bw(x, None, rn, goff, None, R, D, dc, 1.0, 1.0, EPS)),
            (arg, lambda: bw(x, None, rn, g, None, 0, D, dc, 1.0, 1.0, EPS)),
            (uns, lambda: bw(x, None, rn, g, None, R, 64, dc, 1.0, 1.0, EPS)),
        ]
        for v in (0.0, -1.0, inf, nan):   # a scale or an eps that is not finite and positive
            bad += [(arg, lambda v=v: fw(x, None, y, None, rn, R, D, dc, v, 1.0, EPS)), (arg, lambda v=v: fw(x, None, y, None, rn, R, D, dc, 1.0, v, EPS)),
                    (arg, lambda v=v: fw(x, None, y, None, rn, R, D, dc, 1.0, 1.0, v)), (arg, lambda v=v: bw(x, None, rn, g, None, R, D, dc, v, 1.0, EPS)),
                    (arg, lambda v=v: bw(x, None, rn, g, None, R, D, dc, 1.0, 1.0, v))]
        for code, f in bad:
            with pytest.raises(L.DpcError, match=code):
                f()
        k.sync()
        assert bool(torch.isnan(y.float()).all()) and bool(torch.isnan(rn).all()) and torch.equal(bits(g), bits(g0))


# ================================================================================================================ engine
ARMS = nq.ARMS
arm_cfg = nq.arm_cfg
inputs = nq.inputs


def engine(cfg: Cfg, dt=BF16, T=None, k_slots=0, **kw):
    if kw:
        from dpc_amd.engine import DPCEngine
        from oracle import dpc_oracle as O
        eng = DPCEngine("resnet18", cfg.size, cfg.N, cfg.SL, cfg.P, cfg.B, cfg.device, dt, cfg.widths, lib=cfg.simulator, **kw)
        eng.load_params(O.make_params_pcg("resnet18", cfg.widths))
    else:
        eng = gc.dpc_engine(cfg, dt)
    if T is not None:
        eng.set_score_norm("cosine", T)
    if k_slots:
        eng.set_neg_queue(k_slots)
    return eng


def all_arenas(eng):
    return nq.all_arenas(eng) + [eng.flat_g.detach().clone()]


same = nq.same


def case_off_is_off(cfg: Cfg, arm: str, dt=BF16):   # E1
    c = arm_cfg(cfg, arm)
    a, b = engine(c, dt), engine(c, dt)
    b.set_score_norm("cosine", 0.2)
    assert b.score_norm == ("cosine", 0.2) and b.pred_n is not None and ("score_norm", "cosine", 0.2) in b._baked_scalars()
    b.set_score_norm("dot", 1.0)
    assert b.score_norm == a.score_norm == ("dot", 1.0) and b.pred_n is None and b.finf_n is None and b.rnorm is None
    assert b._baked_scalars() == a._baked_scalars()
    la, lb = a._launches, b._launches
    for x in inputs(c, 2):
        ra, rb = a.train_step(x).clone(), b.train_step(x).clone()
        assert torch.equal(bits(ra), bits(rb)) and same(all_arenas(a), all_arenas(b))
        assert torch.equal(bits(a.pred), bits(b.pred)) and torch.equal(bits(a.d_pred), bits(b.d_pred)) and torch.equal(bits(a.d_finf), bits(b.d_finf))
    assert a._launches - la == b._launches - lb


def operands(eng):
    R, D = eng.R, eng.D
    return [t.detach().reshape(R, D).cpu().clone() for t in (eng.pred, eng.feat_inf, eng.pred_n, eng.finf_n)]


def f64_terms(P, Fk, scale, normalise=True):
    """every row's loss term of the in-batch contrastive loss from raw operands, in f64"""
    P, Fk = P.double(), Fk.double()
    if normalise:
        P, Fk = F.normalize(P, dim=1, eps=EPS), F.normalize(Fk, dim=1, eps=EPS)
    S = (P * scale) @ Fk.t()
    return (torch.logsumexp(S, 1) - S.diagonal()).numpy()


def hand_step(eng, x, bank_keys, T, report, tag, mutations=False):
    """One training step of the cosine score taken apart and held to f64, link by link:

      1. pred_n / finf_n against F.normalize of the step's own raw pred / feat_inf in f64, times float32(1 / T): the forward kernel's
         bound, (h + (D + 8) u) |ref| per element; rnorm likewise.
      2. every row's loss term and rank, the mean, and the score backward's d_pred / d_finf against negq_cases.hand_reference on the
         normalised operands as the device holds them (exact inputs of the contraction): its bounds, unchanged -- the in-batch logits
         as the loss kernel read them, one f32 rounding per accumulated product, the bf16 rounding of dS.
      3. d_pred / d_finf after dpc_rownorm_bwd against the f64 projection of 2.'s f64 gradient G.  The projection is linear in G, so
         what 2. allows (b, per element) passes through it as scale rn (b_d + |u_d| sum_e |u_e| b_e), and the kernel adds its own
         (D + 8) u scale rn (|G_d| + |u_d| sum |G u|).  Nothing else is rounded in between: the kernel reads the f32 gradients the
         score backward wrote.
    mutations (case_by_hand): the same f64 loss terms at 2 T, and without the normalisation, must each miss every row's term by more
    than the row kernel's f32 arithmetic allows (counted there); and the unmutated f64 chain from the raw operands lies where 1. and 2. put it."""
    R, D = eng.R, eng.D
    dt = eng.cdtype
    scale = f32(1.0 / T)
    eng._forward_loss(x, True)
    P, Fk, Pn, Fn = operands(eng)
    rn = eng.rnorm.detach().cpu().double()
    s_in = (eng.score16 if eng._score16_live else eng.score).detach().cpu().clone()
    res = eng.result.detach().cpu().clone()
    rows = eng.row_ws.detach().cpu().double().numpy().reshape(R, 2).copy()
    eng.backward()
    d_pred, d_finf = eng.d_pred.detach().reshape(R, D).cpu().double(), eng.d_finf.detach().reshape(R, D).cpu().double()
    # 1.
    worst1 = 0.0
    for raw, got, s, r in ((P, Pn, scale, rn[:R]), (Fk, Fn, 1.0, rn[R:])):
        ref = F.normalize(raw.double(), dim=1, eps=EPS) * s
        e, b = (got.double() - ref).abs(), fwd_bound(D, dt) * ref.abs()
        assert bool((e <= b).all()), (tag, "normalised operand", float((e[b > 0] / b[b > 0]).max()))
        want = 1.0 / raw.double().norm(dim=1)
        assert bool(((r - want).abs() <= (D + 8) * U * want).all()), (tag, "rnorm")
        worst1 = max(worst1, float((e[b > 0] / b[b > 0]).max()))
    # 2.
    ref = nq.hand_reference(Pn, Fn, s_in, bank_keys, eng._score16_live)
    er = np.abs(rows[:, 0] - ref["term"])
    assert (er < ref["rbound"]).all(), (tag, np.nonzero(~(er < ref["rbound"]))[0][:8].tolist(), float((er / ref["rbound"]).max()))
    assert np.array_equal(rows[:, 1], ref["rank"].astype(np.float64)), (tag, "rank")
    assert abs(float(res[0]) - ref["loss"]) < ref["lbound"], (tag, float(res[0]), ref["loss"], ref["lbound"])
    for i, kk in enumerate((1, 3, 5)):
        assert float(res[1 + i]) == float(np.float32(int((ref["rank"] < kk).sum())) / np.float32(R)), (tag, kk)
    if mutations:
        # The row kernel's own arithmetic on the logits it read, without the dropped-column quarter of hand_reference (at R = 8 and
        # near-uniform rows that quarter is 0.03, more than the temperature moves a row): with b the largest of |mx|, |tgt|, |lse|,
        # |term|, the argument of each exponential is s - mx rounded and scaled (2 roundings of a value below 2 b) and the exponential
        # one more -- (4 b + 2) u relative per term; the sum of R positive terms R u more; the logarithm turns that into an absolute
        # error and adds u log R; + mx - tgt two roundings at b.  Together below (6 b + 2 R + 4) u.
        S = s_in.double().numpy()
        mx, tgt = S.max(1), np.diagonal(S)
        big = np.maximum(np.maximum(np.abs(mx), np.abs(tgt)), np.maximum(np.abs(ref["term"] + tgt), np.abs(ref["term"])))
        tbound = (6 * big + 2 * R + 4) * U
        assert (er <= tbound).all(), (tag, "row arithmetic", float((er / tbound).max()))
        for what, terms in (("2 T", f64_terms(P, Fk, scale / 2)), ("no normalisation", f64_terms(P, Fk, scale, normalise=False))):
            miss = np.abs(rows[:, 0] - terms) > tbound
            assert miss.all(), (tag, what, "rows it does not miss:", np.nonzero(~miss)[0].tolist())
        full = f64_terms(P, Fk, scale)   # and the unmutated f64 chain from the raw operands lies where 1. and 2. put it
        # a logit is at most 1 / T in size: both operands' rounding (1.) and the rounding of the logit itself move it by `moved` at most,
        # and a row's term by no more than twice its worst logit
        moved = (2 * fwd_bound(D, dt) + fwd_bound(D, dt) ** 2) * scale + (2.0 ** -8 if eng._score16_live else D * 2.0 ** -23) * scale
        assert (np.abs(rows[:, 0] - full) <= ref["rbound"] + 2 * moved).all(), (tag, "raw f64 chain")
    # 3.
    worst3 = 0.0
    for raw, G, bG, got, s, r in ((P, ref["d_pred"], ref["b_pred"], d_pred, scale, rn[:R]), (Fk, ref["d_finf"], ref["b_finf"], d_finf, 1.0, rn[R:])):
        x64 = raw.double()
        rr = 1.0 / x64.norm(dim=1, keepdim=True)
        u = x64 * rr
        G, bG = torch.from_numpy(G), torch.from_numpy(bG)
        want = s * rr * (G - u * (G * u).sum(1, keepdim=True))
        bound = s * rr * (bG + u.abs() * (u.abs() * bG).sum(1, keepdim=True)) + (D + 8) * U * s * rr * (G.abs() + u.abs() * (G * u).abs().sum(1, keepdim=True))
        e = (got - want).abs()
        assert bool((e <= bound).all()), (tag, "projected gradient", float((e[bound > 0] / bound[bound > 0]).max()))
        worst3 = max(worst3, float((e[bound > 0] / bound[bound > 0]).max()))
    report(f"[score-norm] {tag}: loss {float(res[0]):.5f} (f64 {ref['loss']:.5f}); operands {worst1:.3g}, rows {float((er / ref['rbound']).max()):.3g}, "
           f"projected gradients {worst3:.3g} of their bounds")
    return Fn, ref


def case_by_hand(cfg: Cfg, arm: str, T: float, dt=BF16, report=print):   # E2
    c = arm_cfg(cfg, arm)
    eng = engine(c, dt, T)
    hand_step(eng, inputs(c, 1)[0], [], T, report, f"{arm} {dt} T {T}", mutations=True)
    eng.adam_step()
    assert eng.step_count == 1


def case_range_and_norms(cfg: Cfg, arm: str, dt=BF16, T=0.07):   # E3 + E4 (i), (ii)
    c = arm_cfg(cfg, arm)
    eng = engine(c, dt, T)
    R, D = eng.R, eng.D
    x = inputs(c, 1)[0]
    n0 = eng._launches
    score = eng.forward(x, train=False).detach().cpu().clone().view(R, R)
    launches = eng._launches - n0
    e1 = fwd_bound(D, dt)
    bound = 2 * e1 + e1 * e1 + D * 2.0 ** -23    # both operands' rounding, and the f32 accumulation of D products
    assert 0 < float(score.abs().max()) <= (1.0 / T) * (1 + bound)
    _, _, Pn, Fn = operands(eng)
    sq = 2 * e1 + e1 * e1 + 2 * U
    assert bool((((Pn.double() ** 2).sum(1) * T * T - 1).abs() <= sq + 2 * U).all()) and bool((((Fn.double() ** 2).sum(1)) - 1).abs().le(sq).all())
    # scale of the keys: feat_inf times 4 in front of the normalisation (a power of two: every product is exact) -- the same score bits
    twin = engine(c, dt, T)
    call = twin.call

    def hooked(name, *args):
        if name == "dpc_rownorm_fwd":
            twin.feat_inf.mul_(4.0)
        return call(name, *args)
    twin.call = hooked
    s4 = twin.forward(x, train=False).detach().cpu().view(R, R)
    assert torch.equal(bits(twin.feat_inf.cpu()), bits((eng.feat_inf * 4.0).cpu())) and torch.equal(bits(s4), bits(score))
    # ... while the dot-product score of the same keys is four times as large
    plain = engine(c, dt)
    n1 = plain._launches
    sp = plain.forward(x, train=False).detach().cpu().view(R, R)
    assert launches == plain._launches - n1 + 1, "one launch more per evaluation step"
    assert torch.equal(bits(plain.pred), bits(eng.pred)) and torch.equal(bits(plain.feat_inf), bits(eng.feat_inf)), "pred / feat_inf keep the raw values"
    assert not torch.equal(bits(sp), bits(score))


def case_predictor_scale(cfg: Cfg, arm: str, dt=BF16, T=0.07):   # E4 (iii)
    """network_pred.2.weight and .bias times 4 scale pred by exactly 4 (a power of two through f32 accumulators and one rounding): the
    score keeps its bits, and the projection leaves the gradient of those two parameters at a quarter -- exactly, every factor on the
    way being the same power of two"""
    from oracle import dpc_oracle as O
    c = arm_cfg(cfg, arm)
    x = inputs(c, 1)[0]
    out = []
    for mult in (1.0, 4.0):
        eng = engine(c, dt, T)
        prm = O.make_params_pcg("resnet18", c.widths)
        for name in ("network_pred.2.weight", "network_pred.2.bias"):
            prm[name] = prm[name] * mult
        eng.load_params(prm)
        s = eng.forward(x, train=False).detach().cpu().clone()
        eng.loss_topk(True)
        eng.backward()
        out.append((s, eng.pred.detach().float().cpu().clone(), {n: eng.G[n].detach().cpu().clone() for n in ("network_pred.2.weight", "network_pred.2.bias")},
                    eng.d_pred.detach().cpu().clone()))
    (s1, p1, g1, d1), (s4, p4, g4, d4) = out
    assert torch.equal(p4, 4 * p1) and torch.equal(bits(s4), bits(s1))
    bound = (eng.D + 8) * U
    assert bool(((4 * d4 - d1).abs() <= bound * d1.abs()).all())
    for n in g1:
        assert float(g1[n].abs().max()) > 0 and bool(((4 * g4[n] - g1[n]).abs() <= bound * g1[n].abs().max()).all()), n


def case_queue(cfg: Cfg, arm: str, T=0.2, report=print):   # E5
    c = arm_cfg(cfg, arm)
    eng = engine(c, BF16, T, k_slots=2)
    R, D = eng.R, eng.D
    assert eng.score_norm == ("cosine", T) and eng.neg_queue == 2
    batches = []
    for j, x in enumerate(inputs(c, 3)):   # the third step wraps: it overwrites slot 0
        fn, _ = hand_step(eng, x, nq.live_keys(batches, 2), T, report, f"{arm} queue step {j}")
        eng.adam_step()
        batches.append(fn)
        nq.check_ring(eng, batches)   # the ring holds the NORMALISED keys, bit for bit
        live = eng._negq_ring[:min(j + 1, 2), :R].detach().cpu().double()
        assert bool(((live.norm(dim=2) - 1).abs() <= 2.0 ** -8 + (D + 8) * U).all()), "a live ring row is not of unit norm"
    eng.set_score_norm("cosine", 2 * T)
    assert eng.neg_queue_filled() == 0 and eng.neg_queue == 2, "set_score_norm empties the bank"


def case_module(cfg: Cfg, arm: str):   # E6
    from dpc_amd.model import DPC_RNN
    from oracle import dpc_oracle as O
    c = arm_cfg(cfg, arm)
    x = inputs(c, 1)[0]
    prm = O.make_params_pcg("resnet18", c.widths)

    def module(**kw):
        m = DPC_RNN(c.size, c.N, c.SL, c.P, "resnet18", widths=c.widths, _simulator=c.simulator, **kw)
        m.load_state_dict(prm, strict=True)
        return m.to(c.device).eval()

    def target_loss(score, mask):
        B, NP, SQ, B2, NS, _ = mask.size()
        tgt = (mask == 1).view(B * NP * SQ, B2 * NS * SQ).to(int).argmax(dim=1)
        return F.cross_entropy(score.view(B * NP * SQ, B2 * NS * SQ), tgt)
    m = module(score_norm="cosine", temperature=0.1)
    score, mask = m(x)
    assert m.engine.score_norm == ("cosine", 0.1)
    eng = engine(c, F32, 0.1)
    want = eng.forward(x, train=False)
    assert torch.equal(bits(score.detach()), bits(want)), "the module does not return the engine's score"
    assert float(score.detach().abs().max()) <= 10.0 * (1 + 2 * fwd_bound(eng.D, F32) + eng.D * 2.0 ** -23)
    target_loss(score, mask).backward()   # through backward(dscore_external): the normalisation's backward runs there too
    eng.loss_topk(True)
    eng.backward()
    named = dict(m.named_parameters())
    for kname, (o, n) in eng.offsets.items():
        a, b = named[kname].grad.detach().reshape(-1).cpu(), eng.flat_g[o:o + n].cpu()
        assert float((a - b).abs().max()) <= 2e-5 * max(float(b.abs().max()), 1e-6), kname
    d, plain = module(), engine(c, F32)
    assert (d.score_norm, d.temperature) == ("dot", 1.0)
    s0 = d(x)[0]
    assert torch.equal(bits(s0.detach()), bits(plain.forward(x, train=False))) and d.engine.score_norm == ("dot", 1.0) and d.engine.pred_n is None
    for kw in (dict(score_norm="cos"), dict(temperature=0.5), dict(score_norm="cosine", temperature=0.0), dict(score_norm="cosine", temperature=float("nan"))):
        with pytest.raises(ValueError):
            DPC_RNN(c.size, c.N, c.SL, c.P, "resnet18", widths=c.widths, **kw)


def case_combination(cfg: Cfg, arm: str, T=0.1):   # E7
    """guard + accumulation (N = 2) + EMA + schedule under the cosine score, against a twin that takes the cycle apart with the engine's
    own calls (forward + loss, backward, the mean of the two gradients in torch's f32 -- (0 + g0) + g1, then times 1/2: the roundings
    of dpc_grad_accumulate --, one guarded step); then a cycle whose second micro-batch is NaN: skipped on both, nothing moves"""
    from dpc_amd.optim import LRSchedule
    c = arm_cfg(cfg, arm)
    xs = inputs(c, 4)
    xs[3] = xs[3].clone()
    xs[3].view(-1)[17] = float("nan")

    def make(accum):
        e = engine(c, BF16, T)
        e.set_grad_guard(max_norm=0.5, skip_nonfinite=True)
        e.set_ema(0.9)
        e.set_lr_schedule(LRSchedule("cosine", warmup_steps=1, total_steps=4))
        if accum:
            e.set_grad_accum(2)
        return e
    a, b = make(True), make(False)

    def by_hand(x0, x1):
        b._forward_loss(x0, True)
        b.backward()
        g0 = b.flat_g.clone()
        b._forward_loss(x1, True)
        b.backward()
        b.flat_g.copy_(((0.0 + g0) + b.flat_g) * 0.5)
        b.adam_step()
    a.train_step(xs[0])
    assert a.accum_pending == 1 and a.step_count == 0
    a.train_step(xs[1])
    by_hand(xs[0], xs[1])
    assert a.step_count == b.step_count == 1 and a.grad_stats()["skip"] == 0
    assert same(nq.all_arenas(a), nq.all_arenas(b)) and torch.equal(bits(a.flat_ema), bits(b.flat_ema)) and torch.equal(bits(a.flat_g), bits(b.flat_g))
    before = nq.all_arenas(a) + [a.flat_ema.clone()]
    a.train_step(xs[2])
    a.train_step(xs[3])
    by_hand(xs[2], xs[3])
    assert a.step_count == b.step_count == 1 and a.grad_stats()["skip"] == 1 and b.grad_stats()["skip"] == 1
    assert same(nq.all_arenas(a) + [a.flat_ema], before) and same(nq.all_arenas(b) + [b.flat_ema], before)


def case_checkpoint(cfg: Cfg, arm: str, tmp_path):   # E8
    import torch.nn as nn
    from dpc_amd import checkpoint as ckpt
    from dpc_amd.model import DPC_RNN
    c = arm_cfg(cfg, arm)
    a, b, plain = engine(c, BF16, 0.07), engine(c, BF16, 0.07), engine(c, BF16)
    a.train_step(inputs(c, 1)[0])
    state = ckpt.build_state(a, 1, "resnet18", 0.0, 1)
    assert state["score_norm"] == {"kind": "cosine", "temperature": 0.07} and "score_norm" not in ckpt.build_state(plain, 1, "resnet18", 0.0, 1)
    path, ppath = str(tmp_path / "cos" / "epoch1.pth.tar"), str(tmp_path / "dot" / "epoch1.pth.tar")
    for p, st in ((path, state), (ppath, ckpt.build_state(plain, 1, "resnet18", 0.0, 1))):
        (tmp_path / ("cos" if p == path else "dot")).mkdir()
        ckpt.save_checkpoint(st, filename=p)
    info = ckpt.resume(b, path)
    assert info["epoch"] == 1 and b.score_norm == ("cosine", 0.07) and b.step_count == 1
    assert torch.equal(bits(b.flat_p), bits(a.flat_p)) and torch.equal(bits(b.flat_m), bits(a.flat_m))
    before = plain.flat_p.clone()
    with pytest.raises(ValueError, match="cosine score at temperature 0.07"):   # the kind disagrees
        ckpt.resume(plain, path)
    assert torch.equal(bits(plain.flat_p), bits(before)), "a refused file must leave the engine as it was"
    b.set_score_norm("cosine", 0.1)
    with pytest.raises(ValueError, match="temperature 0.07.*temperature 0.1"):   # T disagrees
        ckpt.resume(b, path)
    with pytest.raises(ValueError, match="dot score"):
        ckpt.resume(b, ppath)
    ckpt.resume(plain, ppath)
    ckpt.pretrain(plain, path, log=lambda *_: None)   # --pretrain reads named weights only
    # the reference's resume lines (dpc/main.py:91-98) still read the file
    model = nn.DataParallel(DPC_RNN(sample_size=c.size, num_seq=c.N, seq_len=c.SL, pred_step=c.P, network="resnet18", widths=c.widths))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    ck = torch.load(path, map_location=torch.device("cpu"), weights_only=False)
    model.load_state_dict(ck["state_dict"])
    opt.load_state_dict(ck["optimizer"])
    named = dict(model.module.named_parameters())
    assert all(torch.equal(named[n].detach().cpu(), a.PRM[n].cpu()) for n in a.PRM)   # (DataParallel moves its module to the device when there is one)


def case_refusals(cfg: Cfg, arm: str):   # E10
    from dpc_amd.engine import DPCEngine
    c = arm_cfg(cfg, arm)
    eng = engine(c, BF16)
    for kind, T in (("cosine", 0.0), ("cosine", -0.1), ("cosine", float("inf")), ("cosine", float("nan")), ("cosine", 1e-45), ("cos", 1.0), ("dot", 0.5)):
        with pytest.raises(ValueError, match="set_score_norm"):
            eng.set_score_norm(kind, T)
    assert eng.score_norm == ("dot", 1.0) and eng.pred_n is None
    if c.simulator is not None:   # a feature size the kernels do not serve (the GPU tier runs the reference's widths: D = 256)
        odd = DPCEngine("resnet18", c.size, c.N, c.SL, c.P, c.B, c.device, BF16, (8, 16, 32, 64), lib=c.simulator)
        with pytest.raises(L.DpcError, match="256 or 32"):
            odd.set_score_norm("cosine", 0.1)
        odd.set_score_norm("dot", 1.0)
    for dt, path in ((F32, "auto"), (BF16, "fused")):   # every compute dtype and the fused route take it
        e = DPCEngine("resnet18", c.size, c.N, c.SL, c.P, c.B, c.device, dt, c.widths, lib=c.simulator, score_path=path)
        e.set_score_norm("cosine", 0.3)
        assert e.score_norm == ("cosine", 0.3)
    eng.set_grad_accum(2)
    eng.train_step(inputs(c, 1)[0])
    with pytest.raises(RuntimeError, match="accumulation cycle is open"):
        eng.set_score_norm("cosine", 0.1)
    eng.reset_accum()
    eng.set_score_norm("cosine", 0.1)
    if c.device != "cpu":
        t = torch.zeros(8, device=c.device)
        torch.cuda.synchronize()
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            t.add_(1.0)
            with pytest.raises(L.DpcError, match="captured"):
                eng.set_score_norm("cosine", 0.2)
        assert eng.score_norm == ("cosine", 0.1)


def case_fused_route(cfg: Cfg, arm: str, T=0.2):   # E10b: score_path="fused" reads the normalised operands too
    """the fused route (no [R][R] tensor) against the materialised one on the same step: the same operands, so the loss agrees within
    what the two routes differ by without the cosine score, and the projected gradients are held by the kernel's bound on the
    route's own pre-projection gradient -- here: against the materialised route, relative to the largest element"""
    c = arm_cfg(cfg, arm)
    x = inputs(c, 1)[0]
    fused, mat = engine(c, BF16, T, score_path="fused"), engine(c, BF16, T, score_path="materialised")
    plain_f, plain_m = engine(c, BF16, score_path="fused"), engine(c, BF16, score_path="materialised")
    res = []
    for e in (fused, mat, plain_f, plain_m):
        e._forward_loss(x, True)
        e.backward()
        res.append((e.result.detach().cpu().clone(), e.d_pred.detach().cpu().double().clone()))
    assert fused.score_mode == "fused" and torch.equal(bits(fused.pred_n), bits(mat.pred_n)) and torch.equal(bits(fused.finf_n), bits(mat.finf_n))
    gap = lambda p, q: float((p[1] - q[1]).abs().max() / q[1].abs().max())   # noqa: E731
    assert abs(float(res[0][0][0]) - float(res[1][0][0])) <= max(2 * abs(float(res[2][0][0]) - float(res[3][0][0])), 2.0 ** -8 * float(res[1][0][0]))
    assert gap(res[0], res[1]) <= max(2 * gap(res[2], res[3]), 2.0 ** -7)
    assert abs(float(res[1][0][0]) - float(res[3][0][0])) > 4 * 2.0 ** -8 * float(res[1][0][0]), "the two scores are too close for this case to tell them apart"


# ---------------------------------------------------------------------- the entry (simulator)
def case_entry(emu, widths, capsys):   # E11
    from dpc_amd import main as dpc_main
    common = ["--net", "resnet18", "--img_dim", "64", "--batch_size", "2", "--gpu", "0", "--print_freq", "1", "--num_seq", "4", "--epochs", "1",
              "--pred_step", "1", "--synthetic", "2"]
    dpc_main.main(common + ["--score_norm", "cosine", "--temperature", "0.1"], _simulator=emu, _widths=widths)
    out = capsys.readouterr().out
    assert out.splitlines().count("Score: cosine, temperature 0.1") == 1 and "Training from ep 0 to ep 1 finished" in out, out
    losses = [float(v) for v in re.findall(r"Loss (\d+\.\d+) \(", out)]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)
    for flags in (["--score_norm", "cosine", "--temperature", "0"], ["--score_norm", "cosine", "--temperature", "-1"],
                  ["--score_norm", "cosine", "--temperature", "nan"], ["--score_norm", "cosine", "--temperature", "inf"], ["--temperature", "0.5"]):
        with pytest.raises(ValueError, match="--temperature"):   # before a rank starts: nothing is printed
            dpc_main.main(common + flags, _simulator=emu, _widths=widths)
        assert capsys.readouterr().out == ""


# ---------------------------------------------------------------------- captured steps, training (HIP device only)
EXTRA_TRAIN, EXTRA_EVAL = 2, 1   # launches per step with the cosine score on: dpc_rownorm_fwd (+ dpc_rownorm_bwd)


def case_captured(cfg: Cfg, arm: str, k_slots: int = 0, accum: int = 1, T=0.1):   # E9
    """a captured step replayed five times against an eager twin, bit for bit; the capture holds the cosine-less capture's launches plus
    two per training step; a replay after set_score_norm changed raises"""
    c = arm_cfg(cfg, arm)
    xs = inputs(c, 6 * accum)
    a, b, plain = engine(c, BF16, T, k_slots), engine(c, BF16, T, k_slots), engine(c, BF16, None, k_slots)
    for e in (a, b, plain):
        if accum > 1:
            e.set_grad_accum(accum)
        for x in xs[:accum]:   # an eager step (cycle) sizes every lazy buffer
            e.train_step(x)
    block = xs[0].clone()
    ref = plain.capture_train_step(block, warmup=0)
    replay = a.capture_train_step(block, warmup=0)
    if accum > 1:
        assert replay.micro.kernels == [ref.micro.kernels[0] + EXTRA_TRAIN] and replay.last.kernels == [ref.last.kernels[0] + EXTRA_TRAIN]
    else:
        assert replay.kernels == [ref.kernels[0] + EXTRA_TRAIN]
    for j, x in enumerate(xs[accum:6 * accum]):
        block.copy_(x)
        ra = replay().clone()
        rb = b.train_step(x).clone()
        assert torch.equal(bits(ra), bits(rb)), j
        assert torch.equal(bits(a.flat_p), bits(b.flat_p)) and (not k_slots or same(nq.ring_state(a), nq.ring_state(b))), j
    assert a.step_count == b.step_count == 6
    if not k_slots and accum == 1:   # the evaluation step: one launch more
        for e in (a, plain):
            e.forward(xs[0], train=False, materialise=False)
            e.loss_topk(with_grad=False)
        ev, ev0 = a.capture_eval_step(), plain.capture_eval_step()
        assert ev.kernels == [ev0.kernels[0] + EXTRA_EVAL]
        b.forward(xs[0], train=False, materialise=False)
        assert torch.equal(bits(ev().clone()), bits(b.loss_topk(with_grad=False)))
    a.set_score_norm("cosine", 2 * T)
    with pytest.raises(RuntimeError):
        replay()
    a.release_captures()
    plain.release_captures()


def case_training(cfg: Cfg, arm: str, T=0.1, steps=30, report=print):   # E12
    c = arm_cfg(cfg, arm)
    eng = engine(c, BF16, T, dropout=0.0)
    x = inputs(c, 1)[0]
    losses = [eng.train_step(x).clone() for _ in range(steps)]
    vals = torch.stack(losses).cpu()
    report(f"[score-norm] training, T {T}: loss {float(vals[0, 0]):.4f} -> {float(vals[-1, 0]):.4f}")
    assert bool(torch.isfinite(vals).all()) and float(vals[-1, 0]) < float(vals[0, 0])
    floor = math.log1p((eng.R - 1) * math.exp(-2.0 / T))   # what a bounded logit leaves of the loss
    assert float(vals[:, 0].min()) >= floor * (1 - 2.0 ** -6)
