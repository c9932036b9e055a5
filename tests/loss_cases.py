"""Case bodies of the loss-family tests, shared by the simulator tier (tests/test_loss_emu.py) and the MI355X tier
(tests/test_loss_gpu.py): the row kernels behind dpc_ce_topk / dpc_ce_topk_bf16 (csrc/loss.hip: ce_row_kernel,
ce_row_vec_kernel<TD,NV,FAST>, ce_row_vec16_kernel<NV>), ce_finalize_kernel on its own (dpc_ce_finalize) and the forward of the fused
score (csrc/score_fused.hip: dpc_score_fwd), held PER ROW.

Data is exact by construction: every logit is a value of both f32 and bf16, every difference x - max and every comparison is exact,
so the strict-greater count is an integer fact and the only rounding left is that of exp / the sums / log.  Row kinds (the target
column of row r is r):

  flat      every logit from {-1/4, 0, 1/4}: every column carries at least e^(-1/2) / cols of the row's mass
  ties      the same grid with a planted rank: n logits at +1/4, the target and many others at 0 (on both sides of the target), the
            rest at -1/4; one row all equal (rank 0); one row with the target as the unique minimum (rank cols - 1)
  sentinel  background and target at -20, J columns at 0, placed where indexing goes wrong (sentinel_positions)
  hot       the same with -100 / +100: without the max subtraction the row is inf / NaN

Bounds carry no tolerance constant.  The loss term of a row is held to the f64 logsumexp - target within a QUARTER (the factor of
kcases.rejects_dropped_row) of what removing one column from the row's sum-exp changes: -log1p(-p_min) on flat / ties rows (the
lightest column), log(J / (J - 1)) on sentinel / hot rows (any sentinel).  An f32 gradient element is held RELATIVE TO ITSELF within a
quarter of the relative change a dropped column makes to every probability of the row: p_min, resp. 1 / J.  A bf16 gradient element is
within 2^-8 of its reference: one bf16 rounding (2^-9 of the next power of two) plus the same again for an f32 value on the other side
of a rounding boundary.  A correctly rounded value just above a power of two comes to 0.996 of that bound (half an ulp of 2^-7 against
1 + 2^-8) and an f32 error ahead of the rounding moves it by 2^-22, so correct code reaches 0.97 here and cannot pass 1.  An element whose reference is below the smallest normal number must itself be below it.  J is 8; a row with fewer than 16 columns
takes J = cols // 2 (cols = 4, 8), the formulas unchanged."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np
import torch

import kcases as kc
from dpc_amd import _lib as L

F32, BF16 = torch.float32, torch.bfloat16
QUARTER = 0.25                       # kcases.rejects_dropped_row's factor
TINY = float(np.finfo(np.float32).tiny)   # smallest normal f32; bf16 has the same exponent range
GUARD = 64                           # poisoned elements behind the last row of an output

# (cols, ld, ld_d, score offset in elements) of dpc_ce_topk; 0 = tight.  The form is what the dispatcher of loss.hip selects
# (dpc_last_kernel names the finalize launch after these entries, so the form is argued from the dispatch conditions).
CE_SHAPES = {
    # ce_row_kernel, the three-sweep form
    "sweep_37": (37, 0, 0, 0),                   # cols % 4 != 0
    "sweep_1030": (1030, 0, 0, 0),               # cols % 4 != 0, five trips of 256, the last one ragged
    "sweep_16388": (16388, 0, 0, 0),             # past the register cap of 16 384 columns
    "sweep_1024_ld1025": (1024, 1025, 0, 0),     # ld % 4 != 0
    "sweep_1024_off4": (1024, 0, 0, 1),          # score pointer 4 bytes off a 16-byte boundary
    "sweep_1024_ldd1026": (1024, 0, 1026, 0),    # ld_d % 4 != 0 (with a gradient; without one this is the NV = 8 form)
    # ce_row_vec_kernel<., 8, .>
    "nv8_4": (4, 0, 0, 0),                       # one 16-byte unit, 255 idle threads
    "nv8_1024": (1024, 0, 0, 0),                 # exactly one register trip
    "nv8_1028": (1028, 0, 0, 0),                 # one unit into the second trip
    "nv8_8192": (8192, 0, 0, 0),                 # all 8 trips full
    "nv8_1028_ld1040_ldd1048": (1028, 1040, 1048, 0),
    "nv8_square_40": (40, 0, 0, 0),              # rows == cols == 40, all four row kinds
    # ce_row_vec_kernel<., 16, .>
    "nv16_8196": (8196, 0, 0, 0),                # one unit past NV = 8
    "nv16_16384": (16384, 0, 0, 0),              # all 16 trips full
}
# dpc_ce_topk_bf16: ce_row_vec16_kernel<4> up to 8 192 columns, <8> beyond
CE16_SHAPES = {
    "vec16x4_8": (8, 0, 0, 0),
    "vec16x4_2048": (2048, 0, 0, 0),             # exactly one register trip
    "vec16x4_2056": (2056, 0, 0, 0),             # one unit into the second trip
    "vec16x4_8192": (8192, 0, 0, 0),             # vec16<4> full
    "vec16x8_8200": (8200, 0, 0, 0),             # one unit past vec16<4>
    "vec16x8_16384": (16384, 0, 0, 0),           # vec16<8> full
    "vec16x4_2056_ld2064_ldd2072": (2056, 2064, 2072, 0),
}
FINALIZE_ROWS = (1, 255, 256, 257, 1000)
SCORE_SHAPES = ((24, 32), (200, 32), (264, 32), (136, 256), (520, 32))   # (520, 32): two column splits, last tile 8 columns, last row block 8 rows
SCORE_SHAPES_GPU = SCORE_SHAPES + ((1100, 256),)                          # four splits, the last one short

RowCase = namedtuple("RowCase", "s kinds J rank term loss_bound grad grad_bound covered positions")


def sentinel_positions(cols, U):
    """columns where a row kernel's indexing goes wrong, for U logits per 16-byte unit: the ends, the last full unit and the element
    behind it, the wave seams of the first trip, and both sides of every trip start"""
    P = [0, cols - 1]
    nfull = cols // U
    if nfull:
        P += [U * (nfull - 1), U * nfull - 1, U * nfull]
    for w in (1, 2, 3):
        P += [U * 64 * w - 1, U * 64 * w + 1]
    i = 1
    while U * 256 * i < cols:
        P += [U * 256 * i - 1, U * 256 * i, U * 256 * i + 1]
        i += 1
    out = []
    for p in P:
        if 0 <= p < cols and p not in out:
            out.append(p)
    return out


def _t(a):
    return torch.from_numpy(np.array(a))   # a copy: the shared expectations are read-only


def _take(cands, J, r, cols):
    got = []
    for c in cands:
        if 0 <= c < cols and c != r and c not in got:
            got.append(c)
            if len(got) == J:
                break
    return got


@functools.lru_cache(maxsize=None)
def row_case(cols, U, square=False):
    """the planted matrix of a shape and its f64 expectations; computed once, shared by every case of the shape, never written to"""
    rng = np.random.Generator(np.random.PCG64(1000 + cols))
    J = min(8, cols // 2)
    P = sentinel_positions(cols, U)
    pending = list(P)
    todo = {"flat": 6, "hot": 3, "ties": [0, 1, 2, 3, 4, 5, 6, "equal", "min"]}
    grid = np.array([-0.25, 0.0, 0.25])
    srows, kinds, planted = [], [], {}
    while len(srows) < cols and (pending or todo["flat"] or todo["hot"] or todo["ties"]):
        for kind in ("flat", "sentinel", "hot", "ties"):
            r = len(srows)
            if r >= cols:
                break
            if kind == "flat" and todo["flat"]:
                todo["flat"] -= 1
                v = grid[rng.integers(0, 3, cols)]
            elif kind == "sentinel" and pending:
                cs = _take([r - 1, r + 1] + pending + P + list(range(cols)), J, r, cols)
                pending = [p for p in pending if p not in cs]
                v = np.full(cols, -20.0)
                v[cs] = 0.0
            elif kind == "hot" and todo["hot"]:
                todo["hot"] -= 1
                rot = (5 * todo["hot"]) % len(P)
                cs = _take([r - 1, r + 1] + P[rot:] + P[:rot] + list(range(cols)), J, r, cols)
                v = np.full(cols, -100.0)
                v[cs] = 100.0
            elif kind == "ties" and todo["ties"]:
                n = todo["ties"].pop(0)
                others = rng.permutation([c for c in range(cols) if c != r])
                if n == "equal":
                    v = np.zeros(cols)
                    planted[r] = 0
                elif n == "min":
                    v = grid[rng.integers(1, 3, cols)]
                    v[r] = -0.25
                    planted[r] = cols - 1
                else:
                    n = min(n, (cols - 1) // 2)
                    above = others[:n]
                    v = np.full(cols, -0.25)
                    v[others[n:n + max(1, (cols - 1 - n) // 3)]] = 0.0
                    for c in (r - 1, r + 1):          # ties on both sides of the target
                        if 0 <= c < cols:
                            v[c] = 0.0
                    v[above] = 0.25
                    v[r] = 0.0
                    planted[r] = n
            else:
                continue
            srows.append(v)
            kinds.append(kind)
    while square and len(srows) < cols:
        srows.append(grid[rng.integers(0, 3, cols)])
        kinds.append("flat")
    s = np.stack(srows)
    rows = s.shape[0]
    assert rows <= cols and (not square or rows == cols)
    idx = np.arange(rows)
    tgt = s[idx, idx]
    rank = (s > tgt[:, None]).sum(1)
    for r, n in planted.items():
        assert rank[r] == n, (r, n, rank[r])
    mx = s.max(1)
    e = np.exp(s - mx[:, None])
    se = e.sum(1)
    term = np.log(se) + mx - tgt
    p = e / se[:, None]
    onehot = np.zeros_like(p)
    onehot[idx, idx] = 1.0
    grad = (p - onehot) / rows
    jrow = np.array([kd in ("sentinel", "hot") for kd in kinds])
    pmin = p.min(1)
    if J > 1:
        loss_bound = QUARTER * np.where(jrow, np.log(J / (J - 1.0)), -np.log1p(-pmin))
    else:
        loss_bound = QUARTER * -np.log1p(-pmin)
    grad_bound = QUARTER * np.where(jrow, 1.0 / J, pmin)
    covered = not pending
    for a in (s, rank, term, loss_bound, grad, grad_bound):
        a.setflags(write=False)
    return RowCase(s, tuple(kinds), J, rank, term, loss_bound, grad, grad_bound, covered, tuple(P))


def data_is_exact_case(cols, U):
    """on the reference alone: the logits are bf16 values, x - max is exact in bf16's 8 bits, every listed position is a sentinel
    of some row (where the rows are not cut short by cols), every kind is present"""
    rc = row_case(cols, U)
    t = _t(rc.s)
    assert torch.equal(t.to(BF16).double(), t)
    d = _t(rc.s - rc.s.max(1)[:, None])
    assert torch.equal(d.to(BF16).double(), d)
    if cols >= 64:
        assert rc.covered and set(rc.kinds) == {"flat", "sentinel", "hot", "ties"} and 16 <= rc.s.shape[0] <= 40 < cols
        sent = set()
        for r, kd in enumerate(rc.kinds):
            if kd == "sentinel":
                sent |= set(np.nonzero(rc.s[r] == 0.0)[0].tolist())
        assert set(rc.positions) <= sent


def _strided(k, host, ld, dtype, off=0):
    """[rows, cols] -> a device buffer with leading dimension ld that starts `off` elements behind an aligned address; whatever lies
    between the rows is NaN, so a kernel that read it shows in every sum"""
    rows, cols = host.shape
    buf = torch.full((off + rows * ld,), float("nan"), dtype=dtype)
    buf[off:].view(rows, ld)[:, :cols] = _t(host).to(dtype)
    dev = buf.to(k.dev)
    view = dev[off:]
    assert dev.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (off * dev.element_size()) % 16
    return dev, view


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu()


class Out:
    """the outputs of one call: row_ws and result poisoned, dscore (or None) poisoned with a guard band behind its last row"""

    def __init__(self, k, rows, ld_d, gdt):
        self.ws, self.res = k.poison(rows, 2), k.poison(4)
        self.gdt, self.rows, self.ld_d = gdt, rows, ld_d
        self.dbuf = None if gdt is None else k.poison(rows * ld_d + GUARD, dtype=gdt)
        self.before = None if gdt is None else _bits(self.dbuf)

    @property
    def d(self):
        return None if self.dbuf is None else self.dbuf[:self.rows * self.ld_d].view(self.rows, self.ld_d)

    def guard_untouched(self):
        if self.dbuf is not None:
            n = self.rows * self.ld_d
            assert torch.equal(_bits(self.dbuf)[n:], self.before[n:]), "the guard band behind dscore was written"

    def untouched(self):
        """after a rejected call"""
        assert bool(torch.isnan(self.ws).all()) and bool(torch.isnan(self.res).all())
        if self.dbuf is not None:
            assert torch.equal(_bits(self.dbuf), self.before)


def _launch(k, entry, sview, rows, cols, ld, out, dtype_code):
    if entry == "dpc_ce_topk":
        k.call(entry, sview, rows, cols, ld, out.ws, out.res, out.d, dtype_code, out.ld_d)
    else:
        k.call(entry, sview, rows, cols, ld, out.ws, out.res, out.d, out.ld_d)
    k.sync()


def check_rows(name, rc, cols, ws, res):
    """rank, loss term, result: every row"""
    rows = rc.s.shape[0]
    kc.all_finite(ws, res)
    w = ws.cpu().numpy().astype(np.float64)
    assert np.array_equal(w[:, 1], rc.rank.astype(np.float64)), f"{name}: rank differs on rows {np.nonzero(w[:, 1] != rc.rank)[0][:8].tolist()}"
    e = np.abs(w[:, 0] - rc.term)
    worst = int(np.argmax(e / rc.loss_bound))
    print(f"[loss-row] {name}: rows {rows} cols {cols} e_ok {e[worst]:.3g} bound {rc.loss_bound[worst]:.3g} "
          f"(row {worst}, {rc.kinds[worst]}; ratio {e[worst] / rc.loss_bound[worst]:.3g})")
    bad = np.nonzero(~(e < rc.loss_bound))[0]
    assert bad.size == 0, f"{name}: loss term of rows {bad[:8].tolist()} off by {e[bad[:8]].tolist()}, a quarter of a dropped column is {rc.loss_bound[bad[:8]].tolist()}"
    r = res.cpu().numpy()
    for i, kk in enumerate((1, 3, 5)):
        want = np.float32(int((rc.rank < kk).sum())) / np.float32(rows)
        assert r[1 + i] == want, f"{name}: top-{kk} {r[1 + i]!r}, exactly {want!r}"
    assert abs(float(r[0]) - rc.term.mean()) < rc.loss_bound.max(), f"{name}: mean loss {r[0]} against {rc.term.mean()}"
    return e[worst] / rc.loss_bound[worst]


def check_grad(name, rc, cols, d, gdt):
    """d(loss)/d(score), element by element, relative to the element; the padding columns are zero"""
    g = d[:, :cols].float().cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all(), f"{name}: {int((~np.isfinite(g)).sum())} gradient elements are not finite (left unwritten?)"
    ref = rc.grad
    tiny = np.abs(ref) < TINY
    assert (np.abs(g[tiny]) < TINY).all(), f"{name}: an element whose reference underflows is not below the smallest normal number"
    rel = np.abs(g - ref) / np.where(tiny, 1.0, np.abs(ref))
    rel[tiny] = 0.0
    bound = rc.grad_bound if gdt == F32 else np.full(rc.s.shape[0], 2.0 ** -8)
    ratio = rel.max(1) / bound
    worst = int(np.argmax(ratio))
    print(f"[loss-grad] {name} {'f32' if gdt == F32 else 'bf16'}: rows {rc.s.shape[0]} cols {cols} e_ok {rel[worst].max():.3g} bound {bound[worst]:.3g} "
          f"(row {worst}, {rc.kinds[worst]}, column {int(np.argmax(rel[worst]))}; ratio {ratio[worst]:.3g})")
    bad = np.nonzero(~(rel.max(1) < bound))[0]
    assert bad.size == 0, f"{name}: gradient rows {bad[:8].tolist()} off by {rel.max(1)[bad[:8]].tolist()} of the element, bound {bound[bad[:8]].tolist()}"
    if d.shape[1] > cols:
        assert float(d[:, cols:].float().abs().max()) == 0.0, f"{name}: dscore[:, cols:ld_d] is not zero"
    return ratio[worst]


def ce_rows_case(k, entry, name, mode):
    """one shape of CE_SHAPES / CE16_SHAPES under one gradient mode.  dpc_ce_topk: "f32" (and the same call without a gradient, bit for
    bit), "bf16", "bf16-null" (dtype_d = bf16, dscore = NULL).  dpc_ce_topk_bf16: "bf16", "null"."""
    bf_logits = entry == "dpc_ce_topk_bf16"
    cols, ld, ld_d, off = (CE16_SHAPES if bf_logits else CE_SHAPES)[name]
    rc = row_case(cols, 8 if bf_logits else 4, square="square" in name)
    rows = rc.s.shape[0]
    ld, ld_d = ld or cols, ld_d or cols
    keep, sview = _strided(k, rc.s, ld, BF16 if bf_logits else F32, off)
    gdt = {"f32": F32, "bf16": BF16}.get(mode)
    code = L.dtype_code(F32 if mode == "f32" else BF16)
    out = Out(k, rows, ld_d, gdt)
    _launch(k, entry, sview, rows, cols, ld, out, code)
    tag = f"{entry} {name} {mode}"
    ratios = {"loss": check_rows(tag, rc, cols, out.ws, out.res)}
    if gdt is not None:
        ratios["grad"] = check_grad(tag, rc, cols, out.d, gdt)
        out.guard_untouched()
    if mode == "f32":       # both calls run the FAST = false instantiation of one form: without a gradient the same bits
        null = Out(k, rows, ld_d, None)
        if "ldd1026" in name:   # ... except where only the gradient's layout demotes the form: held on its own
            _launch(k, entry, sview, rows, cols, ld, null, code)
            check_rows(tag + " (no gradient)", rc, cols, null.ws, null.res)
        else:
            _launch(k, entry, sview, rows, cols, ld, null, code)
            assert torch.equal(_bits(null.ws), _bits(out.ws)) and torch.equal(_bits(null.res), _bits(out.res)), f"{tag}: other bits without a gradient"
    del keep
    return ratios


def ce_rejects_case(k):
    """argument errors and unsupported layouts launch nothing: the poisoned outputs stay as they were"""
    import pytest
    arg, uns = f"code {L.ERR_ARG}$", f"code {L.ERR_UNSUPPORTED}$"
    s32 = k.zeros(8 * 64)               # real inputs of calls that must not read them
    for rows, cols, ld, ld_d, code in ((8, 4, 4, 8, L.dtype_code(F32)),       # cols < rows
                                       (8, 16, 12, 16, L.dtype_code(F32)),    # ld < cols
                                       (8, 16, 16, 12, L.dtype_code(BF16)),   # ld_d < cols
                                       (8, 16, 16, 16, 77)):                  # unknown dtype_d
        out = Out(k, 8, 16, F32)
        with pytest.raises(L.DpcError, match=arg):
            k.call("dpc_ce_topk", s32, rows, cols, ld, out.ws, out.res, out.d, code, ld_d)
        k.sync()
        out.untouched()
    s16 = k.zeros(8 * 16400 + 8, dtype=BF16)
    for cols, ld, ld_d, soff, doff in ((16392, 16392, 16392, 0, 0),   # past the register cap of vec16<8>
                                       (36, 40, 40, 0, 0),            # cols % 8 != 0
                                       (40, 44, 48, 0, 0),            # ld % 8 != 0
                                       (40, 40, 40, 4, 0),            # score pointer 8 bytes off
                                       (40, 40, 40, 0, 4)):           # dscore pointer 8 bytes off
        out = Out(k, 8, max(ld_d, 48), BF16)
        d = out.dbuf[doff:]
        with pytest.raises(L.DpcError, match=uns):
            k.call("dpc_ce_topk_bf16", s16[soff:], 8, cols, ld, out.ws, out.res, d, ld_d)
        k.sync()
        out.untouched()
    out = Out(k, 8, 48, BF16)
    with pytest.raises(L.DpcError, match=arg):                        # argument errors come first
        k.call("dpc_ce_topk_bf16", s16, 8, 4, 8, out.ws, out.res, out.d, 8)
    k.sync()
    out.untouched()


# ---- dpc_ce_finalize on a row_ws built by hand -------------------------------------------------------------------------------------
def ce_finalize_case(k, rows):
    """ranks cycle through 0 ... 6 (0 | 1, 2 | 3 and 4 | 5 straddle the three thresholds); loss terms are multiples of 2^-10 below 16,
    so every f32 partial sum is exact in any order and the four results are the correctly rounded quotients"""
    rng = np.random.Generator(np.random.PCG64(rows))
    w = np.zeros((rows, 2), np.float32)
    w[:, 0] = rng.integers(0, 16 * 1024, rows) / 1024.0
    w[:, 1] = np.arange(rows) % 7
    total = float(w[:, 0].astype(np.float64).sum())
    assert np.float32(total) == total
    res = k.poison(4)
    k.call("dpc_ce_finalize", k.t(torch.from_numpy(w)), rows, res)
    k.sync()
    kc.all_finite(res)
    want = [np.float32(total) / np.float32(rows)] + [np.float32(int((w[:, 1] < kk).sum())) / np.float32(rows) for kk in (1, 3, 5)]
    assert res.cpu().numpy().tolist() == [float(v) for v in want], f"rows {rows}: {res.cpu().numpy().tolist()} against {want}"


# ---- fused score forward on exact operands -----------------------------------------------------------------------------------------
ScoreData = namedtuple("ScoreData", "pred finf S rank lse term bound planted pairs zero")


@functools.lru_cache(maxsize=None)
def score_data(R, D):
    """pred / finf with entries in {0, +-1/2}, at most four non-zeros in a pred row: every S[i][j] is a multiple of 1/4 in [-1, 1],
    exact under any accumulation order.  Planted: rows of rank 0 ... 6 (pred = p_n on four features of its own, the target at 3/4, and
    n columns whose finf holds p_n itself: 1), two pairs of identical finf rows (a tie at the target, value 1/2) and an all-zero pred
    row (everything ties)."""
    rng = np.random.Generator(np.random.PCG64(7 * R + D))

    def sparse(n):
        m = np.zeros((n, D))
        for i in range(n):
            nn = int(rng.integers(1, 5))
            m[i, rng.choice(D, nn, replace=False)] = rng.choice([-0.5, 0.5], nn)
        return m
    pred, finf = sparse(R), sparse(R)
    sp = []
    for c in [0, R - 1, 63, 64, 127, 128, R - 8, R - 9] + rng.permutation(R).tolist():   # the ends, tile seams, the short last block
        if 0 <= c < R and c not in sp:
            sp.append(c)
    planted, copies, pairs, zero = sp[0:7], sp[7:13], ((sp[13], sp[14]), (sp[15], sp[16])), sp[17]
    supp = rng.permutation(D)[:28].reshape(7, 4)
    p = np.zeros((7, D))
    for n in range(7):
        p[n, supp[n]] = rng.choice([-0.5, 0.5], 4)
        pred[planted[n]] = p[n]
        finf[planted[n]] = p[n]
        finf[planted[n], supp[n][3]] = 0.0
    for kk in range(1, 7):
        finf[copies[kk - 1]] = p[kk:].sum(0)
    for a, b in pairs:
        f = np.zeros(D)
        f[rng.choice(D, 2, replace=False)] = rng.choice([-0.5, 0.5], 2)
        finf[a] = finf[b] = pred[a] = f
    pred[zero] = 0.0
    S = pred @ finf.T
    assert np.abs(S).max() <= 1.0 and np.array_equal(S * 4, np.round(S * 4))
    dg = np.diagonal(S)
    rank = (S > dg[:, None]).sum(1)
    for n in range(7):
        assert rank[planted[n]] == n, (n, rank[planted[n]])
    for a, b in pairs:
        assert S[a, a] == S[a, b] == 0.5
    assert rank[zero] == 0
    mx = S.max(1)
    e = np.exp(S - mx[:, None])
    lse = np.log(e.sum(1)) + mx
    pmin = (e / e.sum(1)[:, None]).min(1)
    bound = QUARTER * -np.log1p(-pmin)
    for a in (pred, finf, S, rank, lse, bound):
        a.setflags(write=False)
    return ScoreData(pred, finf, S, rank, lse, lse - dg, bound, tuple(planted), pairs, zero)


def score_fwd_case(k, R, D):
    sd = score_data(R, D)
    pk, fk = k.t(_t(sd.pred), BF16), k.t(_t(sd.finf), BF16)
    nf, nb = C.c_int64(0), C.c_int64(0)
    assert k.lib.call("dpc_score_ws_floats", R, D, C.byref(nf), C.byref(nb)) >= 1
    runs = []
    for with_score in (True, False):
        ws = k.poison(nf.value + GUARD)
        diag, lse2, row_ws, res = k.poison(R), k.poison(R), k.poison(R, 2), k.poison(4)
        score = k.poison(R * R + GUARD) if with_score else None
        k.call("dpc_score_fwd", pk, fk, R, D, diag, lse2, row_ws, score, ws)
        k.call("dpc_ce_finalize", row_ws, R, res)
        k.sync()
        kc.all_finite(ws[:nf.value], diag, lse2, row_ws, res)
        assert bool(torch.isnan(ws[nf.value:]).all()), "the workspace was written past dpc_score_ws_floats"
        if with_score:
            assert bool(torch.isnan(score[R * R:]).all())
            assert np.array_equal(score[:R * R].view(R, R).cpu().numpy().astype(np.float64), sd.S), "score != S on exact operands"
        runs.append((diag, lse2, row_ws, res))
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert torch.equal(_bits(a), _bits(b)), "score = NULL changes diag / lse2 / row_ws bits"
    diag, lse2, row_ws, res = runs[0]
    assert np.array_equal(diag.cpu().numpy().astype(np.float64), np.diagonal(sd.S))
    w = row_ws.cpu().numpy().astype(np.float64)
    assert np.array_equal(w[:, 1], sd.rank.astype(np.float64)), f"rank differs on rows {np.nonzero(w[:, 1] != sd.rank)[0][:8].tolist()}"
    r = res.cpu().numpy()
    for i, kk in enumerate((1, 3, 5)):
        assert r[1 + i] == np.float32(int((sd.rank < kk).sum())) / np.float32(R)
    e = np.abs(w[:, 0] - sd.term)
    worst = int(np.argmax(e / sd.bound))
    print(f"[loss-row] dpc_score_fwd ({R}, {D}): rows {R} cols {R} e_ok {e[worst]:.3g} bound {sd.bound[worst]:.3g} (row {worst}; ratio {e[worst] / sd.bound[worst]:.3g})")
    assert (e < sd.bound).all(), f"loss term of rows {np.nonzero(~(e < sd.bound))[0][:8].tolist()}"
    assert abs(float(r[0]) - sd.term.mean()) < sd.bound.max()
    L2E = 1.4426950408889634
    want2 = (sd.lse + np.log(float(R))) * L2E
    e2 = np.abs(lse2.cpu().numpy().astype(np.float64) - want2)
    b2 = sd.bound * L2E + np.spacing(want2.astype(np.float32)).astype(np.float64)
    assert (e2 < b2).all(), f"lse2 of rows {np.nonzero(~(e2 < b2))[0][:8].tolist()}: {e2.max():.3g}"
    return e[worst] / sd.bound[worst]
