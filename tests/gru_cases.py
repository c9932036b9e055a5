"""The fused ConvGRU recurrence (csrc/gru_chain.hip: dpc_gru_pack, dpc_gru_chain_fwd / _bwd) held step by step, one rounding per element.
Shared by the host-simulator tier (tests/test_gru_emu.py) and the MI355X tier (tests/test_gru_gpu.py).

The errors of the recurrence compound; the errors of ONE step given its stored inputs do not.  After forward + backward every saved
tensor comes back and each value is recomputed in f64 from the KERNEL'S OWN stored operands (Chain.evaluate): weights quantised to the
compute dtype as dpc_gru_pack does, biases f32, the dropout masks explicit, drawn by kcases.dropout_mask_np for the kernel's
(seed, step), or ones (eval).  Only the backward's carried dh is the reference's own (f64); its f32 error budget is carried beside it.

Bounds, per element (U24 = 2^-24, r = 2^-8 in bf16 and 0 in f32), no tolerance constant but GATE_F32_MEASURED:
  * exact facts (torch.equal): HR_all = rounding of the one f32 product h * r of the stored operands; X_all[n_agg + i] = relu(pred[i]);
    inputs, guard bands and rows >= M untouched.
  * stored in the compute dtype (H_all, P1_all, pred, G_all, dP1, dP2):  |got - v| <= r |v| + slack (1 + r).
  * stored in f32: d_x, the final dh (ws[0]) and the last dx that fed a prediction (ws[1]): slack alone; the gates U, R, O: slack x Lipschitz constant (1/4 sigmoid, 1 tanh)
    + 8 x GATE_F32_MEASURED.
  * slack of a product: (n + 2) U24 (sum_k |a_k||b_k| + |bias|), n = K for the bf16 MFMA (exact products, f32 accumulation), 2K for
    v_mfma_f32_32x32x2_f32, pushed through the element-wise factor behind it; slack of an element-wise expression: its count of f32
    operations (named beside each expression in Chain.evaluate, counted from gru_chain.hip) x U24 x the product of the sums of the
    magnitudes of its terms.  Both are worst cases over any summation order.
Teeth (Chain.teeth), proven on a CPU model of the chain (evaluate() with no kernel data: every storage point rounded) before a kernel
result is looked at: for every tensor a product feeds, blocks of 32 x 32 outputs (last ragged row tile x last column tile, first x
first) are recomputed with one reduction position left out -- one MFMA K-step (16 indices bf16, 8 f32) for compute-dtype tensors, one
single index for f32-stored ones; first, last and two inner positions of every operand half; some element must move by more than
4 x its bound."""
import ctypes as C
import functools
from collections import namedtuple

import torch

import kcases as kc
from dpc_amd import _lib as L

F32, BF16 = torch.float32, torch.bfloat16
U24 = 2.0 ** -24
TILE = 32
P_DROP, SEED = 0.1, 233

# Largest |got - ref| of an element of U_all / R_all / O_all against the step-pinned f64 reference over every case of the MI355X tier
# (tests/test_gru_gpu.py): 1.19e-6, an element of O_all in f32 at 640 rows x D = 256 (the tanh of a 512-term f32 MFMA chain; U and R stay
# below 4.5e-7, every bf16 case below 4.3e-7); the simulator tier (std::exp, a true division) reaches 9.6e-7 at the engine's shape.
# The only measured constant of this module: the error of __expf / __frcp_rn is in no specification the project has.  It enters the
# gate bound 8-fold (DX_F32_BOUND's margin: another expansion of exp / rcp on another driver, not a bug).
GATE_F32_MEASURED = 1.2e-6

Case = namedtuple("Case", "B SQ D P n_agg drop h0 hlast step seed", defaults=("masks", False, False, 0, 5))

CASES = {
    # every gemm_acc regime and every 2 / 1 / 0-tiles-per-wave mix; M = 36 or 18: a ragged last (or only) row tile
    "d32": Case(3, 12, 32, 2, 2), "d64": Case(2, 9, 64, 2, 2), "d96": Case(3, 12, 96, 2, 2), "d160": Case(2, 9, 160, 2, 2),
    "d224": Case(3, 12, 224, 2, 2), "d256": Case(2, 9, 256, 2, 2),
    "p1": Case(2, 9, 64, 1, 2),                                  # no prediction feeds a step
    "lc": Case(2, 9, 64, 0, 8, hlast=True),                      # LC form: P = 0, the backward seeded by d_hlast alone
    "lc_h0": Case(2, 9, 64, 0, 8, h0=True, hlast=True),
    "p3_hlast": Case(2, 5, 32, 3, 2, hlast=True),                # d_hlast on top of d_pred
    "nagg1": Case(3, 12, 64, 2, 1),
    "sq1": Case(37, 1, 64, 2, 2), "sq49": Case(2, 49, 64, 2, 2),  # 98 rows: both clips straddle row tiles
    "philox_d32": Case(3, 12, 32, 2, 2, drop="philox", step=3), "philox_d256": Case(2, 9, 256, 2, 2, drop="philox", step=7),
    "eval": Case(3, 12, 64, 2, 2, drop="none"),
}
ENGINE = Case(3, 16, 256, 3, 5)      # the engine's shape: 7 steps, one full and one ragged row tile (both wave counts)


def rows640(D):
    return Case(40, 16, D, 3, 5)     # 20 workgroups


FED = ("U_all", "R_all", "O_all", "P1_all", "pred", "G_r", "dP1", "d_x")     # tensors a product feeds (teeth)
KIND = {"X_all": "exact", "H_all": "T", "HR_all": "exact", "U_all": "gate", "R_all": "gate", "O_all": "gate", "P1_all": "T", "pred": "T",
        "G_u": "T", "G_r": "T", "G_o": "T", "dP1": "T", "dP2": "T", "d_x": "f32", "dh0": "f32", "dxn": "f32"}
WORST = {}       # (tier, tensor) -> largest error / bound seen in this process
GATE_SEEN = {}   # tier -> largest |got - ref| of a gate element


class Held:
    """reference, per-element bound and (product-fed tensors) the recipe of every slab of one saved tensor"""

    def __init__(self, shape):
        self.ref = torch.full(shape, float("nan"), dtype=torch.float64)
        self.bound = torch.zeros(shape, dtype=torch.float64)
        self.rec = {}


Recipe = namedtuple("Recipe", "parts pre post")   # parts [(A [M][K], W [N][K])], pre [M][N], post(pre block, rows, cols) -> values
Mut = namedtuple("Mut", "name idx rows cols part ks")


def dropped(rec, m):
    """the recipe's values on block (m.rows, m.cols) with reduction indices m.ks of operand half m.part left out"""
    A, W = rec.parts[m.part]
    pre = rec.pre[m.rows, m.cols] - A[m.rows, m.ks] @ W[m.cols, m.ks].t()
    return rec.post(pre, m.rows, m.cols)


class Chain:
    def __init__(self, c: Case, dtype, rows=None):
        """rows: run only these rows of the case's data, in this order (SQ = 1 cases: rows are independent sequences)"""
        self.c, self.dtype = c, dtype
        B, SQ, D, P, n_agg = c.B, c.SQ, c.D, c.P, c.n_agg
        g = torch.Generator().manual_seed(c.seed)
        M, ns = B * SQ, n_agg + max(P, 1) - 1
        # NOT quantised: dpc_gru_pack rounds them, the reference rounds them the same way (torch's f32 -> bf16 is to nearest even)
        self.w = {n: torch.randn(D, 2 * D, generator=g) * (1.0 / (2 * D) ** 0.5) for n in ("update", "reset", "out")}
        self.w["p0"] = torch.randn(D, D, generator=g) * (1.0 / D ** 0.5)
        self.w["p2"] = torch.randn(D, D, generator=g) * (1.0 / D ** 0.5)
        self.b = {n: torch.randn(D, generator=g) * 0.1 for n in ("update", "reset", "out", "p0", "p2")}
        self.x = kc.q(torch.relu(torch.randn(n_agg, M, D, generator=g)), dtype)
        self.d_pred = torch.randn(B, max(P, 1), SQ, D, generator=g) * 0.1
        self.d_hlast = torch.randn(M, D, generator=g) * 0.1
        self.h0 = kc.q(torch.randn(M, D, generator=g) * 0.5, dtype) if c.h0 else torch.zeros(M, D)
        if c.drop == "masks":
            self.masks = (torch.rand(ns, M, D, generator=g) > P_DROP).float() / (1 - P_DROP)
        elif c.drop == "philox":   # the definition, not dpc_dropout_mask: element (s, m, col) is word idx % 4 of Philox block idx / 4
            self.masks = torch.from_numpy(kc.dropout_mask_np(ns * M * D, P_DROP, SEED, c.step).reshape(ns, M, D))
        else:
            self.masks = torch.ones(ns, M, D)
        if rows is not None:
            assert SQ == 1 and P == 0
            rows = torch.as_tensor(rows)
            self.x, self.d_hlast, self.h0, self.masks = self.x[:, rows], self.d_hlast[rows], self.h0[rows], self.masks[:, rows]
            B = M = len(rows)
        self.B, self.M, self.ns = B, M, ns
        self.r = 2.0 ** -8 if dtype == BF16 else 0.0
        self.kstep = 16 if dtype == BF16 else 8          # reduction indices of one MFMA K-step (two 16-byte units)
        wq = {n: v.to(dtype).double() for n, v in self.w.items()}
        self.Wx = {n: wq[n][:, :D].contiguous() for n in ("update", "reset", "out")}
        self.Wh = {n: wq[n][:, D:].contiguous() for n in ("update", "reset", "out")}
        self.W1, self.W2 = wq["p0"], wq["p2"]
        self.bd = {n: v.double() for n, v in self.b.items()}
        # rows m = (b, sq) of [B][P][SQ][D]
        self.d_pred_rows = self.d_pred.double().permute(1, 0, 2, 3).reshape(max(P, 1), -1, D)[:, :M]

    # ---- arithmetic model -------------------------------------------------------------------------------------------------------
    def rnd(self, v, kind):
        v = v.float()
        return (v if kind in ("gate", "f32") else v.to(self.dtype).float()).double()

    def gemm(self, parts, bias=None):
        """value, slack and recipe of sum_j A_j @ W_j^T + bias accumulated in f32: (n + 2) U24 (sum |a||b| + |bias|)"""
        pre = sum(A @ W.t() for A, W in parts)
        mag = sum(A.abs() @ W.abs().t() for A, W in parts)
        K = sum(A.shape[1] for A, _ in parts)
        if bias is not None:
            pre, mag = pre + bias, mag + bias.abs()
        n = K if self.dtype == BF16 else 2 * K
        return pre, (n + 2) * U24 * mag, (parts, pre)

    def bT(self, v, slack):
        return self.r * v.abs() + slack * (1 + self.r)

    @staticmethod
    def bgate(slack, lip):
        return slack * lip + 8 * GATE_F32_MEASURED

    def evaluate(self, S=None, mut=None, backward=True):
        """S: the kernel's saved tensors (f64, keys of KIND without dh0 / dxn, which come from ws) -> {name: Held} recomputed slab by slab from them.
        S = None: the CPU model of the chain -- every value rounded where the kernel stores it and read back from there, optionally
        with one mutation (Mut) applied at its storage point; returns (Q, S)."""
        c, D, M, ns, P, n_agg = self.c, self.c.D, self.M, self.ns, self.c.P, self.c.n_agg
        model = S is None
        if model:
            S = {n: torch.zeros(ns, M, D, dtype=torch.float64) for n in ("X_all", "HR_all", "U_all", "R_all", "O_all", "G_u", "G_r", "G_o")}
            S["H_all"] = torch.zeros(ns + 1, M, D, dtype=torch.float64)
            S["X_all"][:n_agg], S["H_all"][0] = self.x.double(), self.h0.double()
            for n in ("P1_all", "pred", "dP1", "dP2"):
                S[n] = torch.zeros(P, M, D, dtype=torch.float64)
            S["d_x"] = torch.zeros(n_agg, M, D, dtype=torch.float64)
        Q = {n: Held(S[n].shape) for n in S}
        Q["dh0"], Q["dxn"] = Held((1, M, D)), Held((1, M, D))     # what the backward leaves in ws[0] (d loss / d h_0) and ws[1]
        k = self.masks.double()

        def put(name, idx, ref, bound=None, rec=None):
            if rec is not None:
                rec = Recipe(rec[0][0], rec[0][1], rec[1])
                Q[name].rec[idx] = rec
            if model and mut is not None and (mut.name, mut.idx) == (name, idx):
                ref = ref.clone()
                ref[mut.rows, mut.cols] = dropped(rec, mut)
            Q[name].ref[idx] = ref
            if bound is not None:
                Q[name].bound[idx] = bound
            if model and name in S:
                S[name][idx] = self.rnd(ref, KIND[name])

        ident = lambda p, r, c_: p
        # ---------------- forward
        for s in range(ns):
            x, h = S["X_all"][s], S["H_all"][s]
            for name, gname in (("U_all", "update"), ("R_all", "reset")):
                pre, sl, rec = self.gemm([(x, self.Wx[gname]), (h, self.Wh[gname])], self.bd[gname])
                put(name, s, torch.sigmoid(pre), self.bgate(sl, 0.25), (rec, lambda p, r, c_: torch.sigmoid(p)))
            put("HR_all", s, (h.float() * S["R_all"][s].float()).to(self.dtype).double())    # ONE f32 product, rounded once
            pre, sl, rec = self.gemm([(x, self.Wx["out"]), (S["HR_all"][s], self.Wh["out"])], self.bd["out"])
            put("O_all", s, torch.tanh(pre), self.bgate(sl, 1.0), (rec, lambda p, r, c_: torch.tanh(p)))
            u, o = S["U_all"][s], S["O_all"][s]
            v = (h * (1 - u) + o * u) * k[s]           # 5 operations: 1 - u, h *, o * u, +, * k
            put("H_all", s + 1, v, self.bT(v, 5 * U24 * (h.abs() * (1 + u.abs()) + (o * u).abs()) * k[s]))
            i = s - (n_agg - 1)
            if 0 <= i < P:
                pre, sl, rec = self.gemm([(S["H_all"][s + 1], self.W1)], self.bd["p0"])
                put("P1_all", i, torch.relu(pre), self.bT(torch.relu(pre), sl), (rec, lambda p, r, c_: torch.relu(p)))
                pre, sl, rec = self.gemm([(S["P1_all"][i], self.W2)], self.bd["p2"])
                put("pred", i, pre, self.bT(pre, sl), (rec, ident))
                if i < P - 1:
                    put("X_all", s + 1, torch.relu(S["pred"][i]))   # rounding commutes with relu
        if not backward:
            return Q, S
        # ---------------- backward: dh carried in f64, its f32 error budget e beside it
        dh = self.d_hlast.double() if c.hlast else torch.zeros(M, D, dtype=torch.float64)
        e = torch.zeros(M, D, dtype=torch.float64)

        def step_bwd(s, dh, e):
            u, o, r, h, kk = S["U_all"][s], S["O_all"][s], S["R_all"][s], S["H_all"][s], k[s]
            dhn = dh * kk                                   # 1 operation
            en = e * kk + U24 * dhn.abs()
            f_u = (o - h) * u * (1 - u)                     # G_u = dhn (o - h) u (1 - u): 5 operations: o - h, *, * u, 1 - u, *
            put("G_u", s, dhn * f_u, self.bT(dhn * f_u, en * f_u.abs() + 5 * U24 * dhn.abs() * (o.abs() + h.abs()) * u * (1 + u)))
            f_o = u * (1 - o * o)                           # G_o = dhn u (1 - o o): 4 operations: * u, o * o, 1 -, *
            put("G_o", s, dhn * f_o, self.bT(dhn * f_o, en * f_o.abs() + 4 * U24 * dhn.abs() * u * (1 + o * o)))
            dp = dhn * (1 - u)                              # 2 operations: 1 - u, *
            e_dp = en * (1 - u) + 2 * U24 * dhn.abs() * (1 + u)
            Go = S["G_o"][s]
            g, sl_g, rec = self.gemm([(Go, self.Wh["out"].t().contiguous())])        # dhr = G_o @ Wo_h
            f_r = h * r * (1 - r)                           # G_r = dhr h r (1 - r): 4 operations: * h, * r, 1 - r, *
            put("G_r", s, g * f_r, self.bT(g * f_r, sl_g * f_r.abs() + 4 * U24 * g.abs() * h.abs() * r * (1 + r)),
                (rec, lambda p, rr, cc, f_r=f_r: p * f_r[rr, cc]))
            e_dp = e_dp + sl_g * r + 2 * U24 * ((g * r).abs() + dp.abs())            # dp += dhr r: 2 operations
            dp = dp + g * r
            Gu, Gr = S["G_u"][s], S["G_r"][s]
            dx, sl_dx, rec_dx = self.gemm([(Gu, self.Wx["update"].t().contiguous()), (Gr, self.Wx["reset"].t().contiguous()),
                                           (Go, self.Wx["out"].t().contiguous())])
            gh, sl_h, _ = self.gemm([(Gu, self.Wh["update"].t().contiguous()), (Gr, self.Wh["reset"].t().contiguous())])
            e = e_dp + sl_h + U24 * (dp.abs() + gh.abs())                             # dh = dp + .: 1 operation
            return dp + gh, e, dx, sl_dx, rec_dx

        step = ns
        for i in range(P - 1, -1, -1):
            feeds = i < P - 1
            g, sl = self.d_pred_rows[i], torch.zeros(M, D, dtype=torch.float64)
            if feeds:
                step -= 1
                dh, e, dx, sl_dx, _ = step_bwd(step, dh, e)
                gate = (S["X_all"][step] > 0).double()
                sl = gate * sl_dx + U24 * (g.abs() + (gate * dx).abs())               # dP2 = d_pred + [x > 0] dx: 1 operation
                g = g + gate * dx
                put("dxn", 0, dx, sl_dx)      # ws[1] keeps the dx of the last prediction-fed step the backward reaches (i = 0)
            put("dP2", i, g, self.bT(g, sl))
            gate1 = (S["P1_all"][i] > 0).double()
            pre, sl, rec = self.gemm([(S["dP2"][i], self.W2.t().contiguous())])
            put("dP1", i, pre * gate1, self.bT(pre * gate1, sl * gate1), (rec, lambda p, rr, cc, gate1=gate1: p * gate1[rr, cc]))
            g1, sl1, _ = self.gemm([(S["dP1"][i], self.W1.t().contiguous())])
            e = e + sl1 + U24 * (dh.abs() + g1.abs())                                  # dh += dP1 @ W1: 1 operation
            dh = dh + g1
        for t in range(n_agg - 1, -1, -1):
            step -= 1
            dh, e, dx, sl_dx, rec_dx = step_bwd(step, dh, e)
            put("d_x", t, dx, sl_dx, (rec_dx, ident))
        assert step == 0
        put("dh0", 0, dh, e)
        return (Q, S) if model else Q

    # ---- teeth, from the model alone ------------------------------------------------------------------------------------------------
    def blocks(self, n_slabs):
        M, D = self.M, self.c.D
        last = (n_slabs - 1, slice((M - 1) // TILE * TILE, M), slice(D - TILE, D))        # ragged last row tile x last column tile
        first = (min(1, n_slabs - 1), slice(0, min(TILE, M)), slice(0, TILE))
        return [last] if first == last else [last, first]

    def positions(self, A, rows, unit):
        """first, last and two inner MFMA K-steps of an operand half; unit = 1 (f32-stored tensors): ONE index of each, the one whose
        operand column is largest over the block's rows (chosen from reference data; a K-step of zeros is the skipped case)"""
        n = A.shape[1] // self.kstep
        steps = [slice(p * self.kstep, (p + 1) * self.kstep) for p in sorted({0, n // 3, (2 * n) // 3, n - 1})]
        if unit > 1:
            return steps
        at = [ks.start + int(A[rows, ks].abs().amax(0).argmax()) for ks in steps]
        return [slice(i, i + 1) for i in at]

    def teeth(self, Q):
        sampled = skipped = 0
        for name in FED:
            h = Q[name]
            if not h.rec:
                continue
            unit = 1 if KIND[name] in ("gate", "f32") else self.kstep
            for idx, rows, cols in self.blocks(h.ref.shape[0]):
                rec = h.rec[idx]
                for part, (A, _) in enumerate(rec.parts):
                    for ks in self.positions(A, rows, unit):
                        sampled += 1
                        if not bool((A[rows, ks] != 0).any()):
                            skipped += 1
                            continue
                        moved = (dropped(rec, Mut(name, idx, rows, cols, part, ks)) - h.ref[idx][rows, cols]).abs()
                        assert bool((moved > 4 * h.bound[idx][rows, cols]).any()), \
                            (f"{name}[{idx}] rows {rows} cols {cols}: leaving out indices {ks} of operand {part} moves no element by more "
                             f"than 4 x its bound (largest ratio {(moved / h.bound[idx][rows, cols]).max().item():.3g})")
        assert sampled and skipped * 4 <= sampled, f"{skipped} of {sampled} reduction positions carry an all-zero operand column"
        return sampled


@functools.lru_cache(maxsize=None)
def chain_with_teeth(c, dtype):
    ch = Chain(c, dtype)
    Q, _ = ch.evaluate()
    ch.teeth(Q)
    return ch


# ---- device side ------------------------------------------------------------------------------------------------------------------
class Buf:
    """[rows][width] of `dtype` with a guard band of one 32-row tile in front of it and one behind it"""

    def __init__(self, k, rows, width, dtype):
        self.n, self.g = rows * width, TILE * width
        self.flat = k.empty(self.n + 2 * self.g, dtype=dtype)
        self.itype, self.pat = (torch.int16, 0x5A5A) if dtype == BF16 else (torch.int32, 0x5A5A5A5A)
        self.flat.view(self.itype).fill_(self.pat)
        self.body = self.flat[self.g:self.g + self.n]
        self.body.fill_(float("nan"))          # pure output until an input is copied in

    def bands_intact(self):
        v = self.flat.view(self.itype)
        return bool((v[:self.g] == self.pat).all()) and bool((v[self.g + self.n:] == self.pat).all())

    def bits(self):
        return self.flat.view(self.itype).cpu().clone()


_BUFS = {"X_all": ("ns", 1, None), "H_all": ("ns1", 1, None), "HR_all": ("ns", 1, None), "U_all": ("ns", 1, F32), "R_all": ("ns", 1, F32),
         "O_all": ("ns", 1, F32), "P1_all": ("P", 1, None), "pred": ("P", 1, None), "G_all": ("ns", 3, None), "dP1": ("P", 1, None),
         "dP2": ("P", 1, None), "d_x": ("n_agg", 1, F32), "ws": ("two", 1, F32)}


class Run:
    """the case's buffers (outputs poisoned, everything banded) and descriptor"""

    def __init__(self, k, ch: Chain):
        self.k, self.ch = k, ch
        c, dtype, D, M, ns, P = ch.c, ch.dtype, ch.c.D, ch.M, ch.ns, ch.c.P
        slabs = {"ns": ns, "ns1": ns + 1, "P": P, "n_agg": c.n_agg, "two": 2}
        self.buf = {n: Buf(k, slabs[s] * M, w * D, dt or dtype) for n, (s, w, dt) in _BUFS.items() if slabs[s] > 0}
        self.view = {n: b.body.view(-1, M, b.g // TILE) for n, b in self.buf.items()}
        self.view["X_all"][:c.n_agg] = k.t(ch.x, dtype)
        self.view["H_all"][0] = k.t(ch.h0, dtype)
        w = ch.w
        self.packed = k.empty(16 * D * D, dtype=dtype)
        self.inputs = [k.t(w[n]) for n in ("update", "reset", "out")] + ([k.t(w["p0"]), k.t(w["p2"])] if P > 0 else [None, None])
        k.call("dpc_gru_pack", *self.inputs, D, L.dtype_code(dtype), self.packed)
        self.bias = {n: k.t(v) for n, v in ch.b.items()}
        d = self.d = L.GruChainDesc()
        d.dtype, d.M, d.D, d.SQ, d.P, d.n_agg, d.n_steps = L.dtype_code(dtype), M, D, c.SQ, P, c.n_agg, ns
        d.p_drop, d.seed = P_DROP, SEED
        d.packed = self.packed.data_ptr()
        for f, n in (("bias_u", "update"), ("bias_r", "reset"), ("bias_o", "out"), ("bias_1", "p0"), ("bias_2", "p2")):
            setattr(d, f, self.bias[n].data_ptr())
        for n, b in self.buf.items():
            setattr(d, n, b.body.data_ptr())
        if P > 0:
            self.d_pred = k.t(ch.d_pred)
            d.d_pred = self.d_pred.data_ptr()
        if c.hlast:
            self.d_hlast = k.t(ch.d_hlast)
            d.d_hlast = self.d_hlast.data_ptr()
        if c.drop == "masks":
            self.masks = k.t(ch.masks)
            d.drop_masks = self.masks.data_ptr()
        elif c.drop == "philox":
            self.step = torch.tensor([c.step], dtype=torch.int32, device=k.dev)
            d.step_dev = self.step.data_ptr()

    def go(self):
        self.k.call("dpc_gru_chain_fwd", C.byref(self.d))
        self.k.call("dpc_gru_chain_bwd", C.byref(self.d))
        self.k.sync()
        return self

    def saved(self):
        """the saved tensors as evaluate() reads them (f64, CPU); pred in row order m = (b, sq)"""
        ch, D, P = self.ch, self.ch.c.D, self.ch.c.P
        S = {n: v.detach().cpu().double() for n, v in self.view.items()}
        G = S.pop("G_all")
        S["G_u"], S["G_r"], S["G_o"] = G[..., :D].contiguous(), G[..., D:2 * D].contiguous(), G[..., 2 * D:].contiguous()
        if P > 0:
            S["pred"] = S["pred"].reshape(ch.B, P, ch.c.SQ, D).permute(1, 0, 2, 3).reshape(P, ch.M, D)
        else:
            for n in ("P1_all", "pred", "dP1", "dP2"):
                S[n] = torch.zeros(0, ch.M, D, dtype=torch.float64)
        return S

    def bits(self):
        return {n: b.bits() for n, b in self.buf.items()}


def hold(tier, label, ch, S):
    """every saved tensor of a finished run against its step-pinned reference"""
    c, ws = ch.c, S.pop("ws")
    # inputs are read, never written
    assert torch.equal(S["X_all"][:c.n_agg], ch.x.double()) and torch.equal(S["H_all"][0], ch.h0.double())
    # poison: every pure output was written in full (ws[1] only when a prediction feeds a step)
    kc.all_finite(*[S[n] for n in S if S[n].numel()], ws[:2 if c.P > 1 else 1])
    Q = ch.evaluate(S)
    S["dh0"], S["dxn"] = ws[:1], ws[1:]
    for name, h in Q.items():
        valid = ~torch.isnan(h.ref)
        if not bool(valid.any()):
            continue
        got, ref, bound = S[name][valid], h.ref[valid], h.bound[valid]
        if KIND[name] == "exact":
            assert torch.equal(got, ref), f"{label} {name}: {int((got != ref).sum())} elements are not the exact value"
            continue
        err = (got - ref).abs()
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), err)).max().item()
        WORST[(tier, name)] = max(WORST.get((tier, name), 0.0), ratio)
        line = f"[gru-held] {tier} {label} {name}: worst error / bound {ratio:.3g}"
        if KIND[name] == "gate":
            GATE_SEEN[tier] = max(GATE_SEEN.get(tier, 0.0), err.max().item())
            line += f", max |got - ref| {err.max().item():.3g}"
        print(line)
        assert bool((err <= bound).all()), f"{label} {name}: error / bound {ratio:.3g} at {int((err > bound).sum())} elements"


def chain_case(k, tier, name, c, dtype):
    ch = chain_with_teeth(c, dtype)     # data, model and teeth before the kernel's result is looked at
    run = Run(k, ch).go()
    assert all(b.bands_intact() for b in run.buf.values()), [n for n, b in run.buf.items() if not b.bands_intact()]
    hold(tier, f"{name} {str(dtype)[6:]}", ch, run.saved())


def report_case(tier):
    """the figures docs/kernels.md quotes (pytest -s)"""
    for (t, name), v in sorted(WORST.items()):
        if t == tier:
            print(f"[gru-report] {tier} {name}: worst error / bound {v:.3g}")
    print(f"[gru-report] {tier} gates: max |got - ref| {GATE_SEEN.get(tier, float('nan')):.3g} (GATE_F32_MEASURED {GATE_F32_MEASURED:.3g})")


# ---- the regression this module is for ----------------------------------------------------------------------------------------------
def slipped_mutation_case():
    """From the model alone, at case_gru_chain's shape (3, 16, 256, 3, 5) in bf16: one MFMA K-step of the h operand left out of the
    update gate for one 32 x 32 output block at one step moves H_all (all later steps included) by less than the 0.03 of its max-abs
    that case_gru_chain allows -- and U_all, where the step-pinned bound meets it, by more than 4 x its bound."""
    ch = Chain(ENGINE, BF16)
    Q, S = ch.evaluate()
    D, slips = ENGINE.D, []
    for s in (2, 4, 6):
        for rows, cols in ((slice(0, 32), slice(0, 32)), (slice(32, 48), slice(D - 32, D))):
            for p in range(D // 16):
                m = Mut("U_all", s, rows, cols, 1, slice(p * 16, (p + 1) * 16))
                _, Sm = ch.evaluate(mut=m, backward=False)
                moved_h = (Sm["H_all"][1:] - S["H_all"][1:]).abs().max().item() / S["H_all"][1:].abs().max().item()
                moved_u = (dropped(Q["U_all"].rec[s], m) - Q["U_all"].ref[s][rows, cols]).abs()
                assert moved_h > 0 and bool((moved_u > 4 * Q["U_all"].bound[s][rows, cols]).any())
                slips.append(moved_h)
    print(f"[gru-slip] H_all moves by {min(slips):.3g} .. {max(slips):.3g} of its max-abs over {len(slips)} dropped K-steps; "
          f"{sum(v < 3e-2 for v in slips)} are below case_gru_chain's 3e-2")
    assert min(slips) < 3e-2


# ---- metamorphic: rows are independent sequences ----------------------------------------------------------------------------------
META = Case(80, 1, 96, 0, 3, h0=True, hlast=True, seed=9)


def rows_case(k, dtype):
    """80 rows, SQ = 1, LC form, explicit masks, non-zero h_0: the same rows under a permutation that moves every row to another tile
    and another position in it give bit-identical saved tensors; so do the first 37 rows run alone"""
    M = META.B
    perm = (torch.arange(M) + 33) % M          # position j of the permuted run holds row perm[j]
    j = torch.arange(M)
    assert bool((perm // TILE != j // TILE).all()) and bool((perm % TILE != j % TILE).all())
    big = Run(k, Chain(META, dtype)).go()
    shuf = Run(k, Chain(META, dtype, rows=perm)).go()
    pre = Run(k, Chain(META, dtype, rows=torch.arange(37))).go()
    for r in (big, shuf, pre):
        assert all(b.bands_intact() for b in r.buf.values())
    inv = torch.argsort(perm)
    for n, v in big.view.items():
        slabs = v.shape[0] if n != "ws" else 1     # ws[1] is not written without predictions
        it = big.buf[n].itype
        a = v[:slabs].view(it).cpu()
        assert not bool(torch.isnan(v[:slabs].float()).any()), n
        assert torch.equal(shuf.view[n][:slabs].view(it).cpu()[:, inv], a), f"{n}: a row's result depends on its place in the tile"
        assert torch.equal(pre.view[n][:slabs].view(it).cpu(), a[:, :37]), f"{n}: a row's result depends on the rows behind it"


# ---- rejections ----------------------------------------------------------------------------------------------------------------------
def gru_rejects_case(k):
    """argument errors and unsupported shapes launch nothing: poisoned outputs, inputs and guard bands stay as they were"""
    import pytest
    arg, uns = f"code {L.ERR_ARG}$", f"code {L.ERR_UNSUPPORTED}$"
    run = Run(k, Chain(Case(2, 5, 32, 2, 2, hlast=True), F32))
    before = run.bits()
    d = run.d
    fields = [f for f, _ in L.GruChainDesc._fields_]

    def rejected(code, fns=("dpc_gru_chain_fwd", "dpc_gru_chain_bwd"), **kw):
        old = {f: getattr(d, f) for f in fields}
        for f, v in kw.items():
            setattr(d, f, v)
        for fn in fns:
            with pytest.raises(L.DpcError, match=code):
                k.call(fn, C.byref(d))
        for f, v in old.items():
            setattr(d, f, v)
        k.sync()
        after = run.bits()
        assert all(torch.equal(before[n], after[n]) for n in before), f"{kw}: a rejected call wrote"

    rejected(uns, D=48)
    rejected(uns, D=288)
    rejected(uns, SQ=3)                                     # M = 10 is no multiple
    rejected(arg, n_steps=d.n_steps + 1)
    rejected(arg, n_steps=d.n_steps - 1)
    rejected(arg, P=0)                                      # n_steps = 3 != n_agg
    for f in ("M", "D", "SQ", "n_agg"):
        rejected(arg, **{f: 0})
        rejected(arg, **{f: -1})
    rejected(arg, P=-1)
    for p in (1.0, -0.1, float("nan")):
        rejected(arg, p_drop=p)
    for f in ("packed", "bias_u", "bias_r", "bias_o", "bias_1", "bias_2", "X_all", "H_all", "HR_all", "U_all", "R_all", "O_all", "P1_all", "pred"):
        rejected(arg, **{f: None})
    for f in ("G_all", "d_x", "ws", "d_pred", "dP1", "dP2"):
        rejected(arg, fns=("dpc_gru_chain_bwd",), **{f: None})
    rejected(arg, fns=("dpc_gru_chain_bwd",), P=0, n_steps=d.n_agg, d_hlast=None)   # nothing would flow into the recurrence
    rejected(arg, dtype=77)
    # dpc_gru_pack
    packed = k.poison(16 * 32 * 32)
    w3, w1 = [k.zeros(32, 64) for _ in range(3)], k.zeros(32, 32)     # real inputs of calls that must not read them
    for p0, p2, D, code in ((w1, None, 32, arg), (None, w1, 32, arg), (w1, w1, 0, arg), (w1, w1, 48, uns), (w1, w1, 288, uns)):
        with pytest.raises(L.DpcError, match=code):
            k.call("dpc_gru_pack", *w3, p0, p2, D, L.F32, packed)
    with pytest.raises(L.DpcError, match=arg):
        k.call("dpc_gru_pack", *w3, w1, w1, 32, 77, packed)
    with pytest.raises(L.DpcError, match=arg):
        k.call("dpc_gru_pack", None, w3[1], w3[2], w1, w1, 32, L.F32, packed)
    k.sync()
    assert bool(torch.isnan(packed).all())
