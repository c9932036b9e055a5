"""f32 contractions held to f32-grade error term by term: the cases shared by the CPU tier (kernels on the host SIMT simulator,
tests/test_x6_emu.py) and the GPU tier (libdpc_hip.so on an MI355X, tests/test_x6_gpu.py).

The f32 kernels multiply either in chains of v_mfma_f32_32x32x2_f32 ("exact") or with every operand split in registers into three
bf16 pieces, x = x1 + x2 + x3, and the six piece products (1,1) (2,1) (1,2) (2,2) (3,1) (1,3) on the bf16 matrix pipe ("bf16x6":
csrc/dpc_rt.h split3_f32x8 / mfma_f32x6; switch dpc_set_f32_matmul).  kcases.tol(f32) = 1e-4 of max-abs cannot tell six terms from
three; the bounds here can.

The term-loss rule.  Every operation is bilinear, L(a, b): conv forward (x, w), input-gradient (gy, w), weight-gradient (x, gy),
GEMM (A, B).  The reference is L in f64 on the f32 operands.  The loss of term (i, j) is L(a_i, b_j) in f64 -- what a kernel without
that MFMA would miss.  A case's bound is 1/4 of the smallest non-zero loss among the six terms, in the case's metric (the x4 margin
of kcases.rejects_dropped_tap); it comes from the reference and the operands alone and is never written down as a constant.

Two operand kinds.  `random`: randn activations / gradients, 0.1 randn weights, metric rel-L2 over the tensor (bound ~ 6e-7).
Piece probes, positive coherent operands with c in {1/2, 1, 2} per element: three-piece values c (1 + 2^-9 + 2^-18), two-piece values
c (1 + 2^-9), one-piece values k/8, k = 1..15; P31 = (a three-piece, b one-piece), P13 mirrored, P22 both two-piece; metric
max |got - ref| / L(|a|, |b|) per element, so each small term costs 2^-18 on every output and the bound is ~ 2^-20.  Outputs whose
L(|a|, |b|) is 0 (positions of a strided input-gradient that no tap reaches) must be exactly 0 and are left out of the ratio.

Every reduction is at most 576 long (taps x Ci forward, the taps that can meet one input position x Co for the input-gradient, output
positions for the weight gradient): the missing-term error does not depend on the reduction length, the f32 accumulation noise grows
with its square root.  model() is the arithmetic in plain torch: products in f64, the f32 accumulator rounded after each term of each
K = 16 block in mfma_f32x6's order (bf16x6) or after each product (exact: an fmaf chain, which is bit for bit what
v_mfma_f32_32x32x2_f32 does -- simulator and MI355X gave the same figures to every printed digit).  The model has to stay below half of
every bound in both arithmetics (tests/test_x6_emu.py), and that decides how many live products an output may have:

  Measured with dense operands first (every reduction index live), error / bound at a reduction of 576:
    bf16x6, MI355X: random 0.41 .. 0.56, probes 0.29 .. 0.73 -- inside the bound (model: 0.40 .. 0.43 / 0.29 .. 0.43).
    exact, MI355X = simulator = model: random 0.50 .. 0.68, probes 2.1 .. 3.3 (3.2e-6 against a bound of 9.5e-7); still 1.06 .. 1.5 at
    128 positions (wgrad2_kernel), 0.97 at 90 (wgrad_kernel), 0.38 .. 0.42 at 32 .. 36.  The kernels are right; an f32 fmaf chain over
    positive operands simply drifts by more than a quarter of 2^-18 once it is longer than ~ 90 products.
  So the reductions are shortened, as arithmetic and not as shapes: LIVE["random"] = 128 and LIVE["probe"] = 16 are the largest powers
  of two at which the model of both arithmetics is below 0.45 of every bound (measured: <= 0.41).  A case whose reduction is longer
  keeps that share of operand b's reduction indices (one per stratum of the kernel's reduction order, the rest are zeros): the
  kernel still walks its full shape -- 18 chunks at 576, every one with live products -- and each term still costs every output
  its full 2^-18, but the accumulator takes only LIVE rounding steps.

Which MFMA of mfma_f32x6 a term is: the kernels' A operand is the case's a for igemm_kernel, but dy -- the case's b -- for the weight
gradients, so deleting the a.p[2] x b.p[0] line there is the loss of term (1,3), carried by P13.  Checked by hand (not committed): with
any one of the six lines deleted, random and the probes that carry the term fail on the simulator for igemm_kernel, wgrad_kernel and
wgrad2_kernel alike, and nothing else does; conv_halo_kernel<float,...> never notices.

Shapes that differ from the layer-like shapes one would write down first, and why:
  * forward `gather == 2` case: Ci = 4, not 12 -- make_gather_geom takes only power-of-two Ci when there is more than one tap.  Ci = 4
    keeps the edge: Ci = 4 mod 8, one 16-byte unit per tap, so the two units of every split pair come from different taps.
  * strided 3x3x3 input-gradient: Co = 32, not 16 -- the parity-class form (GATHER 3) wants whole 32-element chunks per tap, Co = 16
    runs GATHER 0.  Nominally 27 x 32 = 864, but at stride 2 at most 2 x 2 x 2 taps meet one input position: 256 products.
  * the conv_halo_kernel<float,...> case: Ci = 32, not 64 -- the patch kernel takes 128-byte positions only (conv_halo.hip halo_plan);
    an f32 1x3x3 conv over 64 channels runs igemm_kernel and takes the switch.
  * the padded-grid weight gradient (2, 64, 128, 2, 14, 14), 3x3x3 stride 2: T = 2 gives ONE output frame, 2 x 49 = 98 real positions
    on two 8 x 8 grids (128 rows, 4 chunks of 32).

Worst error / bound per kernel over all its cases and operand kinds, exact | bf16x6 (must be < 1; run either test file with -s):
                              simulator         MI355X
  igemm_kernel              0.344 | 0.512    0.344 | 0.515
  wgrad_kernel              0.269 | 0.223    0.269 | 0.224
  wgrad2_kernel             0.339 | 0.365    0.339 | 0.366
  wgrad2_kernel, padded     0.315 | 0.279    0.315 | 0.279
  conv_halo_kernel<float>   0.334 | 0.334    0.334 | 0.334   (no bf16x6 form: identical bits under the switch)
  model(), worst case       0.343 | 0.404
The simulator's bf16 MFMA rounds the accumulator once per lane half (tests/simt_emu/simt_emu.h), which is what the MI355X was measured
to do; with one rounding per product, as before, the simulator's bf16x6 figures were up to twice the hardware's.
"""
import contextlib
import ctypes as C
import functools
import itertools

import torch
import torch.nn.functional as F

from dpc_amd import _lib as L
from kcases import K, check_kernel, cl, conv_desc

F32 = torch.float32
TERMS = ((3, 1), (1, 3), (2, 2), (2, 1), (1, 2), (1, 1))   # mfma_f32x6's order: smallest first
KINDS = ("random", "P31", "P13", "P22")
MAX_REDUCTION = 576
# rounding steps of the f32 accumulator per output that the bound leaves room for (docstring above): live products per output
LIVE = {"random": 128, "probe": 16}


# ------------------------------------------------------------------ the switch
@contextlib.contextmanager
def f32_matmul(k: K, mode: int):
    """the process-wide arithmetic of the f32 kernels (0 exact, 1 bf16x6) for the duration of the block; lib._f32_mode -- the
    engine's idea of what the library holds (engine.py) -- follows the library both ways"""
    prev = k.lib.call("dpc_set_f32_matmul", mode)
    k.lib._f32_mode = mode
    try:
        yield
    finally:
        k.lib.call("dpc_set_f32_matmul", prev)
        k.lib._f32_mode = prev


def current_mode(k: K) -> int:
    prev = k.lib.call("dpc_set_f32_matmul", 0)
    k.lib.call("dpc_set_f32_matmul", prev)
    return prev


# ------------------------------------------------------------------ plain-torch model of the arithmetic
def split3(x):
    """the three bf16 pieces of an f32 tensor as f32 tensors: round-to-nearest casts of successive residuals (split3_f32x8)"""
    x1 = x.bfloat16().float()
    r = x - x1
    x2 = r.bfloat16().float()
    x3 = (r - x2).bfloat16().float()
    return x1, x2, x3


def assert_split_exact(x):
    p = split3(x)
    assert torch.equal((p[0] + p[1]) + p[2], x), "x1 + x2 + x3 != x in f32"
    assert torch.equal(p[0].double() + p[1].double() + p[2].double(), x.double()), "x1 + x2 + x3 != x"


def model(A, B, mode, drop=None):
    """A [M, K] @ B [N, K]^T as the kernels accumulate it: products in f64, the accumulator rounded to f32 after each term of each
    K = 16 block (mode 1; `drop` = one of TERMS left out) or after each product (mode 0: an f32 FMA chain)"""
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=F32)
    Kd = A.shape[1]
    if mode == 0:
        Ad, Bd = A.double(), B.double()
        for kk in range(Kd):
            acc = (acc.double() + Ad[:, kk, None] * Bd[None, :, kk]).float()
        return acc
    As, Bs = [p.double() for p in split3(A)], [p.double() for p in split3(B)]
    for k0 in range(0, Kd, 16):
        for (i, j) in TERMS:
            if (i, j) != drop:
                acc = (acc.double() + As[i - 1][:, k0:k0 + 16] @ Bs[j - 1][:, k0:k0 + 16].t()).float()
    return acc


# ------------------------------------------------------------------ operands
def _probe_values(shape, pieces, g):
    c = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, shape, generator=g)]
    if pieces == 3:
        return (c.double() * (1 + 2.0 ** -9 + 2.0 ** -18)).float()
    if pieces == 2:
        return (c.double() * (1 + 2.0 ** -9)).float()
    return torch.randint(1, 16, shape, generator=g).float() / 8


_PROBE_PIECES = {"P31": (3, 1), "P13": (1, 3), "P22": (2, 2)}


def _operands(shape_a, shape_b, kind, seed, b_scale):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        return torch.randn(shape_a, generator=g), torch.randn(shape_b, generator=g) * b_scale
    pa, pb = _PROBE_PIECES[kind]
    return _probe_values(shape_a, pa, g), _probe_values(shape_b, pb, g)


# ------------------------------------------------------------------ the operations: f64 reference, GEMM view, kernel call
def _out_size(S, ks, st, pd):
    return tuple((S[i] + 2 * pd[i] - ks[i]) // st[i] + 1 for i in range(3))


def _im2col(x_cl, ks, st, pd, R):
    """[N, T, H, W, C] -> [N, To, Ho, Wo, taps, C]; tap order (kt, kh, kw) as the packed weights"""
    xp = F.pad(x_cl, (0, 0, pd[2], pd[2], pd[1], pd[1], pd[0], pd[0]))
    cols = [xp[:, kt:kt + (R[0] - 1) * st[0] + 1:st[0], kh:kh + (R[1] - 1) * st[1] + 1:st[1], kw:kw + (R[2] - 1) * st[2] + 1:st[2]]
            for kt, kh, kw in itertools.product(range(ks[0]), range(ks[1]), range(ks[2]))]
    return torch.stack(cols, 4)


def _dgrad_cols(gy_cl, ks, st, pd, S):
    """[N, To, Ho, Wo, Co] -> [N, T, H, W, taps, Co]: the output gradient every (input position, tap) pair meets, 0 where there is
    none: gy spread out by the stride, then gx[i] = sum_k gyd[i + p - k] w[k]"""
    N, R, Co = gy_cl.shape[0], gy_cl.shape[1:4], gy_cl.shape[4]
    gyd = gy_cl.new_zeros(N, *[(R[i] - 1) * st[i] + 1 for i in range(3)], Co)
    gyd[:, ::st[0], ::st[1], ::st[2]] = gy_cl
    pads = []
    for i in (2, 1, 0):
        lo = ks[i] - 1 - pd[i]
        pads += [lo, S[i] + ks[i] - 1 - lo - gyd.shape[1 + i]]
    gp = F.pad(gyd, [0, 0] + pads)
    cols = [gp[:, ks[0] - 1 - kt:ks[0] - 1 - kt + S[0], ks[1] - 1 - kh:ks[1] - 1 - kh + S[1], ks[2] - 1 - kw:ks[2] - 1 - kw + S[2]]
            for kt, kh, kw in itertools.product(range(ks[0]), range(ks[1]), range(ks[2]))]
    return torch.stack(cols, 4)


class Case:
    """one operation at one shape.  a / b are the bilinear operands in the reference's layouts (NCDHW activations, [Co][Ci][kt][kh][kw]
    weights, row-major matrices); results are compared in the kernel's own layout."""

    def __init__(self, name, op, shape, expect, switched=True, seed=0, pad=0):
        self.name, self.op, self.shape, self.expect, self.switched, self.seed, self.pad = name, op, shape, expect, switched, seed, pad
        if op in ("gemm", "splitk"):
            M, N, Kd = shape
            self.shape_a, self.shape_b, self.reduction = (M, Kd), (N, Kd), Kd
        else:
            N, Ci, Co, T, H, W, ks, st, pd = shape
            self.S, self.ks, self.st, self.pd = (T, H, W), ks, st, pd
            self.R = _out_size(self.S, ks, st, pd)
            self.taps = ks[0] * ks[1] * ks[2]
            xs, ws, ys = (N, Ci, T, H, W), (Co, Ci, *ks), (N, Co, *self.R)
            self.shape_a, self.shape_b = {"fwd": (xs, ws), "dgrad": (ys, ws), "wgrad": (xs, ys)}[op]
            reach = [-(-ks[i] // st[i]) for i in range(3)]   # taps of one dimension that can meet the same input position
            self.reduction = {"fwd": self.taps * Ci, "dgrad": reach[0] * reach[1] * reach[2] * Co,
                              "wgrad": N * self.R[0] * self.R[1] * self.R[2]}[op]
        assert self.reduction <= MAX_REDUCTION, (name, self.reduction)

    def __repr__(self):
        return self.name

    def operands(self, kind):
        """the operands of one kind; where the case's reduction is longer than LIVE[kind] allows, operand b keeps only that share of
        its reduction indices (one per stratum of the kernel's reduction order, so every chunk of the kernel's loop still carries
        live products): the kernel walks the full shape, the f32 accumulator takes LIVE[kind] rounding steps"""
        b_scale = 0.1 if self.op in ("fwd", "dgrad") else 1.0
        seed = self.seed + KINDS.index(kind)
        a, b = _operands(self.shape_a, self.shape_b, kind, seed, b_scale)
        cap = LIVE["random" if kind == "random" else "probe"]
        if self.reduction > cap:
            b = b * self._reduction_mask(cap, seed)
        return a, b

    def _reduction_mask(self, cap, seed):
        """0 / 1 over operand b's reduction index, broadcastable to b"""
        g = torch.Generator().manual_seed(1000 + seed)
        if self.op in ("gemm", "splitk"):
            n, view = self.shape[2], lambda m: m.reshape(1, -1)
        elif self.op == "fwd":       # b = w [Co][Ci][kt][kh][kw], reduction order (tap, ci)
            Ci = self.shape[1]
            n, view = self.taps * Ci, lambda m: m.reshape(*self.ks, Ci).permute(3, 0, 1, 2).unsqueeze(0)
        elif self.op == "dgrad":     # b = w, reduction order (tap, co)
            Co = self.shape[2]
            n, view = self.taps * Co, lambda m: m.reshape(*self.ks, Co).permute(3, 0, 1, 2).unsqueeze(1)
        else:                        # b = gy [N][Co][To][Ho][Wo], reduction over the output positions
            N = self.shape[0]
            n, view = N * self.R[0] * self.R[1] * self.R[2], lambda m: m.reshape(N, 1, *self.R)
        live = -(-n * cap // self.reduction)
        lo = torch.arange(live) * n // live
        hi = (torch.arange(live) + 1) * n // live
        idx = lo + (torch.rand(live, generator=g) * (hi - lo)).long()
        m = torch.zeros(n)
        m[idx] = 1.0
        return view(m)

    # -- L(a, b) in f64, in the layout the kernel writes
    def L(self, a, b):
        a, b = a.double(), b.double()
        if self.op in ("gemm", "splitk"):
            return a @ b.t()
        N, Ci, Co = self.shape[:3]
        if self.op == "fwd":
            return cl(F.conv3d(a, b, None, self.st, self.pd))
        if self.op == "dgrad":
            x = torch.zeros(N, Ci, *self.S, dtype=torch.float64, requires_grad=True)
            return cl(torch.autograd.grad(F.conv3d(x, b, None, self.st, self.pd), x, a)[0])
        w = torch.zeros(Co, Ci, *self.ks, dtype=torch.float64, requires_grad=True)
        return torch.autograd.grad(F.conv3d(a, w, None, self.st, self.pd), w, b)[0]

    # -- the same product as A [M, K] @ B [N, K]^T with the reduction index in the kernel's order, and the way back
    def gemm_view(self, a, b):
        if self.op in ("gemm", "splitk"):
            return a, b, lambda o: o
        N, Ci, Co = self.shape[:3]
        if self.op == "fwd":
            A = _im2col(cl(a), self.ks, self.st, self.pd, self.R).reshape(-1, self.taps * Ci)
            return A, b.permute(0, 2, 3, 4, 1).reshape(Co, -1), lambda o: o.reshape(N, *self.R, Co)
        if self.op == "dgrad":
            A = _dgrad_cols(cl(a), self.ks, self.st, self.pd, self.S).reshape(-1, self.taps * Co)
            return A, b.permute(1, 2, 3, 4, 0).reshape(Ci, -1), lambda o: o.reshape(N, *self.S, Ci)
        Am = _im2col(cl(a), self.ks, self.st, self.pd, self.R).reshape(-1, self.taps * Ci).t()   # a = x stays the left operand
        return Am, cl(b).reshape(-1, Co).t(), lambda o: o.t().reshape(Co, *self.ks, Ci).permute(0, 4, 1, 2, 3)

    # -- device buffers once, then one launch per call: both modes run on the same buffers
    def prepare(self, k: K, a, b):
        nan = float("nan")
        if self.op == "gemm":
            M, N, Kd = self.shape
            d = conv_desc(F32, F32, 0, M, (1, 1, 1), (1, 1, 1), Kd, Kd, N, Kd, N, (1, 1, 1), (1, 1, 1), (0, 0, 0))
            ka, kb, out = k.t(a), k.t(b), k.empty(M, N)

            def run():
                out.fill_(nan)
                k.call("dpc_conv_igemm", C.byref(d), ka, kb, out, None, None)
                check_kernel(k, self.expect)
                return out, L.last_kernel(k.lib)
            return run
        if self.op == "splitk":
            M, N, Kd = self.shape
            ld = Kd + self.pad
            Ap, Bp = torch.full((M, ld), 77.0), torch.full((N, ld), -55.0)   # the padding columns must not be read
            Ap[:, :Kd], Bp[:, :Kd] = a, b
            ns = C.c_int32(0)
            k.call("dpc_gemm_nt_splitk", L.dtype_code(F32), M, N, Kd, None, ld, None, ld, None, C.byref(ns))
            assert ns.value > 1, "the case is meant to split the reduction"
            ka, kb, part, out = k.t(Ap), k.t(Bp), k.empty(ns.value, M, N), k.empty(M, N)

            def run():
                part.fill_(nan); out.fill_(nan)
                k.call("dpc_gemm_nt_splitk", L.dtype_code(F32), M, N, Kd, ka, ld, kb, ld, part, C.byref(ns))
                check_kernel(k, self.expect)
                kern = L.last_kernel(k.lib)
                k.call("dpc_reduce_unpack", part, ns.value, out, M, 1, N, N, 0, 1, 0)
                return out, kern
            return run
        N, Ci, Co = self.shape[:3]
        ks, st, pd, taps = self.ks, self.st, self.pd, self.taps
        if self.op == "fwd":
            d = conv_desc(F32, F32, 0, N, self.R, self.S, Ci, Ci, Co, taps * Ci, Co, ks, st, pd)
            src, wp, out = k.t(cl(a)), k.t(b.permute(0, 2, 3, 4, 1).reshape(Co, taps * Ci)), k.empty(N, *self.R, Co)
        elif self.op == "dgrad":
            d = conv_desc(F32, F32, 1, N, self.S, self.R, Co, Co, Ci, taps * Co, Ci, ks, st, pd)
            src, wp, out = k.t(cl(a)), k.t(b.permute(1, 2, 3, 4, 0).reshape(Ci, taps * Co)), k.empty(N, *self.S, Ci)
        if self.op in ("fwd", "dgrad"):
            def run():
                out.fill_(nan)
                k.call("dpc_conv_igemm", C.byref(d), src, wp, out, None, None)
                check_kernel(k, self.expect)
                return out, L.last_kernel(k.lib)
            return run
        d = conv_desc(F32, F32, 0, N, self.R, self.S, Ci, Ci, Co, taps * Ci, Co, ks, st, pd)
        ns = C.c_int32(0)
        k.call("dpc_conv_wgrad", C.byref(d), None, None, Co, None, C.byref(ns))
        xk, gk, part, dw = k.t(cl(a)), k.t(cl(b)), k.empty(ns.value, Co, taps * Ci), k.empty(Co, Ci, *ks)

        def run():
            part.fill_(nan); dw.fill_(nan)
            k.call("dpc_conv_wgrad", C.byref(d), xk, gk, Co, part, C.byref(ns))
            check_kernel(k, self.expect)
            kern = L.last_kernel(k.lib)
            k.call("dpc_reduce_unpack", part, ns.value, dw, Co, taps, Ci, Ci * taps, 1, taps, 0)
            return dw, kern
        return run


# ------------------------------------------------------------------ reference, term losses, bound: once per (case, kind)
class Ref:
    pass


def _metric(kind, diff, ref, denom):
    """random: rel-L2 over the tensor; probes: max |diff| / L(|a|, |b|) over the outputs a tap reaches"""
    if kind == "random":
        return (diff.norm() / ref.norm()).item()
    live = denom > 0
    return (diff[live].abs() / denom[live]).max().item()


@functools.lru_cache(maxsize=None)
def reference(case: Case, kind: str) -> Ref:
    r = Ref()
    r.a, r.b = case.operands(kind)
    assert_split_exact(r.a)
    assert_split_exact(r.b)
    r.ref = case.L(r.a, r.b)
    r.denom = case.L(r.a.abs(), r.b.abs())
    r.dead = r.denom == 0                       # outputs no tap reaches: exactly 0, left out of the ratio
    ap, bp = split3(r.a), split3(r.b)
    r.loss = {(i, j): _metric(kind, case.L(ap[i - 1], bp[j - 1]), r.ref, r.denom) for (i, j) in TERMS}
    live = [v for v in r.loss.values() if v > 0]
    r.bound = 0.25 * min(live)
    return r


def error(case: Case, kind: str, got) -> float:
    r = reference(case, kind)
    got = got.detach().cpu().double()
    assert torch.isfinite(got).all(), "an output was not written"
    assert bool((got[r.dead] == 0).all()), "outputs no tap reaches must be exactly 0"
    return _metric(kind, got - r.ref, r.ref, r.denom)


def model_error(case: Case, kind: str, mode: int, drop=None) -> float:
    r = reference(case, kind)
    A, B, back = case.gemm_view(r.a, r.b)
    return error(case, kind, back(model(A.contiguous(), B.contiguous(), mode, drop)))


def gemm_view_error(case: Case, kind: str) -> float:
    """the GEMM view the model works on is the operation the reference computes (f64 against f64)"""
    r = reference(case, kind)
    A, B, back = case.gemm_view(r.a, r.b)
    return ((back(A.double() @ B.double().t()) - r.ref).abs().max() / r.ref.abs().max()).item()


def probe_terms_seen():
    """every one of the six terms has a non-zero loss in at least one probe of every case"""
    for case in CASES:
        seen = {t for kind in KINDS[1:] for t, v in reference(case, kind).loss.items() if v > 0}
        assert seen == set(TERMS), (case, seen)


# ------------------------------------------------------------------ running a case on a library
RESULTS = {}   # (tier, kernel family, mode) -> worst error / bound


def _family(kern):
    for f in ("wgrad2_kernel", "wgrad_kernel", "igemm_kernel", "conv_halo_kernel"):
        if kern.startswith(f):
            return f + ("|padded=1" if "padded=1" in kern else "")
    return kern.split("<")[0]


def run_case(k: K, case: Case, kind: str, tier: str):
    """both arithmetics on the same device buffers: each within the bound; a kernel with a bf16x6 path gives different bits under the
    switch (random operands: the proof that the switch reached the kernel -- the plan string does not say which arithmetic ran;
    on a probe the few live products can round alike both ways, 5 of the 39 switched probe runs on the MI355X, so there it is only
    printed), a kernel without one the same bits"""
    r = reference(case, kind)
    run = case.prepare(k, r.a, r.b)
    got, errs = {}, {}
    for mode in (0, 1):
        with f32_matmul(k, mode):
            out, kern = run()
            k.sync()
        got[mode] = out.detach().cpu().clone()
        errs[mode] = error(case, kind, got[mode])
        key = (tier, _family(kern), "bf16x6" if mode else "exact")
        RESULTS[key] = max(RESULTS.get(key, 0.0), errs[mode] / r.bound)
        print(f"x6 [{tier}] {case.name:<22} {kind:<6} {'bf16x6' if mode else 'exact ':<6} error {errs[mode]:.3e}  bound {r.bound:.3e}  "
              f"ratio {errs[mode] / r.bound:.3f}  {kern}")
    same = torch.equal(got[0], got[1])
    print(f"x6 [{tier}] {case.name:<22} {kind:<6} bits across the switch: {'identical' if same else 'different'}")
    if not case.switched:
        assert same, "a kernel without a bf16x6 path changed its result under the switch"
    elif kind == "random":
        assert not same, "the switch did not reach the kernel: bf16x6 and exact results are bit-identical"
    for mode in (0, 1):
        assert errs[mode] < r.bound, f"{case.name} {kind} mode {mode}: error {errs[mode]:.3e} over the bound {r.bound:.3e}"


def print_results():
    for (tier, fam, mode), v in sorted(RESULTS.items()):
        print(f"x6 worst [{tier}] {fam:<28} {mode:<6} error / bound {v:.3f}")


# ------------------------------------------------------------------ the cases (all f32)
S1, P011 = (1, 1, 1), (0, 1, 1)
CASES = [
    # igemm_kernel, forward
    Case("fwd_gather2_ragged", "fwd", (2, 4, 40, 2, 9, 7, (1, 3, 3), S1, P011), "igemm_kernel<T,TO,BN,2>"),      # Ci below a chunk, a unit per tap, ragged everything
    Case("fwd_strided_k576", "fwd", (2, 64, 64, 1, 6, 6, (1, 3, 3), (1, 2, 2), P011), "igemm_kernel<T,TO,BN,1>"),
    Case("fwd_1x1_k32", "fwd", (3, 32, 72, 1, 5, 5, S1, S1, (0, 0, 0)), "igemm_kernel<T,TO,BN,1>"),               # one chunk, ragged column tile
    Case("fwd_3x3x3_k432", "fwd", (1, 16, 32, 3, 4, 4, (3, 3, 3), S1, S1), "igemm_kernel<T,TO,BN,2>"),
    # igemm_kernel, input-gradient without addend
    Case("dgrad_unit_k576", "dgrad", (2, 32, 64, 1, 10, 16, (1, 3, 3), S1, P011), "igemm_kernel<T,TO,BN,1>", seed=10),
    Case("dgrad_parity_3x3x3", "dgrad", (2, 16, 32, 3, 8, 8, (3, 3, 3), (2, 2, 2), S1), "igemm_kernel<T,TO,BN,3>", seed=10),
    Case("dgrad_1x1_strided", "dgrad", (2, 16, 64, 1, 8, 8, S1, (1, 2, 2), (0, 0, 0)), "igemm_kernel<T,TO,BN,3>", seed=10),  # 3/4 of the outputs untouched: 0
    # weight gradient
    Case("wgrad2_128pos", "wgrad", (2, 64, 64, 1, 8, 8, (1, 3, 3), S1, P011), "wgrad2_kernel|padded=0", seed=20),
    Case("wgrad2_padded_7x7", "wgrad", (2, 64, 128, 2, 14, 14, (3, 3, 3), (2, 2, 2), S1), "wgrad2_kernel|padded=1", seed=20),  # masked lanes inside a 16-position step
    Case("wgrad_90pos_ragged", "wgrad", (5, 8, 24, 2, 6, 6, (1, 3, 3), (1, 2, 2), P011), "wgrad_kernel", seed=20),            # 3 x 3 output = 56 % of a 4 x 4 grid, below wgrad2's 60 %: ragged last chunk, ragged 16-position step
    Case("wgrad2_256pos_co72", "wgrad", (1, 64, 72, 1, 16, 16, (1, 3, 3), S1, P011), "wgrad2_kernel|padded=0", seed=20),      # ragged Co tile
    # GEMMs
    Case("gemm_200x100x264", "gemm", (200, 100, 264), "igemm_kernel<T,TO,BN,1>", seed=30),
    Case("splitk_130x64x576", "splitk", (130, 64, 576), "igemm_kernel<T,TO,BN,1>", seed=30, pad=8),
    # the f32 patch kernel has no bf16x6 path: identical bits under the switch
    Case("halo_f32_no_x6", "fwd", (1, 32, 64, 1, 32, 32, (1, 3, 3), S1, P011), "conv_halo_kernel<float", switched=False, seed=40),
]
PARAMS = [(c, kind) for c in CASES for kind in KINDS]
