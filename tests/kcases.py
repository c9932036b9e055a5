"""Kernel parity cases shared by the CPU tier (kernels executed by the host SIMT
simulator, tests/test_kernels_emu.py) and the GPU tier (the same C ABI of
libdpc_hip.so on an MI355X, tests/test_kernels_gpu.py).

Every case computes its expectation with plain torch CPU ops (f32, or f64 where
the quantity is a long reduction) -- the same ops the reference model runs
(backbone/resnet_2d3d.py, backbone/convrnn.py, dpc/model_3d.py, dpc/main.py) -- and
calls the kernel through dpc_amd._lib.

Element-wise outputs: f32 mode 1e-4 relative to the tensor's max-abs (the reference's
own fp32 noise floor is ~1e-4); bf16 mode 2^-7 relative (tol()).  Every
convolution proves that its bound rejects an expectation with one tap dropped
(rejects_dropped_tap).

Reductions over rows (the BatchNorm partial sums of the conv epilogues, the sums of the
BatchNorm backward, the pooled forms of both, dpc_colsum): the kernel's vector got[C]
is held to the f64 column sum of the per-row terms the reduction is defined over, with
a bound that no tolerance constant enters: the error must stay below a QUARTER of what
removing ONE row from the expectation changes (rejects_dropped_row; by symmetry the
same bound rejects a row counted twice).  The rows removed are the first, the middle
and the last one, for convolutions also the last row of the first 128-row tile and the
first row of the last tile (mutation_rows).  They are chosen from reference data alone:
a row whose largest term is below a tenth of the median over all rows (a ReLU-gated row
can be all zeros) gives way to the nearest row that is not.  dx of the BatchNorm
backward: one rounding of the output in bf16 (tol(bf16)), DX_F32_BOUND in f32.

Poison rule: the engine allocates its statistics tables and split-K slabs with `empty`
and shares them between layers, so a launch must write every partial row and every slab
element it promises.  Every f32 table that is purely an OUTPUT of the call under test
is therefore handed over full of NaN (K.poison) and must be finite afterwards
(all_finite); K.zeros is left to tables whose zeros are real inputs, each marked so.
"""
import ctypes as C

import torch
import torch.nn.functional as F

from dpc_amd import _lib as L


def cl(x):  # NCDHW -> channels-last contiguous
    return x.permute(0, 2, 3, 4, 1).contiguous()


def tol(dtype):
    """max-abs error relative to the tensor's max-abs.  bf16: 2^-7 = two roundings of the largest element (the kernels accumulate in
    f32 and round once; an addend is one more) -- round 3 allowed 2^-6.  Every convolution case also proves that this bound has
    teeth: an expectation with ONE tap dropped must fail it (rejects_dropped_tap)."""
    return 1e-4 if dtype == torch.float32 else 1.0 / 128


def rejects_dropped_tap(got, want, want_without_tap, bound):
    """mutation check: the tolerance that accepts `got` against `want` must reject the same result against an expectation
    computed with one kernel tap zeroed (tolerances with no margin for a missing tap)"""
    e_ok, e_mut = relerr(got, want), relerr(got, want_without_tap)
    assert e_ok < bound <= e_mut * 0.25, f"tolerance {bound:.3g}: real error {e_ok:.3g}, error against the dropped-tap expectation only {e_mut:.3g}"


def mutation_rows(ref_terms, extra=()):
    """the rows rejects_dropped_row removes: first, middle, last (+ extra), chosen from REFERENCE terms [rows, C] alone.  A row whose
    max_c |term| is below a tenth of the median of that statistic over all rows is replaced by the nearest row that reaches it."""
    stat = ref_terms.detach().double().abs().amax(1)
    n = stat.numel()
    floor = 0.1 * stat.median().item()
    assert floor > 0, "more than half of the rows carry no term at all: no row to remove"
    ok = (stat >= floor).nonzero().flatten()
    picks = []
    for r in (0, n // 2, n - 1, *extra):
        r = min(max(int(r), 0), n - 1)
        if stat[r].item() < floor:
            r0, r = r, int(ok[(ok - r).abs().argmin()])
            print(f"[mutation-rows] row {r0} of {n} carries {stat[r0].item():.3g} < {floor:.3g}: row {r} instead")
        if r not in picks:
            picks.append(r)
    return picks


def conv_tile_rows(rows, tile=128):
    """last row of the first 128-row tile, first row of the last tile"""
    return (min(tile, rows) - 1, (rows - 1) // tile * tile)


def rejects_dropped_row(got, terms, rows, what=""):
    """mutation check of a reduction over rows: got[C] against ref = terms.sum(0) (terms [rows, C] f64) must be closer than a quarter
    of its distance to the same sum with ONE row removed, for every row in `rows` (rejects_dropped_tap's factor).  Returns
    (e_ok, bound), both absolute."""
    got, terms = got.detach().double().cpu().reshape(-1), terms.detach().double()
    assert bool(torch.isfinite(got).all()), f"{what}: the reduced vector is not finite"
    ref = terms.sum(0)
    e_ok = (got - ref).abs().max().item()
    e_mut = {r: (got - (ref - terms[r])).abs().max().item() for r in rows}
    worst = min(e_mut, key=e_mut.get)
    bound = 0.25 * e_mut[worst]
    print(f"[row-reduction] {what}: rows {terms.shape[0]} C {terms.shape[1]} e_ok {e_ok:.3g} bound {bound:.3g} (row {worst})")
    assert e_ok < bound, f"{what}: error {e_ok:.3g} is not below {bound:.3g}, a quarter of the effect of dropping row {worst} of {terms.shape[0]}"
    return e_ok, bound


def all_finite(*tables):
    """a poisoned output table (K.poison) was written in full"""
    for t in tables:
        bad = int((~torch.isfinite(t)).sum())
        assert bad == 0, f"{bad} of {t.numel()} elements of an output table {tuple(t.shape)} were left unwritten"


# dx of the BatchNorm backward in f32, relerr against the f64 expectation: 8 x the largest value measured on an MI355X over the f32
# cases of test_bn / test_stem_pool of the GPU tier (1.6e-7 at 20 011 rows x 128 channels; 1.35e-7 on the host simulator;
# docs/kernels.md, `bn_*`), capped at tol(f32).  The 8 covers another summation order on another driver, not a bug.
DX_F32_MEASURED = 1.6e-7
DX_F32_BOUND = min(8 * DX_F32_MEASURED, 1e-4)


def q(x, dtype):  # quantise like the device tensor will be
    return x.to(dtype).float()


def bits_of(y, E):
    """byte-per-unit sign mask of a [rows, C] tensor (what dpc_bn_apply writes)"""
    b = (y.float().cpu().reshape(-1, E) > 0).to(torch.int32) * (1 << torch.arange(E, dtype=torch.int32))
    return b.sum(1)


def relerr(a, b):
    return (a.float().cpu() - b.float()).abs().max().item() / max(b.abs().max().item(), 1e-6)


def row_offdiag_relerr(got, want, chunk=1024):
    """per row of a [rows, cols] gradient with its target on the diagonal: max-abs error over the OFF-diagonal elements relative to
    that row's largest off-diagonal reference element -- relerr's bound, one number per row instead of one per tensor (the tensor's
    max-abs is a diagonal element, ~1/rows: under it every small off-diagonal element may be anything).  Returns the worst row's."""
    rows = want.shape[0]
    worst = 0.0
    for r0 in range(0, rows, chunk):
        w = want[r0:r0 + chunk].float()
        e = (got[r0:r0 + chunk].float().cpu() - w).abs()
        w = w.abs()
        i = torch.arange(w.shape[0])
        e[i, r0 + i] = 0
        w[i, r0 + i] = 0
        worst = max(worst, (e.amax(1) / w.amax(1).clamp_min(1e-30)).max().item())
    return worst


class K:
    """binds a Lib + device"""

    def __init__(self, lib, device):
        self.lib, self.dev = lib, torch.device(device)

    def t(self, x, dtype=None):
        x = x.to(dtype) if dtype is not None else x
        return x.contiguous().to(self.dev)

    def empty(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=self.dev)

    def zeros(self, *shape, dtype=torch.float32):
        """for tables whose zeros are a real INPUT of the call; pure outputs take poison()"""
        return torch.zeros(*shape, dtype=dtype, device=self.dev)

    def poison(self, *shape, dtype=torch.float32):
        """an f32 table that is purely an OUTPUT of the call under test: every element NaN until the kernel writes it"""
        return torch.full(shape, float("nan"), dtype=dtype, device=self.dev)

    def call(self, name, *args):
        return self.lib.call(name, *args, self.lib.stream())

    def sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize()


def check_kernel(k: K, expect):
    """the kernel the last C-ABI call launched (dpc_last_kernel) is the variant the case is meant to cover.
    expect: None, a name prefix, or "prefix|substring" (both must match)"""
    if not expect:
        return
    got = L.last_kernel(k.lib)
    pre, _, sub = expect.partition("|")
    assert got.startswith(pre) and sub in got, f"case meant for {expect}, the library launched {got}"


def conv_desc(dtype_in, dtype_out, mode, N, R, S, Ci, src_ld, Co, ldw, ldo, k, s, p):
    return L.ConvDesc(L.dtype_code(dtype_in), L.dtype_code(dtype_out), mode, N, R[0], R[1], R[2], S[0], S[1], S[2],
                      Ci, src_ld, Co, ldw, ldo, k[0], k[1], k[2], s[0], s[1], s[2], p[0], p[1], p[2])


# ------------------------------------------------------------------ conv forward (+ BN partial sums)
def case_conv_fwd(k: K, dtype, N, Ci, Co, T, H, W, ks, st, pd, seed=0, expect=None):
    g = torch.Generator().manual_seed(seed)
    x = q(torch.randn(N, Ci, T, H, W, generator=g), dtype)
    w = q(torch.randn(Co, Ci, *ks, generator=g) * 0.1, dtype)
    y = F.conv3d(x, w, None, st, pd)
    To, Ho, Wo = y.shape[2:]
    taps = ks[0] * ks[1] * ks[2]
    d = conv_desc(dtype, dtype, 0, N, (To, Ho, Wo), (T, H, W), Ci, Ci, Co, taps * Ci, Co, ks, st, pd)
    src = k.t(cl(x), dtype)
    wp = k.t(w.permute(0, 2, 3, 4, 1).reshape(Co, taps * Ci), dtype)
    out = k.empty(N, To, Ho, Wo, Co, dtype=dtype)
    rows = k.lib.call("dpc_conv_stats_rows", C.byref(d))
    stats = k.poison(rows, 2, Co)
    yr = cl(y).reshape(-1, Co).double()
    mut = mutation_rows(yr, conv_tile_rows(yr.shape[0]))   # from the reference, before the kernel's result is looked at
    k.call("dpc_conv_igemm", C.byref(d), src, wp, out, None, stats)
    check_kernel(k, expect)
    k.sync()
    assert relerr(out, cl(y)) < tol(dtype)
    if taps > 1:
        wm = w.clone()
        wm[:, :, ks[0] // 2, ks[1] // 2, ks[2] // 2] = 0   # the centre tap gone (the one tap every output position sees)
        rejects_dropped_tap(out, cl(y), cl(F.conv3d(x, wm, None, st, pd)), tol(dtype))
    o = out.float().cpu().reshape(-1, Co).double()   # batch-norm partial sums are those of the STORED values
    all_finite(stats)
    s = stats.cpu().double()
    rejects_dropped_row(s[:, 0].sum(0), o, mut, "conv_fwd sum o")
    rejects_dropped_row(s[:, 1].sum(0), o * o, mut, "conv_fwd sum o^2")
    # the bounds these replace, kept: a quarter of a row is not below them for every shape
    assert (s[:, 0].sum(0) - o.sum(0)).abs().max().item() < 1e-3 * max(1.0, o.abs().sum(0).max().item())
    assert (s[:, 1].sum(0) - (o * o).sum(0)).abs().max().item() < 1e-4 * (o * o).sum(0).max().item()


def case_conv_dgrad(k: K, dtype, N, Ci, Co, T, H, W, ks, st, pd, seed=1, expect=None, with_add=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Ci, T, H, W, generator=g).requires_grad_()
    w = q(torch.randn(Co, Ci, *ks, generator=g) * 0.1, dtype)
    y = F.conv3d(x, w, None, st, pd)
    gy = q(torch.randn(y.shape, generator=g), dtype)
    gx = torch.autograd.grad(y, x, gy)[0]
    To, Ho, Wo = y.shape[2:]
    taps = ks[0] * ks[1] * ks[2]
    d = conv_desc(dtype, dtype, 1, N, (T, H, W), (To, Ho, Wo), Co, Co, Ci, taps * Co, Ci, ks, st, pd)
    add = q(torch.randn(N, T, H, W, Ci, generator=g), dtype)
    out = k.empty(N, T, H, W, Ci, dtype=dtype)
    wd = k.t(w.permute(1, 2, 3, 4, 0).reshape(Ci, taps * Co), dtype)
    k.call("dpc_conv_igemm", C.byref(d), k.t(cl(gy), dtype), wd, out, k.t(add, dtype) if with_add else None, None)
    check_kernel(k, expect)
    k.sync()
    want = cl(gx) + add if with_add else cl(gx)
    assert relerr(out, want) < tol(dtype)
    if taps > 1:
        wm = w.clone()
        wm[:, :, ks[0] // 2, ks[1] // 2, ks[2] // 2] = 0   # centre tap: a corner tap of a strided, padded conv may never touch the input
        gxm = cl(torch.autograd.grad(F.conv3d(x, wm, None, st, pd), x, gy)[0])
        rejects_dropped_tap(out, want, gxm + add if with_add else gxm, tol(dtype))


def case_conv_dgrad_alias(k: K, dtype, N, Ci, Co, T, H, W, ks, st, pd, seed=31, expect=None, gate=False):
    """the API's aliasing contract (include/dpc_hip.h): addend == out gives bit for bit what a separate addend buffer gives --
    through dpc_conv_igemm, and through dpc_conv_igemm_ex with the addend gated by a ReLU mask (the engine's in-place dx of a
    block's first conv, dpc_amd/engine.py _Block.backward)"""
    g = torch.Generator().manual_seed(seed)
    E = 8 if dtype == torch.bfloat16 else 4
    w = q(torch.randn(Co, Ci, *ks, generator=g) * 0.1, dtype)
    y_shape = F.conv3d(torch.zeros(N, Ci, T, H, W), w, None, st, pd).shape
    To, Ho, Wo = y_shape[2:]
    taps = ks[0] * ks[1] * ks[2]
    gy = k.t(cl(q(torch.randn(y_shape, generator=g), dtype)), dtype)
    d = conv_desc(dtype, dtype, 1, N, (T, H, W), (To, Ho, Wo), Co, Co, Ci, taps * Co, Ci, ks, st, pd)
    wd = k.t(w.permute(1, 2, 3, 4, 0).reshape(Ci, taps * Co), dtype)
    add = q(torch.randn(N, T, H, W, Ci, generator=g), dtype)
    mask = None
    if gate:
        mask = k.t(bits_of(torch.randn(N * T * H * W, Ci, generator=g), E).to(torch.uint8))

    def run(out, addend):
        if not gate:
            k.call("dpc_conv_igemm", C.byref(d), gy, wd, out, addend, None)
        else:
            ep = L.ConvEpilogue()
            ep.addend, ep.addend_mask = addend.data_ptr(), mask.data_ptr()
            k.call("dpc_conv_igemm_ex", C.byref(d), gy, wd, out, C.byref(ep))
        check_kernel(k, expect)
        k.sync()

    sep = k.empty(N, T, H, W, Ci, dtype=dtype)
    run(sep, k.t(add, dtype))
    inplace = k.t(add, dtype)
    run(inplace, inplace)
    assert torch.equal(sep.cpu(), inplace.cpu()), "addend aliased to out differs from the out-of-place result"


def case_conv_dgrad_ex(k: K, dtype, N, Ci, Co, T, H, W, ks, st, pd, gate=True, bnred=True, bn_relu=True, seed=7, expect=None, with_add=True):
    """dpc_conv_igemm_ex: input-gradient + (ReLU-gated residual addend) + (BatchNorm-backward partial sums of the unit whose
    output gradient it produces) in one launch == autograd's input-gradient, the addend masked by the sign mask, and the sums
    dpc_bn_bwd_reduce takes from the stored result (torch expectations, f64 sums)"""
    g = torch.Generator().manual_seed(seed)
    E = 8 if dtype == torch.bfloat16 else 4
    x = torch.randn(N, Ci, T, H, W, generator=g).requires_grad_()
    w = q(torch.randn(Co, Ci, *ks, generator=g) * 0.1, dtype)
    y = F.conv3d(x, w, None, st, pd)
    gy = q(torch.randn(y.shape, generator=g), dtype)
    gx = cl(torch.autograd.grad(y, x, gy)[0])                      # [N,T,H,W,Ci]
    To, Ho, Wo = y.shape[2:]
    taps = ks[0] * ks[1] * ks[2]
    d = conv_desc(dtype, dtype, 1, N, (T, H, W), (To, Ho, Wo), Co, Co, Ci, taps * Co, Ci, ks, st, pd)
    rows = N * T * H * W
    add = q(torch.randn(N, T, H, W, Ci, generator=g), dtype)
    act_out = q(torch.randn(rows, Ci, generator=g), dtype)          # the block output whose sign gates the addend
    raw = q(torch.randn(rows, Ci, generator=g) * 1.5 + 0.3, dtype)  # raw conv output of the unit being differentiated
    act_in = q(torch.randn(rows, Ci, generator=g), dtype)           # its activation (sign mask of the ReLU that follows it)
    mean, invstd = torch.randn(Ci, generator=g) * 0.2, torch.rand(Ci, generator=g) + 0.5
    amask, bmask = bits_of(act_out, E).to(torch.uint8), bits_of(act_in, E).to(torch.uint8)
    gate = gate and with_add
    want = gx + (add * (act_out.reshape(add.shape) > 0).float() if gate else add) if with_add else gx
    e = L.ConvEpilogue()
    keep = [k.t(add, dtype), k.t(amask), k.t(raw, dtype), k.t(bmask), k.t(mean), k.t(invstd)]
    nrows = k.lib.call("dpc_conv_stats_rows", C.byref(d))
    stats = k.poison(nrows, 2, Ci)
    e.addend, e.addend_mask = (keep[0].data_ptr() if with_add else None), (keep[1].data_ptr() if gate else None)
    if bnred:
        e.bn_raw, e.bn_mask, e.bn_mean, e.bn_invstd = keep[2].data_ptr(), (keep[3].data_ptr() if bn_relu else None), keep[4].data_ptr(), keep[5].data_ptr()
        e.stats = stats.data_ptr()
    out = k.empty(N, T, H, W, Ci, dtype=dtype)
    wd = k.t(w.permute(1, 2, 3, 4, 0).reshape(Ci, taps * Co), dtype)
    k.call("dpc_conv_igemm_ex", C.byref(d), k.t(cl(gy), dtype), wd, out, C.byref(e))
    check_kernel(k, expect)
    k.sync()
    assert relerr(out, want) < tol(dtype)
    if bnred:
        o = out.float().cpu().reshape(rows, Ci).double()            # sums are those of the STORED gradient
        dz = o * (act_in > 0).double() if bn_relu else o
        xh = (raw.double() - mean.double()) * invstd.double()
        all_finite(stats)
        sgot = stats.cpu().double()
        wr = want.reshape(rows, Ci).double()                          # the rows to remove: chosen from the expectation alone
        mut = mutation_rows(wr * (act_in > 0).double() if bn_relu else wr, conv_tile_rows(rows))
        rejects_dropped_row(sgot[:, 0].sum(0), dz, mut, "dgrad_ex sum dz")
        rejects_dropped_row(sgot[:, 1].sum(0), dz * xh, mut, "dgrad_ex sum dz*xhat")
        for got, exp in ((sgot[:, 0].sum(0), dz.sum(0)), (sgot[:, 1].sum(0), (dz * xh).sum(0))):   # the earlier bound, kept beside
            assert (got - exp).abs().max().item() < 2e-4 * max(1.0, dz.abs().sum(0).max().item())


def case_conv_dgrad_inplace(k: K, dtype, N, Ci, Co, T, H, W, ks, st, pd, seed=5, expect=None):
    """input-gradient accumulated IN PLACE (addend == out): the engine adds a strided 1x1 downsample's gradient onto the
    main path's dx; positions no tap reaches must keep their value exactly"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Ci, T, H, W, generator=g).requires_grad_()
    w = q(torch.randn(Co, Ci, *ks, generator=g) * 0.1, dtype)
    y = F.conv3d(x, w, None, st, pd)
    gy = q(torch.randn(y.shape, generator=g), dtype)
    gx = torch.autograd.grad(y, x, gy)[0]
    To, Ho, Wo = y.shape[2:]
    taps = ks[0] * ks[1] * ks[2]
    d = conv_desc(dtype, dtype, 1, N, (T, H, W), (To, Ho, Wo), Co, Co, Ci, taps * Co, Ci, ks, st, pd)
    base = q(torch.randn(N, T, H, W, Ci, generator=g), dtype)
    out = k.t(base.clone(), dtype)
    wd = k.t(w.permute(1, 2, 3, 4, 0).reshape(Ci, taps * Co), dtype)
    k.call("dpc_conv_igemm", C.byref(d), k.t(cl(gy), dtype), wd, out, out, None)
    check_kernel(k, expect)
    k.sync()
    assert relerr(out, cl(gx) + base) < tol(dtype)
    untouched = cl(gx) == 0
    assert torch.equal(out.cpu().float()[untouched], base[untouched])


def case_conv_wgrad(k: K, dtype, N, Ci, Co, T, H, W, ks, st, pd, seed=2, expect=None):
    g = torch.Generator().manual_seed(seed)
    x = q(torch.randn(N, Ci, T, H, W, generator=g), dtype)
    w = (torch.randn(Co, Ci, *ks, generator=g) * 0.1).requires_grad_()
    y = F.conv3d(x, w, None, st, pd)
    gy = q(torch.randn(y.shape, generator=g), dtype)
    gw = torch.autograd.grad(y, w, gy)[0]
    To, Ho, Wo = y.shape[2:]
    taps = ks[0] * ks[1] * ks[2]
    d = conv_desc(dtype, torch.float32, 0, N, (To, Ho, Wo), (T, H, W), Ci, Ci, Co, taps * Ci, Co, ks, st, pd)
    ns = C.c_int32(0)
    k.call("dpc_conv_wgrad", C.byref(d), None, None, Co, None, C.byref(ns))
    part = k.poison(ns.value, Co, taps * Ci)
    k.call("dpc_conv_wgrad", C.byref(d), k.t(cl(x), dtype), k.t(cl(gy), dtype), Co, part, C.byref(ns))
    check_kernel(k, expect)
    dw = k.poison(*gw.shape)
    k.call("dpc_reduce_unpack", part, ns.value, dw, Co, taps, Ci, Ci * taps, 1, taps, 0)
    k.sync()
    all_finite(part, dw)
    assert relerr(dw, gw) < 1e-4  # f32 accumulation in both modes
    if taps > 1:
        gm = gw.clone()
        gm[:, :, ks[0] // 2, ks[1] // 2, ks[2] // 2] = 0
        rejects_dropped_tap(dw, gw, gm, 1e-4)
    return ns.value   # slabs the planner chose (tests/switch_cases.py holds the split-K switches to it)


def case_gemm_nt(k: K, dtype, M, N, Kd, seed=3, expect=None):
    g = torch.Generator().manual_seed(seed)
    A = q(torch.randn(M, Kd, generator=g), dtype)
    B = q(torch.randn(N, Kd, generator=g), dtype)
    d = conv_desc(dtype, torch.float32, 0, M, (1, 1, 1), (1, 1, 1), Kd, Kd, N, Kd, N, (1, 1, 1), (1, 1, 1), (0, 0, 0))
    out = k.empty(M, N)
    k.call("dpc_conv_igemm", C.byref(d), k.t(A, dtype), k.t(B, dtype), out, None, None)
    check_kernel(k, expect)
    k.sync()
    assert relerr(out, A.double() @ B.double().t()) < 1e-5


def case_reduce_unpack(k: K, ns, d0, d1, d2, permute, accumulate, expect=None, seed=5):
    """dpc_reduce_unpack: out[i0, i1, i2] (+)= sum over ns slabs of part[s][i0][i1][i2], written through arbitrary strides
    (permute = the conv-parameter layout [d0][d2][d1]); the few-slab / many-slab / transposing kernels"""
    g = torch.Generator().manual_seed(seed)
    part = torch.randn(ns, d0, d1, d2, generator=g)
    base = torch.randn(d0, d1, d2, generator=g)
    want = part.double().sum(0) + (base.double() if accumulate else 0)
    start = base if accumulate else torch.full_like(base, float("nan"))   # without accumulate the destination is a pure output
    if permute:
        out = k.t(start.permute(0, 2, 1).contiguous())
        s0, s1, s2 = d1 * d2, 1, d1
    else:
        out = k.t(start.clone())
        s0, s1, s2 = d1 * d2, d2, 1
    k.call("dpc_reduce_unpack", k.t(part), ns, out, d0, d1, d2, s0, s1, s2, int(accumulate))
    check_kernel(k, expect)
    k.sync()
    all_finite(out)
    got = out.cpu()
    got = got.permute(0, 2, 1) if permute else got
    assert relerr(got, want) < 1e-6


def case_gemm_nt_splitk(k: K, dtype, M, N, Kd, pad=0, seed=13, expect=None):
    """dpc_gemm_nt_splitk: f32 partial slabs of A @ B^T over K ranges, summed by dpc_reduce_unpack (d_pred = dS @ feature_inf);
    leading dimensions Kd + pad, the padding columns hold garbage that must not be read"""
    g = torch.Generator().manual_seed(seed)
    A = q(torch.randn(M, Kd, generator=g), dtype)
    B = q(torch.randn(N, Kd, generator=g), dtype)
    Ap = torch.full((M, Kd + pad), 77.0).to(dtype); Ap[:, :Kd] = A.to(dtype)
    Bp = torch.full((N, Kd + pad), -55.0).to(dtype); Bp[:, :Kd] = B.to(dtype)
    ns = C.c_int32(0)
    k.call("dpc_gemm_nt_splitk", L.dtype_code(dtype), M, N, Kd, None, Kd + pad, None, Kd + pad, None, C.byref(ns))
    part = k.poison(ns.value, M, N)
    k.call("dpc_gemm_nt_splitk", L.dtype_code(dtype), M, N, Kd, k.t(Ap), Kd + pad, k.t(Bp), Kd + pad, part, C.byref(ns))
    check_kernel(k, expect)
    out = k.poison(M, N)
    k.call("dpc_reduce_unpack", part, ns.value, out, M, 1, N, N, 0, 1, 0)
    k.sync()
    all_finite(part, out)
    assert relerr(out, A.double() @ B.double().t()) < 1e-5
    return ns.value


def case_gemm_tn_splitk(k: K, M, N, Kd, pad=0, seed=17, expect="gemm_ws_kernel<true>"):
    """dpc_gemm_tn_splitk: out[m][n] = sum_k A[k][m] * B[n][k], A K-major with leading dimension M + pad (d_feature_inf = dS^T @ pred:
    A = dS [R][ld], B = pred^T [D][ld]); padding columns of both operands hold garbage that must not be read"""
    g = torch.Generator().manual_seed(seed)
    dtype = torch.bfloat16
    A = q(torch.randn(Kd, M, generator=g), dtype)
    B = q(torch.randn(N, Kd, generator=g), dtype)
    Ap = torch.full((Kd, M + pad), 77.0).to(dtype); Ap[:, :M] = A.to(dtype)
    Bp = torch.full((N, Kd + pad), -55.0).to(dtype); Bp[:, :Kd] = B.to(dtype)
    ns = C.c_int32(0)
    k.call("dpc_gemm_tn_splitk", L.dtype_code(dtype), M, N, Kd, None, M + pad, None, Kd + pad, None, C.byref(ns))
    part = k.poison(ns.value, M, N)
    k.call("dpc_gemm_tn_splitk", L.dtype_code(dtype), M, N, Kd, k.t(Ap), M + pad, k.t(Bp), Kd + pad, part, C.byref(ns))
    check_kernel(k, expect)
    out = k.poison(M, N)
    k.call("dpc_reduce_unpack", part, ns.value, out, M, 1, N, N, 0, 1, 0)
    k.sync()
    all_finite(part, out)
    assert relerr(out, A.double().t() @ B.double().t()) < 1e-5
    return ns.value


def case_stem(k: K, dtype, BN, T, H, W, Co=64, seed=4, expect=(None, None)):
    """Conv3d(3,Co,(1,7,7),s(1,2,2),p(0,3,3)) (resnet_2d3d.py:211) through the space-to-depth path."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(BN, 3, T, H, W, generator=g)
    w = (torch.randn(Co, 3, 1, 7, 7, generator=g) * 0.1)
    wq = q(w, dtype).double().requires_grad_()  # f64 expectation: the f32 reference's own noise exceeds 1e-4 at full size
    y = F.conv3d(q(x, dtype).double(), wq, None, (1, 2, 2), (0, 3, 3))
    xs = k.empty(BN, T, H // 2, W // 2, 16, dtype=dtype)
    k.call("dpc_pack_input_s2d", k.t(x), xs, L.dtype_code(dtype), BN, T, H, W)
    wp = k.empty(Co, 16, 16, dtype=dtype)
    k.call("dpc_pack_stem_weight", k.t(w), wp, L.dtype_code(dtype), Co)
    d = conv_desc(dtype, dtype, 0, BN, (T, H // 2, W // 2), (T, H // 2, W // 2), 16, 16, Co, 256, Co, (1, 4, 4), (1, 1, 1), (0, 2, 2))
    out = k.empty(BN, T, H // 2, W // 2, Co, dtype=dtype)
    rows = k.lib.call("dpc_conv_stats_rows", C.byref(d))
    stats = k.poison(rows, 2, Co)
    yr = cl(y.detach()).reshape(-1, Co)
    mut = mutation_rows(yr, conv_tile_rows(yr.shape[0]))
    k.call("dpc_conv_igemm", C.byref(d), xs, wp, out, None, stats)
    check_kernel(k, expect[0])
    k.sync()
    assert relerr(out, cl(y)) < tol(dtype)
    o = out.float().cpu().reshape(-1, Co).double()  # batch-norm partial sums are those of the STORED values
    all_finite(stats)
    st = stats.cpu().double()
    rejects_dropped_row(st[:, 0].sum(0), o, mut, "stem sum o")
    rejects_dropped_row(st[:, 1].sum(0), o * o, mut, "stem sum o^2")
    assert (st[:, 0].sum(0) - o.sum(0)).abs().max().item() < 1e-3 * max(1.0, o.abs().sum(0).max().item())
    assert (st[:, 1].sum(0) - (o * o).sum(0)).abs().max().item() < 1e-4 * (o * o).sum(0).max().item()
    gy = q(torch.randn(y.shape, generator=g), dtype)
    gw = torch.autograd.grad(y, wq, gy.double())[0]
    ns = C.c_int32(0)
    k.call("dpc_conv_wgrad", C.byref(d), None, None, Co, None, C.byref(ns))
    part = k.poison(ns.value, Co, 256)
    k.call("dpc_conv_wgrad", C.byref(d), xs, k.t(cl(gy), dtype), Co, part, C.byref(ns))
    check_kernel(k, expect[1])
    dw = k.poison(Co, 3, 1, 7, 7)
    k.call("dpc_unpack_stem_wgrad", part, ns.value, dw, Co)
    k.sync()
    all_finite(part, dw)
    assert relerr(dw, gw) < 1e-4
    return ns.value


# ------------------------------------------------------------------ batch norm
def _bn_ref(x, gamma, beta, res, rs, rb, relu):
    """x [rows,C] f64: returns y, mean, invstd"""
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    y = (x - mean) * invstd * gamma + beta
    if res is not None:
        y = y + (res * rs + rb if rs is not None else res)
    if relu:
        y = F.relu(y)
    return y, mean, invstd


def case_bn_fwd_bwd(k: K, dtype, rows, Cc, relu, res_mode, seed=5):
    """res_mode: 0 none, 1 identity residual, 2 residual with its own scale/shift (downsample BN)"""
    g = torch.Generator().manual_seed(seed)
    x = q(torch.randn(rows, Cc, generator=g) * 2 + 0.5, dtype)
    gamma = torch.rand(Cc, generator=g) + 0.5
    beta = torch.randn(Cc, generator=g) * 0.3
    res = q(torch.randn(rows, Cc, generator=g), dtype) if res_mode else None
    rs = torch.rand(Cc, generator=g) + 0.5 if res_mode == 2 else None
    rb = torch.randn(Cc, generator=g) if res_mode == 2 else None
    xd = x.double().requires_grad_()
    gd = gamma.double().requires_grad_()
    bd = beta.double().requires_grad_()
    y, mean, invstd = _bn_ref(xd, gd, bd, None if res is None else res.double(),
                              None if rs is None else rs.double(), None if rb is None else rb.double(), relu)
    # partial sums as the conv epilogue would deliver them (3 rows of partials)
    parts = torch.zeros(3, 2, Cc)
    for i, ch in enumerate(torch.chunk(x, 3, 0)):
        parts[i, 0] = ch.sum(0)
        parts[i, 1] = (ch * ch).sum(0)
    dm, di, dsc, dsh = (k.empty(Cc) for _ in range(4))
    k.call("dpc_bn_finalize", k.t(parts), 3, Cc, float(rows), k.t(gamma), k.t(beta), 1e-5,
           dm, di, dsc, dsh)
    k.sync()
    assert relerr(dm, mean.detach()) < 1e-5 and relerr(di, invstd.detach()) < 1e-4
    xk = k.t(x, dtype)
    yk = k.empty(rows, Cc, dtype=dtype)
    E = 4 if dtype == torch.float32 else 8
    mk = k.zeros(rows * Cc // E, dtype=torch.uint8)  # ReLU sign mask, one byte per 16-byte unit (uint8: there is no NaN to poison it with)
    k.call("dpc_bn_apply", xk, yk, L.dtype_code(dtype), rows, Cc, dsc, dsh,
           None if res is None else k.t(res, dtype), None if rs is None else k.t(rs),
           None if rb is None else k.t(rb), int(relu), mk)
    k.sync()
    assert relerr(yk, y.detach()) < tol(dtype)
    bits = (yk.float().cpu().reshape(-1, E) > 0).to(torch.int32) * (1 << torch.arange(E, dtype=torch.int32))
    assert torch.equal(mk.cpu().to(torch.int32), bits.sum(1))
    # backward
    gy = q(torch.randn(rows, Cc, generator=g), dtype)
    y.backward(gy.double())
    yq = k.t(y.detach().float(), dtype)  # saved post-activation output (mask source)
    gyk = k.t(gy, dtype)
    prow = C.c_int32(0)
    k.call("dpc_bn_bwd_reduce", None, None, None, None, L.dtype_code(dtype), rows, Cc, None, None, int(relu), None, C.byref(prow))
    # the ReLU pattern comes either from the saved output y or from the byte mask of the kernel's own forward
    mq = k.t((bits_of(yq, E)).to(torch.uint8))
    dz_ref = gy.double() * ((y.detach() > 0).double() if relu else 1.0)
    xh_ref = ((xd - mean) * invstd).detach()                     # x-hat in f64 from the f64 mean and invstd
    mut = mutation_rows(dz_ref)
    for ysrc, msrc in ((yq, None), (None, mq)) if relu else ((None, None),):
        bp = k.poison(prow.value, 2, Cc)
        k.call("dpc_bn_bwd_reduce", gyk, ysrc, msrc, xk, L.dtype_code(dtype), rows, Cc, dm, di,
               int(relu), bp, C.byref(prow))
        dgam, dbet, coef = k.empty(Cc), k.empty(Cc), k.empty(2, Cc)
        k.call("dpc_bn_bwd_finalize", bp, prow.value, Cc, float(rows), dgam, dbet, coef)
        dx = k.empty(rows, Cc, dtype=dtype)
        dz = k.empty(rows, Cc, dtype=dtype)
        k.call("dpc_bn_bwd_apply", gyk, ysrc, msrc, xk, L.dtype_code(dtype), rows, Cc, dm, di,
               k.t(gamma), coef, int(relu), dx, dz)
        k.sync()
        all_finite(bp)
        src = "y" if ysrc is not None else ("mask" if msrc is not None else "none")
        # relu-mask flips of y~0 elements are excluded by construction: the kernel reads the sign of the expectation's own y.
        # dgamma / dbeta are f32 sums of operands the expectation sees bit for bit, in both dtypes
        rejects_dropped_row(dbet, dz_ref, mut, f"bn_bwd dbeta (mask source {src})")
        rejects_dropped_row(dgam, dz_ref * xh_ref, mut, f"bn_bwd dgamma (mask source {src})")
        t = 2e-3  # the earlier f32 bound against autograd, now for both dtypes (it was 3e-2 in bf16)
        assert relerr(dgam, gd.grad) < t and relerr(dbet, bd.grad) < t
        e_dx = relerr(dx, xd.grad)
        print(f"[dx] bn_bwd_apply {dtype} rows {rows} C {Cc} mask source {src}: relerr {e_dx:.3g}")
        assert e_dx < (DX_F32_BOUND if dtype == torch.float32 else tol(dtype))
        assert relerr(dz, dz_ref) < tol(dtype)


def case_bn_finalize(k: K, rows, Cc, misalign=0, seed=11):
    """dpc_bn_finalize / dpc_bn_bwd_finalize on a table of `rows` partial rows: f64 column sums (the unrolled four-row trips, the row tail,
    channel counts that are no multiple of four, a table that is not 16-byte aligned)"""
    g = torch.Generator().manual_seed(seed)
    parts = torch.randn(rows, 2, Cc, generator=g)
    parts[:, 1] = parts[:, 1].abs() * 3 + parts[:, 0] ** 2          # sum of squares >= (sum)^2 / n per row
    count = float(rows * 7)
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g)
    buf = k.zeros(rows * 2 * Cc + 4)   # real input: the table the finalize kernels READ (filled below)
    pk = buf[misalign:misalign + rows * 2 * Cc].view(rows, 2, Cc)
    pk.copy_(parts)
    s1, s2 = parts[:, 0].double().sum(0), parts[:, 1].double().sum(0)
    m = s1 / count
    var = (s2 / count - m * m).clamp_min(0)
    inv = 1.0 / torch.sqrt(var + 1e-5)
    dm, di, dsc, dsh = (k.empty(Cc) for _ in range(4))
    k.call("dpc_bn_finalize", pk, rows, Cc, count, k.t(gamma), k.t(beta), 1e-5, dm, di, dsc, dsh)
    dgam, dbet, coef = k.empty(Cc), k.empty(Cc), k.empty(2, Cc)
    k.call("dpc_bn_bwd_finalize", pk, rows, Cc, count, dgam, dbet, coef)
    k.sync()
    f = lambda t: t.float().cpu()  # noqa: E731
    assert torch.allclose(f(dm), m.float(), rtol=1e-6, atol=1e-7) and torch.allclose(f(di), inv.float(), rtol=1e-6)
    sc = gamma * inv.float()
    assert torch.allclose(f(dsc), sc, rtol=1e-6) and torch.allclose(f(dsh), beta - m.float() * sc, rtol=1e-5, atol=1e-6)
    assert torch.allclose(f(dbet), s1.float(), rtol=1e-6, atol=1e-6) and torch.allclose(f(dgam), s2.float(), rtol=1e-6)
    assert torch.allclose(f(coef[0]), (s1 / count).float(), rtol=1e-6, atol=1e-7) and torch.allclose(f(coef[1]), (s2 / count).float(), rtol=1e-6)


def case_stem_pool(k: K, dtype, NT, H, W, Cc, seed=6):
    """relu(bn(x)) -> MaxPool3d((1,3,3),(1,2,2),(0,1,1)) and its backward (resnet_2d3d.py:212-214)"""
    g = torch.Generator().manual_seed(seed)
    x = q(torch.randn(NT, H, W, Cc, generator=g), dtype)
    sc = torch.rand(Cc, generator=g) + 0.5
    sh = torch.randn(Cc, generator=g) * 0.2
    a = (x * sc + sh).permute(0, 3, 1, 2).unsqueeze(2).requires_grad_()  # [NT,C,1,H,W]
    y = F.max_pool3d(F.relu(a), (1, 3, 3), (1, 2, 2), (0, 1, 1))
    Ho, Wo = y.shape[3:]
    yk = k.empty(NT, Ho, Wo, Cc, dtype=dtype)
    am = torch.empty(NT, Ho, Wo, Cc, dtype=torch.uint8, device=k.dev)
    k.call("dpc_bn_relu_maxpool_fwd", k.t(x, dtype), L.dtype_code(dtype), NT, H, W, Cc, k.t(sc), k.t(sh),
           yk, am)
    k.sync()
    yref = y.detach().squeeze(2).permute(0, 2, 3, 1)
    assert relerr(yk, yref) < tol(dtype)
    gy = q(torch.randn(NT, Ho, Wo, Cc, generator=g), dtype)
    y.backward(gy.permute(0, 3, 1, 2).unsqueeze(2))
    dz = k.empty(NT, H, W, Cc, dtype=dtype)
    k.call("dpc_maxpool_bwd", k.t(gy, dtype), am, L.dtype_code(dtype), NT, H, W, Cc, dz)
    k.sync()
    dz_ref = a.grad.squeeze(2).permute(0, 2, 3, 1)
    assert relerr(dz, dz_ref) < tol(dtype)
    # fused form used by the engine: BN backward with the pooled gradient routed on the fly
    gamma = torch.rand(Cc, generator=g) + 0.5
    xd = x.double().requires_grad_()
    mean = xd.mean((0, 1, 2)); var = xd.var((0, 1, 2), unbiased=False); invstd = 1 / torch.sqrt(var + 1e-5)
    yb = (xd - mean) * invstd * gamma.double()
    yb.backward(dz_ref.double())
    rows = NT * H * W
    prow = C.c_int32(0)
    k.call("dpc_pool_bn_bwd_reduce", None, None, None, L.dtype_code(dtype), NT, H, W, Cc, None, None, None, C.byref(prow))
    bp = k.poison(prow.value, 2, Cc)
    xk, gyk = k.t(x, dtype), k.t(gy, dtype)
    km, ki = k.t(mean.detach().float()), k.t(invstd.detach().float())
    k.call("dpc_pool_bn_bwd_reduce", gyk, am, xk, L.dtype_code(dtype), NT, H, W, Cc, km, ki, bp, C.byref(prow))
    dgam, dbet, coef = k.empty(Cc), k.empty(Cc), k.empty(2, Cc)
    k.call("dpc_bn_bwd_finalize", bp, prow.value, Cc, float(rows), dgam, dbet, coef)
    dx = k.empty(NT, H, W, Cc, dtype=dtype)
    k.call("dpc_pool_bn_bwd_apply", gyk, am, xk, L.dtype_code(dtype), NT, H, W, Cc, km, ki, k.t(gamma), coef, dx)
    k.sync()
    all_finite(bp)
    dzr = dz_ref.double().reshape(rows, Cc)                     # the routed pooled gradient, one row per input position
    xhr = ((xd - mean) * invstd).detach().reshape(rows, Cc)
    mut = mutation_rows(dzr)
    rejects_dropped_row(dbet, dzr, mut, "pool_bn_bwd dbeta")
    rejects_dropped_row(dgam, dzr * xhr, mut, "pool_bn_bwd dgamma")
    t = 2e-3
    e_dx = relerr(dx, xd.grad)
    print(f"[dx] pool_bn_bwd_apply {dtype} NT {NT} H {H} W {W} C {Cc}: relerr {e_dx:.3g}")
    assert e_dx < (DX_F32_BOUND if dtype == torch.float32 else tol(dtype)) and relerr(dbet, dz_ref.double().sum((0, 1, 2))) < t
    # pooled-tensor form of the same partial sums (y at an argmax position is the pooled value): feed it the
    # scale/shift the forward used as gamma*invstd / beta-mean*scale, i.e. gamma'=sc, beta'=sh, xhat'=x
    prow2 = C.c_int32(0)
    rows_p = NT * Ho * Wo
    k.call("dpc_pooled_bn_bwd_reduce", None, None, None, L.dtype_code(dtype), rows_p, Cc, None, None, None, C.byref(prow2))
    bp2 = k.poison(prow2.value, 2, Cc)
    k.call("dpc_pooled_bn_bwd_reduce", gyk, am, yk, L.dtype_code(dtype), rows_p, Cc, k.t(sc), k.t(sh), bp2, C.byref(prow2))
    k.sync()
    all_finite(bp2)
    s_dz = bp2.cpu().double().sum(0)
    ref1 = dz_ref.double().sum((0, 1, 2))
    ref2 = (dz_ref.double() * x.double()).sum((0, 1, 2))   # with gamma'=sc, beta'=sh the recovered "xhat" is x itself
    # s_dz[0]: the kernel walks the POOLED rows; every pooled element routes to exactly one input position, so the sum over input
    # positions of the routed gradient is the same sum, and a pooled row is what it can lose
    gyr = gy.double().reshape(rows_p, Cc) * (y.detach().squeeze(2).permute(0, 2, 3, 1).reshape(rows_p, Cc) > 0).double()
    # (the two expectations agree: autograd adds the gradients of overlapping windows that share an argmax in f32)
    assert (gyr.sum(0) - ref1).abs().max().item() < 1e-6 * gyr.abs().sum(0).max().item()
    rejects_dropped_row(s_dz[0], gyr, mutation_rows(gyr), "pooled_bn_bwd sum dz")
    assert (s_dz[0] - ref1).abs().max().item() < t * max(ref1.abs().max().item(), 1.0)
    # s_dz[1]: the f32 form keeps the 2e-3 bound; the bf16 form recovers x-hat from a bf16-ROUNDED pooled value (2^-9 relative per
    # term, not a summation error), which no row-sized bound covers: it keeps its 6e-2
    assert (s_dz[1] - ref2).abs().max().item() < (t if dtype == torch.float32 else 6e-2) * max(ref2.abs().max().item(), 1.0)


def case_tpool_split(k: K, dtype, B, N, T, SQ, D, P, seed=7):
    g = torch.Generator().manual_seed(seed)
    x = q(torch.randn(B * N, T, SQ, D, generator=g), dtype).requires_grad_()
    m = x.mean(1).view(B, N, SQ, D)
    fr_ref = F.relu(m).permute(1, 0, 2, 3).reshape(N, B * SQ, D)
    fi_ref = m[:, N - P:]
    fr = k.empty(N, B * SQ, D, dtype=dtype)
    fi = k.empty(B, P, SQ, D, dtype=dtype)
    xk = k.t(x.detach(), dtype)
    k.call("dpc_tpool_split_fwd", xk, L.dtype_code(dtype), B, N, T, SQ, D, P, fr, fi)
    k.sync()
    assert relerr(fr, fr_ref.detach()) < tol(dtype) and relerr(fi, fi_ref.detach()) < tol(dtype)
    d_relu = torch.randn(N - P, B * SQ, D, generator=g)
    d_inf = torch.randn(B, P, SQ, D, generator=g)
    loss = (fr_ref[: N - P] * d_relu).sum() + (fi_ref * d_inf).sum()
    gx = torch.autograd.grad(loss, x)[0]
    dx = k.empty(B * N, T, SQ, D, dtype=dtype)
    k.call("dpc_tpool_split_bwd", xk, k.t(d_relu), k.t(d_inf), L.dtype_code(dtype), B, N, T, SQ, D, P, dx)
    k.sync()
    assert relerr(dx, gx) < tol(dtype)


# ------------------------------------------------------------------ ConvGRU cell pieces
def case_mask(k: K, B, P, SQ):
    from oracle import dpc_oracle as O
    m = torch.empty(B, P, SQ, B, P, SQ, dtype=torch.int8, device=k.dev)
    k.call("dpc_mask_gen", m, B, P, SQ)
    k.sync()
    assert torch.equal(m.cpu(), O.mask_closed_form(B, P, SQ))  # bit exact


def case_ce_topk(k: K, rows, cols, dtype_d, seed=10):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(rows, cols, generator=g) * 3
    idx = torch.arange(0, rows, 3)
    s[idx, idx] += 6.0
    sd = s.double().requires_grad_()
    tgt = torch.arange(rows)
    loss = F.cross_entropy(sd, tgt)
    loss.backward()
    _, pred = s.topk(5, 1, True, True)
    correct = pred.t().eq(tgt.view(1, -1))
    accs = [correct[:kk].reshape(-1).float().sum().item() / rows for kk in (1, 3, 5)]
    ld_d = (cols + 7) // 8 * 8
    ws, res = k.empty(rows, 2), k.empty(4)
    ds = k.empty(rows, ld_d, dtype=dtype_d)
    k.call("dpc_ce_topk", k.t(s), rows, cols, cols, ws, res, ds, L.dtype_code(dtype_d), ld_d)
    k.sync()
    r = res.cpu()
    assert abs(r[0].item() - loss.item()) < 1e-5 * max(1.0, abs(loss.item()))
    assert [round(v, 6) for v in r[1:].tolist()] == [round(v, 6) for v in accs]
    assert relerr(ds[:, :cols], sd.grad) < tol(dtype_d)
    assert row_offdiag_relerr(ds[:, :cols], sd.grad) < tol(dtype_d)   # the same bound, per row (tests/loss_cases.py holds every element)
    assert torch.equal(ws[:, 1].cpu().double(), (s > s.diagonal()[:, None]).sum(1).double())   # random f32 data: no ties
    if ld_d > cols:
        assert ds[:, cols:].float().abs().max().item() == 0


def case_adam(k: K, n, seed=11):
    from oracle import dpc_oracle as O
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g) * 0.01
    m = torch.randn(n, generator=g) * 0.01
    v = torch.rand(n, generator=g) * 1e-4
    pk, mk, vk = k.t(p.clone()), k.t(m.clone()), k.t(v.clone())
    step = 3
    k.call("dpc_adam", pk, k.t(gr), mk, vk, n, 1e-3, 0.9, 0.999, 1e-8, 1e-5,
           1 - 0.9 ** step, 1 - 0.999 ** step, 1.0)
    k.sync()
    O.adam_step(p, gr, m, v, step)
    assert (pk.cpu() - p).abs().max().item() < 1e-6 and relerr(mk, m) < 1e-5 and relerr(vk, v) < 1e-5


def case_transpose(k: K, rows, cols, seed=12):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(rows, cols, generator=g)
    ld = (rows + 7) // 8 * 8
    o = k.zeros(cols, ld, dtype=torch.bfloat16)   # real input: a padded bf16 operand, its padding columns are zeros by contract
    k.call("dpc_transpose2d", k.t(a), 0, cols, o, 1, ld, rows, cols)
    k.sync()
    assert torch.equal(o[:, :rows].cpu(), a.t().bfloat16())


def case_transpose_x2(k: K, rows, cols, seed=21):
    """dpc_transpose2d_bf16x2: two bf16 matrices in one launch; padding columns of the outputs stay untouched (zero)"""
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(rows, cols, generator=g).bfloat16(), torch.randn(rows, cols, generator=g).bfloat16()
    ld = (rows + 7) // 8 * 8
    oa, ob = k.zeros(cols, ld, dtype=torch.bfloat16), k.zeros(cols, ld, dtype=torch.bfloat16)   # real input: padding asserted untouched below
    k.call("dpc_transpose2d_bf16x2", k.t(a), k.t(b), cols, oa, ob, ld, rows, cols)
    k.sync()
    assert torch.equal(oa[:, :rows].cpu(), a.t()) and torch.equal(ob[:, :rows].cpu(), b.t())
    assert not oa[:, rows:].any() and not ob[:, rows:].any()
    oc = k.zeros(cols, ld, dtype=torch.bfloat16)   # real input: padded bf16 operand
    k.call("dpc_transpose2d_bf16x2", k.t(b), None, cols, oc, None, ld, rows, cols)
    k.sync()
    assert torch.equal(oc[:, :rows].cpu(), b.t())


def case_pack3d_multi(k: K, dtype, shapes, seed=14):
    """dpc_pack3d_multi: every conv weight [Co][Ci][taps] f32 -> [Co][tap][Ci] and [Ci][tap][Co] in the compute dtype, one launch
    over a device-side table (the engine's per-step repack; tiled through LDS when the source is contiguous along the middle index)"""
    g = torch.Generator().manual_seed(seed)
    ents, keep, blk = [], [], 0
    for (Co, Ci, t) in shapes:
        w = k.t(torch.randn(Co, Ci, t, generator=g))
        wp, wd = k.poison(Co, t, Ci, dtype=dtype), k.poison(Ci, t, Co, dtype=dtype)   # pure outputs, compared bit for bit below
        for (dst, d0, d1, d2, s0, s1, s2) in ((wp, Co, t, Ci, Ci * t, 1, t), (wd, Ci, t, Co, t, 1, Ci * t)):
            ents.append(L.PackEntry(w.data_ptr(), dst.data_ptr(), d0, d1, d2, blk, s0, s1, s2))
            blk += max(1, min(1024, (d0 * d1 * d2 + 511) // 512))
        keep.append((w, wp, wd))
    tab = (L.PackEntry * len(ents))(*ents)
    tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).clone().to(k.dev)
    k.call("dpc_pack3d_multi", tab_dev, len(ents), blk, L.dtype_code(dtype))
    k.sync()
    for w, wp, wd in keep:
        assert torch.equal(wp.cpu(), w.cpu().permute(0, 2, 1).to(dtype))
        assert torch.equal(wd.cpu(), w.cpu().permute(1, 2, 0).to(dtype))


def case_copy2d_multi(k: K, seed=15):
    """dpc_copy2d_multi: a table of f32 [rows][cols] windows between different leading dimensions in one launch (the nine gate
    slices of the ConvGRU's parameter gradients); everything outside the windows stays untouched"""
    g = torch.Generator().manual_seed(seed)
    D = 24
    srcs = [k.t(torch.randn(3 * D, D, generator=g)), k.t(torch.randn(2 * D, D, generator=g)), k.t(torch.randn(3 * D, generator=g))]
    dsts = [k.t(torch.full((D, 2 * D), -7.0)) for _ in range(3)] + [k.t(torch.full((D,), -7.0)) for _ in range(3)]
    ents = []
    for i in range(3):
        ents.append((srcs[0][i * D:(i + 1) * D], D, dsts[i], 2 * D, D, D))                       # x half of gate i
        if i < 2:
            ents.append((srcs[1][i * D:(i + 1) * D], D, dsts[i][:, D:], 2 * D, D, D))            # h half
        ents.append((srcs[2][i * D:(i + 1) * D], D, dsts[3 + i], D, 1, D))                       # bias
    tab = (L.Copy2dEntry * len(ents))()
    blk = 0
    for i, (src, sld, dst, dld, r, c) in enumerate(ents):
        tab[i] = L.Copy2dEntry(src.data_ptr(), dst.data_ptr(), sld, dld, r, c, blk, 0)
        blk += 1 + (i % 2)
    tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).clone().to(k.dev)
    k.call("dpc_copy2d_multi", tab_dev, len(ents), blk)
    k.sync()
    for i in range(3):
        assert torch.equal(dsts[i][:, :D].cpu(), srcs[0][i * D:(i + 1) * D].cpu())
        if i < 2:
            assert torch.equal(dsts[i][:, D:].cpu(), srcs[1][i * D:(i + 1) * D].cpu())
        else:
            assert bool((dsts[i][:, D:] == -7.0).all())
        assert torch.equal(dsts[3 + i].cpu(), srcs[2][i * D:(i + 1) * D].cpu())


# ---------------------------------------------------------------- column sums (bias gradients of the ConvGRU / network_pred)
def case_colsum(k: K, dtype, M, D, ld, seed=71):
    """dpc_colsum (csrc/gru.hip): out[D] (+)= column sums of x[M][D] with leading dimension ld, through up to 64 row slices of a
    workspace, against f64 column sums (rejects_dropped_row).  Padding columns hold 77 and must not be read; the workspace is handed
    over poisoned and only its first slices * D floats may be touched; accumulate = 1 adds onto a random `out`; a workspace one
    float short of slices * D is an argument error that launches nothing."""
    import pytest
    g = torch.Generator().manual_seed(seed)
    x = q(torch.randn(M, D, generator=g), dtype)
    xp = torch.full((M, ld), 77.0).to(dtype)
    xp[:, :D] = x.to(dtype)
    base = torch.randn(D, generator=g)
    terms = x.double()
    mut = mutation_rows(terms)
    need = min((M + 255) // 256, 64) * D          # one workspace row per 256-row slice, 64 slices at the most
    xk = k.t(xp)
    for accumulate in (0, 1):
        ws = k.poison(need + 32)                   # 32 floats of guard behind what the call may use
        out = k.t(base.clone()) if accumulate else k.poison(D)
        k.call("dpc_colsum", xk, L.dtype_code(dtype), ld, M, D, out, accumulate, ws, need)
        k.sync()
        all_finite(ws[:need], out)
        assert bool(torch.isnan(ws[need:]).all()), "the workspace was written past the size the call was given"
        got = out.cpu().double() - (base.double() if accumulate else 0.0)
        rejects_dropped_row(got, terms, mut, f"colsum {dtype} ({M}, {D}, {ld}) accumulate={accumulate}")
    if need > 1:
        ws, out = k.poison(need), k.t(base.clone())
        with pytest.raises(L.DpcError, match=f"code {L.ERR_ARG}$"):
            k.call("dpc_colsum", xk, L.dtype_code(dtype), ld, M, D, out, 0, ws, need - 1)
        k.sync()
        assert bool(torch.isnan(ws).all()) and torch.equal(out.cpu(), base), "a rejected call launched something"


# ---------------------------------------------------------------- dropout masks (Philox4x32-10) / device-side Adam step
def philox4x32_10_np(ctr, key):
    """numpy Philox4x32-10 (Salmon et al., SC'11): ctr [n,4] uint32, key [2] uint32 -> [n,4] uint32.
    Pinned by the Random123 known-answer vectors in tests/test_kernels_emu.py::test_philox_known_answers."""
    import numpy as np
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    M0, M1, W0, W1, MASK = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, 1).astype(np.uint32)


def dropout_mask_np(n, p, seed, step, stream=0):
    import numpy as np
    nb = (n + 3) // 4
    ctr = np.zeros((nb, 4), np.uint32)
    ctr[:, 0] = np.arange(nb, dtype=np.uint32)
    ctr[:, 1] = step
    ctr[:, 2] = stream
    r = philox4x32_10_np(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(-1)[:n]
    thresh = int(p * 16777216.0 + 0.5)
    return ((r >> 8) >= thresh).astype(np.float32) / np.float32(1.0 - p)


def case_dropout_mask(k: K, n, p=0.1, seed=233, step=5):
    import numpy as np
    st = torch.tensor([step], dtype=torch.int32, device=k.dev)
    m = k.empty(n)
    k.call("dpc_dropout_mask", m, n, p, seed, st)
    k.sync()
    ref = dropout_mask_np(n, p, seed, step)
    assert np.array_equal(m.cpu().numpy(), ref)  # bit-exact
    if n >= 100000:
        assert abs(float((ref > 0).mean()) - (1 - p)) < 4 * (p * (1 - p) / n) ** 0.5
        other = dropout_mask_np(n, p, seed, step + 1)
        assert 0.15 < float((other != ref).mean()) < 0.21  # a new optimizer step draws new masks (2p(1-p) = 0.18)


def case_adam_dev(k: K, n, seed=13):
    from oracle import dpc_oracle as O
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    m = torch.zeros(n)
    v = torch.zeros(n)
    pk, mk, vk = k.t(p.clone()), k.t(m.clone()), k.t(v.clone())
    st = torch.zeros(1, dtype=torch.int32, device=k.dev)
    bc = k.empty(2)
    for step in (1, 2, 3):
        gr = torch.randn(n, generator=g) * 0.01
        k.call("dpc_step_advance", st, bc, 0.9, 0.999)
        k.call("dpc_adam_dev", pk, k.t(gr), mk, vk, n, 1e-3, 0.9, 0.999, 1e-8, 1e-5, bc, 1.0)
        k.sync()
        O.adam_step(p, gr, m, v, step)
        assert int(st.item()) == step
        assert bc.cpu().tolist() == pytest_approx([1 - 0.9 ** step, 1 - 0.999 ** step])
    assert (pk.cpu() - p).abs().max().item() < 2e-6 and relerr(mk, m) < 1e-5 and relerr(vk, v) < 1e-5


def pytest_approx(v):
    import pytest
    return pytest.approx(v, rel=1e-6)


# ---------------------------------------------------------------- fused ConvGRU recurrence (csrc/gru_chain.hip)
def _chain_setup(k: K, dtype, B, SQ, D, P, n_agg, seed):
    g = torch.Generator().manual_seed(seed)
    ns, M = n_agg + P - 1, B * SQ
    w = {n: q(torch.randn(D, 2 * D, generator=g) * (1.0 / (2 * D) ** 0.5), dtype) for n in ("update", "reset", "out")}
    w["p0"] = q(torch.randn(D, D, generator=g) * (1.0 / D ** 0.5), dtype)
    w["p2"] = q(torch.randn(D, D, generator=g) * (1.0 / D ** 0.5), dtype)
    b = {n: torch.randn(D, generator=g) * 0.1 for n in ("update", "reset", "out", "p0", "p2")}
    x = q(torch.relu(torch.randn(n_agg, M, D, generator=g)), dtype)
    d_pred = torch.randn(B, P, SQ, D, generator=g) * 0.1
    dev = {}
    dev["packed"] = k.empty(16 * D * D, dtype=dtype)
    k.call("dpc_gru_pack", k.t(w["update"]), k.t(w["reset"]), k.t(w["out"]), k.t(w["p0"]), k.t(w["p2"]), D, L.dtype_code(dtype), dev["packed"])
    dev["bias"] = {n: k.t(v) for n, v in b.items()}
    X_all = k.zeros(ns, M, D, dtype=dtype)   # real input: the steps' inputs (the aggregation steps filled below)
    X_all[:n_agg] = k.t(x, dtype)
    H_all = k.zeros(ns + 1, M, D, dtype=dtype)   # real input: H_all[0] is the initial state h_0 = 0
    dev.update(X_all=X_all, H_all=H_all, HR_all=k.empty(ns, M, D, dtype=dtype),
               U_all=k.empty(ns, M, D), R_all=k.empty(ns, M, D), O_all=k.empty(ns, M, D), P1_all=k.empty(P, M, D, dtype=dtype),
               pred=k.empty(B, P, SQ, D, dtype=dtype), d_pred=k.t(d_pred), G_all=k.empty(ns, M, 3 * D, dtype=dtype),
               dP1=k.empty(P, M, D, dtype=dtype), dP2=k.empty(P, M, D, dtype=dtype), d_x=k.empty(n_agg, M, D), ws=k.empty(2, M, D))
    d = L.GruChainDesc()
    d.dtype, d.M, d.D, d.SQ, d.P, d.n_agg, d.n_steps = L.dtype_code(dtype), M, D, SQ, P, n_agg, ns
    d.p_drop, d.seed = 0.1, 233
    d.packed = dev["packed"].data_ptr()
    for f, n in (("bias_u", "update"), ("bias_r", "reset"), ("bias_o", "out"), ("bias_1", "p0"), ("bias_2", "p2")):
        setattr(d, f, dev["bias"][n].data_ptr())
    for f in ("X_all", "H_all", "HR_all", "U_all", "R_all", "O_all", "P1_all", "pred", "d_pred", "G_all", "dP1", "dP2", "d_x", "ws"):
        setattr(d, f, dev[f].data_ptr())
    return d, dev, w, b, x, d_pred


def case_gru_chain(k: K, dtype, B, SQ, D, P, n_agg, seed=21):
    """dpc_gru_chain_fwd/_bwd with injected dropout masks against autograd over the reference's recurrence
    (dpc/model_3d.py:62-72 restated with 1x1 convolutions as matmuls on rows m = (b, s))."""
    d, dev, w, b, x, d_pred = _chain_setup(k, dtype, B, SQ, D, P, n_agg, seed)
    ns, M = n_agg + P - 1, B * SQ
    g = torch.Generator().manual_seed(seed + 1)
    masks = (torch.rand(ns, M, D, generator=g) > 0.1).float() / 0.9
    mdev = k.t(masks)
    d.drop_masks = mdev.data_ptr()
    k.call("dpc_gru_chain_fwd", C.byref(d))
    k.call("dpc_gru_chain_bwd", C.byref(d))
    k.sync()
    # ---- expectation (f64 autograd; operands quantised where the kernel stores them in `dtype`)
    W = {n: v.double().requires_grad_() for n, v in w.items()}
    Bs = {n: v.double().requires_grad_() for n, v in b.items()}
    xs = x.double().requires_grad_()
    qd = (lambda t: t) if dtype == torch.float32 else (lambda t: t + (t.detach().to(dtype).double() - t.detach()))  # straight-through rounding

    def cell(xi, h):
        c = torch.cat([xi, h], 1)
        u = torch.sigmoid(c @ W["update"].t() + Bs["update"])
        r = torch.sigmoid(c @ W["reset"].t() + Bs["reset"])
        o = torch.tanh(torch.cat([xi, qd(h * r)], 1) @ W["out"].t() + Bs["out"])
        return h * (1 - u) + o * u

    h = torch.zeros(M, D, dtype=torch.float64)
    step, preds, hs = 0, [], [h]
    for t in range(n_agg):
        h = qd(cell(xs[t], h) * masks[step].double())
        hs.append(h)
        step += 1
    for i in range(P):
        p1 = qd(torch.relu(h @ W["p0"].t() + Bs["p0"]))
        p2 = p1 @ W["p2"].t() + Bs["p2"]
        preds.append(qd(p2))
        if i < P - 1:
            h = qd(cell(qd(torch.relu(p2)), h) * masks[step].double())
            hs.append(h)
            step += 1
    pred = torch.stack(preds, 1).view(B, SQ, P, D).permute(0, 2, 1, 3)  # rows (b, s) -> [B][P][SQ][D]
    (pred * d_pred.double()).sum().backward()
    t_f, t_b = (2e-5, 2e-4) if dtype == torch.float32 else (3e-2, 6e-2)
    assert relerr(dev["pred"], pred.detach()) < t_f
    assert relerr(dev["H_all"][1:], torch.stack(hs[1:]).detach()) < t_f
    assert relerr(dev["d_x"], xs.grad) < t_b
    # the saved operands give the reference's weight gradients (the engine's batched GEMMs compute exactly these products)
    G = dev["G_all"].double().cpu().view(ns * M, 3 * D)
    Xa = dev["X_all"].double().cpu().view(ns * M, D)
    Ha = dev["H_all"][:ns].double().cpu().view(ns * M, D)
    HRa = dev["HR_all"].double().cpu().view(ns * M, D)
    gW = {"update": torch.cat([G[:, :D].t() @ Xa, G[:, :D].t() @ Ha], 1), "reset": torch.cat([G[:, D:2 * D].t() @ Xa, G[:, D:2 * D].t() @ Ha], 1),
          "out": torch.cat([G[:, 2 * D:].t() @ Xa, G[:, 2 * D:].t() @ HRa], 1)}
    Hp = dev["H_all"][n_agg:].double().cpu().view(P * M, D)
    gW["p0"] = dev["dP1"].double().cpu().view(P * M, D).t() @ Hp
    gW["p2"] = dev["dP2"].double().cpu().view(P * M, D).t() @ dev["P1_all"].double().cpu().view(P * M, D)
    for n in gW:
        assert relerr(gW[n], W[n].grad) < t_b, n
    gB = {"update": G[:, :D].sum(0), "reset": G[:, D:2 * D].sum(0), "out": G[:, 2 * D:].sum(0),
          "p0": dev["dP1"].double().cpu().view(P * M, D).sum(0), "p2": dev["dP2"].double().cpu().view(P * M, D).sum(0)}
    for n in gB:
        assert relerr(gB[n], Bs[n].grad) < t_b, n


def case_gru_chain_philox(k: K, dtype, B, SQ, D, P, n_agg, seed=22):
    """train mode: masks generated in the kernel (Philox keyed on seed + device-side step) == the masks dpc_dropout_mask
    writes for the same (seed, step), injected explicitly: bit-identical states and gradients; eval mode = no mask."""
    ns, M = n_agg + P - 1, B * SQ
    step = torch.tensor([3], dtype=torch.int32, device=k.dev)
    d1, dev1, *_ = _chain_setup(k, dtype, B, SQ, D, P, n_agg, seed)
    d1.step_dev = step.data_ptr()
    k.call("dpc_gru_chain_fwd", C.byref(d1))
    k.call("dpc_gru_chain_bwd", C.byref(d1))
    d2, dev2, *_ = _chain_setup(k, dtype, B, SQ, D, P, n_agg, seed)
    masks = k.empty(ns, M, D)
    k.call("dpc_dropout_mask", masks, masks.numel(), 0.1, 233, step)
    d2.drop_masks = masks.data_ptr()
    k.call("dpc_gru_chain_fwd", C.byref(d2))
    k.call("dpc_gru_chain_bwd", C.byref(d2))
    k.sync()
    for f in ("H_all", "pred", "d_x", "G_all", "dP1"):
        assert torch.equal(dev1[f], dev2[f]), f
    assert 0.85 < (masks > 0).float().mean().item() < 0.95
    d3, dev3, *_ = _chain_setup(k, dtype, B, SQ, D, P, n_agg, seed)
    k.call("dpc_gru_chain_fwd", C.byref(d3))  # eval: neither masks nor a step counter
    k.sync()
    assert not torch.equal(dev3["H_all"], dev1["H_all"])


def case_gru_chain_golden(k: K, ops):
    """The reference's own ConvGRUCell(8, 8, 1) fixture (tests/golden/ops.npz "gru::*", forward + autograd of
    backbone/convrnn.py:24-34) through the fused recurrence kernels: one aggregation step from the fixture's non-zero
    h, the 8 channels zero-padded to the kernel's 32-channel granularity (padded channels stay exactly 0), and an
    identity predictor (W1 = W2 = I, b1 = +4, b2 = -4: relu is transparent for |h| < 1) so that d_pred IS d/dh'."""
    f32 = torch.float32
    x, h = torch.from_numpy(ops["gru::x"]), torch.from_numpy(ops["gru::h"])      # [3, 8, 3, 3]
    Bn, Cg, ls = x.shape[0], x.shape[1], x.shape[2]
    D, SQ, M = 32, ls * ls, Bn * ls * ls
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(M, Cg)
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[0], D - Cg)], 1)
    d, dev, *_ = _chain_setup(k, f32, Bn, SQ, D, 1, 1, seed=1)
    w = {}
    for gate in ("update", "reset", "out"):
        wg = torch.from_numpy(ops[f"gru::w::{gate}_gate.weight"]).view(Cg, 2 * Cg)
        full = torch.zeros(D, 2 * D)
        full[:Cg, :Cg], full[:Cg, D:D + Cg] = wg[:, :Cg], wg[:, Cg:]
        w[gate] = full
    eye = torch.eye(D)
    k.call("dpc_gru_pack", k.t(w["update"]), k.t(w["reset"]), k.t(w["out"]), k.t(eye), k.t(eye), D, L.F32, dev["packed"])
    for f, n in (("bias_u", "update"), ("bias_r", "reset"), ("bias_o", "out")):
        bt = k.t(torch.cat([torch.from_numpy(ops[f"gru::w::{n}_gate.bias"]), torch.zeros(D - Cg)]))
        dev["bias"][f] = bt
        setattr(d, f, bt.data_ptr())
    b1, b2 = k.t(torch.full((D,), 4.0)), k.t(torch.full((D,), -4.0))
    d.bias_1, d.bias_2 = b1.data_ptr(), b2.data_ptr()
    dev["X_all"][0] = k.t(pad(rows(x)))
    dev["H_all"][0] = k.t(pad(rows(h)))
    gh = torch.from_numpy(ops["gru::gh"])
    dev["d_pred"].copy_(k.t(pad(rows(gh)).view(Bn, SQ, 1, D).permute(0, 2, 1, 3).contiguous()))
    k.call("dpc_gru_chain_fwd", C.byref(d))
    k.call("dpc_gru_chain_bwd", C.byref(d))
    k.sync()
    hn = dev["H_all"][1].cpu()
    assert (hn[:, :Cg] - rows(torch.from_numpy(ops["gru::hn"]))).abs().max().item() < 1e-5
    assert hn[:, Cg:].abs().max().item() == 0
    assert (dev["pred"].cpu().view(Bn, SQ, D).reshape(M, D) - hn).abs().max().item() < 1e-5
    assert (dev["d_x"][0].cpu()[:, :Cg] - rows(torch.from_numpy(ops["gru::gx"]))).abs().max().item() < 1e-5
    G = dev["G_all"][0].cpu()
    Xr, Hr, HRr = pad(rows(x)), pad(rows(h)), dev["HR_all"][0].cpu()
    for gi, gate in enumerate(("update", "reset", "out")):
        Gg = G[:, gi * D:gi * D + Cg]
        gw = torch.cat([Gg.t() @ Xr[:, :Cg], Gg.t() @ (HRr if gate == "out" else Hr)[:, :Cg]], 1)
        ref = torch.from_numpy(ops[f"gru::gw::{gate}_gate.weight"]).view(Cg, 2 * Cg)
        assert (gw - ref).abs().max().item() < 1e-4, gate
        assert (Gg.sum(0) - torch.from_numpy(ops[f"gru::gw::{gate}_gate.bias"])).abs().max().item() < 1e-4, gate


# ---------------------------------------------------------------- fused score + CE/top-k + backward (csrc/score_fused.hip)
def case_score_fused(k: K, R, D, seed=31, check_score=True):
    """dpc_score_fwd / dpc_ce_finalize / dpc_score_bwd (bf16 operands, nothing [R][R] in memory) against the reference's
    formulation: score = pred @ finf^T (dpc/model_3d.py:83), CrossEntropyLoss with target = arange, calc_topk_accuracy,
    and autograd's d/dpred, d/dfinf -- computed in f64 from the same bf16-rounded operands."""
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(seed)
    pred = (torch.randn(R, D, generator=g) * (2.0 / D ** 0.5)).to(bf)
    finf = (torch.randn(R, D, generator=g) * (2.0 / D ** 0.5)).to(bf)
    idx = torch.arange(0, R, 3)
    finf[idx] = (finf[idx].float() + 1.5 * pred[idx].float()).to(bf)  # a third of the targets rank high
    pd, fd = pred.double().requires_grad_(), finf.double().requires_grad_()
    S = pd @ fd.t()
    tgt = torch.arange(R)
    loss = F.cross_entropy(S, tgt)
    loss.backward()
    rank = (S.detach() > S.detach().diagonal()[:, None]).sum(1)
    accs = [(rank < kk).double().mean().item() for kk in (1, 3, 5)]
    ld = (R + 7) // 8 * 8
    predT, finfT = k.zeros(D, ld, dtype=bf), k.zeros(D, ld, dtype=bf)   # real inputs: padded bf16 operands (filled below)
    predT[:, :R] = k.t(pred.t().contiguous())
    finfT[:, :R] = k.t(finf.t().contiguous())
    pk, fk = k.t(pred), k.t(finf)
    nf, nb = C.c_int64(0), C.c_int64(0)
    ns = k.lib.call("dpc_score_ws_floats", R, D, C.byref(nf), C.byref(nb))
    assert ns >= 1
    ws = k.empty(max(nf.value, nb.value))
    diag, lse2, row_ws, res = k.empty(R), k.empty(R), k.empty(R, 2), k.empty(4)
    score = k.empty(R, R) if check_score else None
    k.call("dpc_score_fwd", pk, fk, R, D, diag, lse2, row_ws, score, ws)
    k.call("dpc_ce_finalize", row_ws, R, res)
    k.sync()
    Sd = S.detach()
    if check_score:
        assert relerr(score, Sd) < 1e-5
    assert (diag.cpu().double() - Sd.diagonal()).abs().max().item() < 1e-4 * max(1.0, Sd.abs().max().item())
    lse = torch.logsumexp(Sd, 1)
    assert (row_ws[:, 0].cpu().double() - (lse - Sd.diagonal())).abs().max().item() < 2e-4
    # a logit within f32 rounding of the target may fall on either side: ranks may differ on a few rows by one
    dr = (row_ws[:, 1].cpu().double() - rank.double()).abs()
    assert dr.max().item() <= 1 and (dr > 0).double().mean().item() < 5e-3
    r = res.cpu()
    assert abs(r[0].item() - loss.item()) < 1e-4 * max(1.0, abs(loss.item()))
    for got, exp in zip(r[1:].tolist(), accs):
        assert abs(got - exp) <= 3.0 / R + 1e-6
    outs = {}
    for name, own, oth, othT, by_owner in (("d_pred", pk, fk, finfT, 1), ("d_finf", fk, pk, predT, 0)):
        n = k.lib.call("dpc_score_bwd", own, oth, othT, ld, R, D, lse2, by_owner, ws, k.lib.stream())
        assert n == ns
        out = k.empty(R, D)
        k.call("dpc_reduce_unpack", ws, n, out, R, 1, D, D, 0, 1, 0)
        outs[name] = out
    k.sync()
    # dS is rounded to bf16 before the second product: 2^-8 relative per term, averaged over R terms
    assert relerr(outs["d_pred"], pd.grad) < 1.5e-2
    assert relerr(outs["d_finf"], fd.grad) < 1.5e-2


def case_stem_wgrad_fused(k: K, BN, T, H, W, Co=64, seed=8):
    """dpc_stem_wgrad_fused (bf16): the stem's weight gradient computed from the gradient at the POOLED output with the
    max-pool routing and the BatchNorm backward inside the weight-gradient kernel, against (a) the two-kernel form
    dpc_pool_bn_bwd_apply -> dpc_conv_wgrad of the same library (bit-identical: same bf16 dz operand, same chunking) and
    (b) f64 autograd through conv -> batch-stat BN -> ReLU -> MaxPool3d (resnet_2d3d.py:211-214)."""
    bf = torch.bfloat16
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(BN, 3, T, H, W, generator=g)
    w = torch.randn(Co, 3, 1, 7, 7, generator=g) * 0.1
    gamma, beta = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.2
    Hs, Ws = H // 2, W // 2
    dc = L.BF16
    xs = k.empty(BN, T, Hs, Ws, 16, dtype=bf)
    k.call("dpc_pack_input_s2d", k.t(x), xs, dc, BN, T, H, W)
    wp = k.empty(Co, 16, 16, dtype=bf)
    k.call("dpc_pack_stem_weight", k.t(w), wp, dc, Co)
    d = conv_desc(bf, bf, 0, BN, (T, Hs, Ws), (T, Hs, Ws), 16, 16, Co, 256, Co, (1, 4, 4), (1, 1, 1), (0, 2, 2))
    dw_ = conv_desc(bf, torch.float32, 0, BN, (T, Hs, Ws), (T, Hs, Ws), 16, 16, Co, 256, Co, (1, 4, 4), (1, 1, 1), (0, 2, 2))
    raw = k.empty(BN, T, Hs, Ws, Co, dtype=bf)
    rows = k.lib.call("dpc_conv_stats_rows", C.byref(d))
    stats = k.poison(rows, 2, Co)
    k.call("dpc_conv_igemm", C.byref(d), xs, wp, raw, None, stats)
    M = BN * T * Hs * Ws
    mean, invstd, scale, shift = (k.empty(Co) for _ in range(4))
    k.call("dpc_bn_finalize", stats, rows, Co, float(M), k.t(gamma), k.t(beta), 1e-5, mean, invstd, scale, shift)
    Ho, Wo = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
    pooled = k.empty(BN * T, Ho, Wo, Co, dtype=bf)
    am = torch.empty(BN * T, Ho, Wo, Co, dtype=torch.uint8, device=k.dev)
    k.call("dpc_bn_relu_maxpool_fwd", raw, dc, BN * T, Hs, Ws, Co, scale, shift, pooled, am)
    gy = q(torch.randn(BN * T, Ho, Wo, Co, generator=g), bf)
    gyk = k.t(gy, bf)
    prow = C.c_int32(0)
    k.call("dpc_pooled_bn_bwd_reduce", None, None, None, dc, BN * T * Ho * Wo, Co, None, None, None, C.byref(prow))
    bp = k.poison(prow.value, 2, Co)
    k.call("dpc_pooled_bn_bwd_reduce", gyk, am, pooled, dc, BN * T * Ho * Wo, Co, k.t(gamma), k.t(beta), bp, C.byref(prow))
    dgam, dbet, coef = k.empty(Co), k.empty(Co), k.empty(2, Co)
    k.call("dpc_bn_bwd_finalize", bp, prow.value, Co, float(M), dgam, dbet, coef)
    # (a) two kernels
    dz = k.empty(BN, T, Hs, Ws, Co, dtype=bf)
    k.call("dpc_pool_bn_bwd_apply", gyk, am, raw, dc, BN * T, Hs, Ws, Co, mean, invstd, k.t(gamma), coef, dz)
    ns = C.c_int32(0)
    k.call("dpc_conv_wgrad", C.byref(dw_), None, None, Co, None, C.byref(ns))
    part = k.poison(ns.value, Co, 256)
    k.call("dpc_conv_wgrad", C.byref(dw_), xs, dz, Co, part, C.byref(ns))
    dw_a = k.poison(Co, 3, 1, 7, 7)
    k.call("dpc_unpack_stem_wgrad", part, ns.value, dw_a, Co)
    # (b) fused
    ns2 = C.c_int32(0)
    rc = k.lib.call("dpc_stem_wgrad_fused", C.byref(dw_), None, None, None, None, None, None, None, None, None, C.byref(ns2), k.lib.stream())
    assert rc == 0 and ns2.value == ns.value
    part2 = k.poison(ns2.value, Co, 256)
    k.call("dpc_stem_wgrad_fused", C.byref(dw_), xs, raw, gyk, am, mean, invstd, k.t(gamma), coef, part2, C.byref(ns2))
    dw_b = k.poison(Co, 3, 1, 7, 7)
    k.call("dpc_unpack_stem_wgrad", part2, ns2.value, dw_b, Co)
    k.sync()
    all_finite(stats, bp, part, part2, dw_a, dw_b)
    assert torch.equal(dw_a, dw_b)
    # (c) autograd (bf16 quantisation of operands / dz: loose bound; the exactness claim is (a) == (b))
    xq, wq = q(x, bf).double(), q(w, bf).double().requires_grad_()
    y = F.conv3d(xq, wq, None, (1, 2, 2), (0, 3, 3))
    # the two tables built on the way, against f64 sums of what the kernels were given: the stored raw output, and the pooled
    # gradient where the pooled activation's argmax byte routes it (a pooled row is what the reduction can lose)
    rw = raw.float().cpu().reshape(M, Co).double()
    mut = mutation_rows(cl(y.detach()).reshape(M, Co), conv_tile_rows(M))   # chosen from the expectation
    sg = stats.cpu().double()
    rejects_dropped_row(sg[:, 0].sum(0), rw, mut, "stem_wgrad_fused forward sum raw")
    rejects_dropped_row(sg[:, 1].sum(0), rw * rw, mut, "stem_wgrad_fused forward sum raw^2")
    rows_p = BN * T * Ho * Wo
    gyp = gy.double().reshape(rows_p, Co) * (pooled.float().cpu().reshape(rows_p, Co) > 0).double()
    rejects_dropped_row(bp.cpu().double()[:, 0].sum(0), gyp, mutation_rows(gyp), "stem_wgrad_fused bp sum dz")
    mu = y.mean((0, 2, 3, 4), keepdim=True); var = y.var((0, 2, 3, 4), unbiased=False, keepdim=True)
    z = (y - mu) / torch.sqrt(var + 1e-5) * gamma.double().view(1, -1, 1, 1, 1) + beta.double().view(1, -1, 1, 1, 1)
    pz = F.max_pool3d(F.relu(z), (1, 3, 3), (1, 2, 2), (0, 1, 1))
    gyr = gy.double().view(BN, T, Ho, Wo, Co).permute(0, 4, 1, 2, 3)
    gw = torch.autograd.grad(pz, wq, gyr)[0]
    assert relerr(dw_b, gw) < 0.15  # sanity: bf16 raw / dz and argmax near-ties at a tiny batch (observed 0.09, identical for (a))


# ------------------------------------------------------------------ bf16 logits of the train step (round 6)
def case_ce_topk_bf16(k: K, rows, cols, seed=10):
    """dpc_ce_topk_bf16: loss, top-1/3/5 and d(loss)/d(score) of bf16-ROUNDED logits (the expectation is computed on the rounded
    values: what the kernel is given); exact ties at the target's value rank behind it"""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(rows, cols, generator=g) * 3
    idx = torch.arange(0, rows, 3)
    s[idx, idx] += 6.0
    sq = s.to(torch.bfloat16)
    sd = sq.double().requires_grad_()
    tgt = torch.arange(rows)
    loss = F.cross_entropy(sd, tgt)
    loss.backward()
    rank = (sq.float() > sq.float().diagonal().view(-1, 1)[:, :1].expand(rows, cols)).sum(1)
    accs = [(rank < kk).float().mean().item() for kk in (1, 3, 5)]
    ld_d = (cols + 7) // 8 * 8
    ws, res = k.empty(rows, 2), k.empty(4)
    ds = k.empty(rows, ld_d, dtype=torch.bfloat16)
    k.call("dpc_ce_topk_bf16", k.t(sq, torch.bfloat16), rows, cols, cols, ws, res, ds, ld_d)
    k.sync()
    r = res.cpu()
    assert abs(r[0].item() - loss.item()) < 2e-5 * max(1.0, abs(loss.item()))
    assert [round(v, 6) for v in r[1:].tolist()] == [round(v, 6) for v in accs]
    assert relerr(ds[:, :cols], sd.grad) < tol(torch.bfloat16)
    assert row_offdiag_relerr(ds[:, :cols], sd.grad) < tol(torch.bfloat16)   # the same bound, per row
    assert torch.equal(ws[:, 1].cpu().double(), rank.double())               # strictly greater among the rounded values


def case_gemm_nt_bf16out(k: K, M, N, Kd, seed=3, expect="score_gemm2_kernel<KS,OUT16>"):
    """the materialised score in the compute dtype: A @ B^T rounded once to bf16 (whole 128-byte rows: N a multiple of 64)"""
    g = torch.Generator().manual_seed(seed)
    dtype = torch.bfloat16
    A = q(torch.randn(M, Kd, generator=g), dtype)
    B = q(torch.randn(N, Kd, generator=g), dtype)
    d = conv_desc(dtype, dtype, 0, M, (1, 1, 1), (1, 1, 1), Kd, Kd, N, Kd, N, (1, 1, 1), (1, 1, 1), (0, 0, 0))
    out = k.empty(M, N, dtype=dtype)
    k.call("dpc_conv_igemm", C.byref(d), k.t(A, dtype), k.t(B, dtype), out, None, None)
    check_kernel(k, expect)
    k.sync()
    want = (A.double() @ B.double().t())
    assert relerr(out, want) < 2.0 ** -8          # one rounding of an f32 accumulator
    assert torch.equal(out.cpu(), want.float().to(dtype)) or (out.cpu().float() - want.float()).abs().max().item() <= 2.0 ** -7 * want.abs().max().item()


# ---------------------------------------------------------------- the LC classifier's own kernels (csrc/lc_head.hip, bn.hip)
def _chain_lc_setup(k: K, dtype, B, SQ, D, n_agg, P, seed):
    """_chain_setup in the form LCEngine uses (dpc_amd/lc.py): P = 0 means n_steps = n_agg and no predictor buffers at all --
    built as the P = 1 setup (the same n_steps) with the predictor's pointers cleared"""
    d, dev, w, b, x, d_pred = _chain_setup(k, dtype, B, SQ, D, max(P, 1), n_agg, seed)
    if P == 0:
        d.P = 0
        d.P1_all = d.pred = d.d_pred = d.dP1 = d.dP2 = None
    return d, dev, w, b, x, d_pred


def case_gru_chain_lc(k: K, dtype, B, SQ, D, n_agg, P=0, h0=False, seed=41):
    """dpc_gru_chain_fwd/_bwd as the LC classifier drives them (eval/model_3d_lc.py:56-60): aggregation only (P = 0, n_steps =
    n_agg, every predictor buffer NULL), the backward seeded through d_hlast = d loss / d (last state); h0 = a non-zero H_all[0];
    P > 0 with d_hlast as well (include/dpc_hip.h: optional for any P).  Expectation: the f64 cell of case_gru_chain with
    loss = sum(H_all[n_steps] * d_hlast) (+ sum(pred * d_pred)); case_gru_chain's bounds."""
    d, dev, w, b, x, d_pred = _chain_lc_setup(k, dtype, B, SQ, D, n_agg, P, seed)
    ns, M = n_agg + max(P, 1) - 1, B * SQ
    g = torch.Generator().manual_seed(seed + 1)
    masks = (torch.rand(ns, M, D, generator=g) > 0.1).float() / 0.9
    d_hlast = torch.randn(M, D, generator=g) * 0.1
    h_init = q(torch.randn(M, D, generator=g) * 0.5, dtype) if h0 else torch.zeros(M, D)
    dev["H_all"][0] = k.t(h_init, dtype)
    mdev, ddev = k.t(masks), k.t(d_hlast)
    d.drop_masks, d.d_hlast = mdev.data_ptr(), ddev.data_ptr()
    k.call("dpc_gru_chain_fwd", C.byref(d))
    k.call("dpc_gru_chain_bwd", C.byref(d))
    k.sync()
    W = {n: v.double().requires_grad_() for n, v in w.items()}
    Bs = {n: v.double().requires_grad_() for n, v in b.items()}
    xs = x.double().requires_grad_()
    qd = (lambda t: t) if dtype == torch.float32 else (lambda t: t + (t.detach().to(dtype).double() - t.detach()))  # straight-through rounding

    def cell(xi, h):
        c = torch.cat([xi, h], 1)
        u = torch.sigmoid(c @ W["update"].t() + Bs["update"])
        r = torch.sigmoid(c @ W["reset"].t() + Bs["reset"])
        o = torch.tanh(torch.cat([xi, qd(h * r)], 1) @ W["out"].t() + Bs["out"])
        return h * (1 - u) + o * u

    h = h_init.double()
    step, preds, hs = 0, [], [h]
    for t in range(n_agg):
        h = qd(cell(xs[t], h) * masks[step].double())
        hs.append(h)
        step += 1
    for i in range(P):
        p1 = qd(torch.relu(h @ W["p0"].t() + Bs["p0"]))
        p2 = p1 @ W["p2"].t() + Bs["p2"]
        preds.append(qd(p2))
        if i < P - 1:
            h = qd(cell(qd(torch.relu(p2)), h) * masks[step].double())
            hs.append(h)
            step += 1
    assert len(hs) == ns + 1
    loss = (hs[-1] * d_hlast.double()).sum()
    if P > 0:
        pred = torch.stack(preds, 1).view(B, SQ, P, D).permute(0, 2, 1, 3)
        loss = loss + (pred * d_pred.double()).sum()
    loss.backward()
    t_f, t_b = (2e-5, 2e-4) if dtype == torch.float32 else (3e-2, 6e-2)
    assert relerr(dev["H_all"][1:], torch.stack(hs[1:]).detach()) < t_f
    assert torch.equal(dev["H_all"][0].cpu(), h_init.to(dtype))   # h_0 is read, never written
    if P > 0:
        assert relerr(dev["pred"], pred.detach()) < t_f
    assert relerr(dev["d_x"], xs.grad) < t_b
    G = dev["G_all"].double().cpu().view(ns * M, 3 * D)
    Xa = dev["X_all"].double().cpu().view(ns * M, D)
    Ha = dev["H_all"][:ns].double().cpu().view(ns * M, D)
    HRa = dev["HR_all"].double().cpu().view(ns * M, D)
    gW = {"update": torch.cat([G[:, :D].t() @ Xa, G[:, :D].t() @ Ha], 1), "reset": torch.cat([G[:, D:2 * D].t() @ Xa, G[:, D:2 * D].t() @ Ha], 1),
          "out": torch.cat([G[:, 2 * D:].t() @ Xa, G[:, 2 * D:].t() @ HRa], 1)}
    gB = {"update": G[:, :D].sum(0), "reset": G[:, D:2 * D].sum(0), "out": G[:, 2 * D:].sum(0)}
    if P > 0:
        Hp = dev["H_all"][n_agg:].double().cpu().view(P * M, D)
        gW["p0"] = dev["dP1"].double().cpu().view(P * M, D).t() @ Hp
        gW["p2"] = dev["dP2"].double().cpu().view(P * M, D).t() @ dev["P1_all"].double().cpu().view(P * M, D)
        gB["p0"], gB["p2"] = dev["dP1"].double().cpu().view(P * M, D).sum(0), dev["dP2"].double().cpu().view(P * M, D).sum(0)
    for n in gW:
        assert relerr(gW[n], W[n].grad) < t_b, n
    for n in gB:
        assert relerr(gB[n], Bs[n].grad) < t_b, n


def case_gru_chain_lc_philox(k: K, dtype, B, SQ, D, n_agg, seed=42):
    """the P = 0 recurrence with masks drawn in the kernel == the masks dpc_dropout_mask writes for the same (seed, step), injected
    explicitly: bit-identical states and gradients; eval mode (neither masks nor a step counter) differs"""
    M = B * SQ
    step = torch.tensor([6], dtype=torch.int32, device=k.dev)
    g = torch.Generator().manual_seed(seed + 1)
    ddev = k.t(torch.randn(M, D, generator=g) * 0.1)
    d1, dev1, *_ = _chain_lc_setup(k, dtype, B, SQ, D, n_agg, 0, seed)
    d1.step_dev, d1.d_hlast = step.data_ptr(), ddev.data_ptr()
    k.call("dpc_gru_chain_fwd", C.byref(d1))
    k.call("dpc_gru_chain_bwd", C.byref(d1))
    d2, dev2, *_ = _chain_lc_setup(k, dtype, B, SQ, D, n_agg, 0, seed)
    masks = k.empty(n_agg, M, D)
    k.call("dpc_dropout_mask", masks, masks.numel(), 0.1, 233, step)
    d2.drop_masks, d2.d_hlast = masks.data_ptr(), ddev.data_ptr()
    k.call("dpc_gru_chain_fwd", C.byref(d2))
    k.call("dpc_gru_chain_bwd", C.byref(d2))
    k.sync()
    for f in ("H_all", "HR_all", "d_x", "G_all"):
        assert torch.equal(dev1[f], dev2[f]), f
    assert 0.85 < (masks > 0).float().mean().item() < 0.95
    d3, dev3, *_ = _chain_lc_setup(k, dtype, B, SQ, D, n_agg, 0, seed)
    k.call("dpc_gru_chain_fwd", C.byref(d3))
    k.sync()
    assert not torch.equal(dev3["H_all"], dev1["H_all"])


LC_MOMENTUM, LC_EPS = 0.1, 1e-5
LC_OFFSET_SPREAD = 0.02    # std of a clip's context around 0.9 in the `offset` variant (widened from 0.003, see case_lc_head)
_LC_BUFS = ("ctx", "xhat", "bn_out", "y", "stat", "logits", "dlogits", "row_ws", "result", "g_fc_weight", "g_fc_bias", "g_bn_weight",
            "g_bn_bias", "dctx", "d_hlast")


def _lc_head_chain(inp, dt, explicit):
    """the head as a chain of torch CPU ops in `dt`: spatial mean -> BatchNorm1d (train) -> keep mask -> Linear -> cross_entropy
    (mean), autograd for the gradients, then the eval-mode forward from the updated running buffers.  explicit: BatchNorm written
    out (the f64 expectation); else F.batch_norm (the f32 chain the reference model itself runs, eval/model_3d_lc.py:58-64)"""
    B, SQ, D = inp["B"], inp["SQ"], inp["D"]
    h = inp["h"].to(dt).requires_grad_()
    gam, bet, W, bias = (inp[n].to(dt).requires_grad_() for n in ("gamma", "beta", "W", "bias"))
    rm, rv, keep, tgt = inp["rm"].to(dt).clone(), inp["rv"].to(dt).clone(), inp["keep"].to(dt), inp["target"]
    ctx = h.view(B, SQ, D).mean(1)
    mean, var = ctx.mean(0), ctx.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + LC_EPS)
    if explicit:
        xhat = (ctx - mean) * invstd
        bn = xhat * gam + bet
        unb = var * B / (B - 1) if B > 1 else var
        rm = (1 - LC_MOMENTUM) * rm + LC_MOMENTUM * mean.detach()
        rv = (1 - LC_MOMENTUM) * rv + LC_MOMENTUM * unb.detach()
        bn_e = (ctx.detach() - rm) / torch.sqrt(rv + LC_EPS) * gam.detach() + bet.detach()
    else:
        xhat = F.batch_norm(ctx, None, None, None, None, True, LC_MOMENTUM, LC_EPS)
        bn = F.batch_norm(ctx, rm, rv, gam, bet, True, LC_MOMENTUM, LC_EPS)   # updates rm / rv in place
        bn_e = F.batch_norm(ctx.detach(), rm, rv, gam.detach(), bet.detach(), False, LC_MOMENTUM, LC_EPS)
    y = bn * keep
    logits = F.linear(y, W, bias)
    logits.retain_grad()
    loss = F.cross_entropy(logits, tgt)
    loss.backward()
    with torch.no_grad():
        logits_e = F.linear(bn_e, W, bias)
    out = dict(ctx=ctx, xhat=xhat, bn_out=bn, y=y, stat_mean=mean, stat_invstd=invstd, logits=logits, loss=loss.view(1), dlogits=logits.grad,
               g_fc_weight=W.grad, g_fc_bias=bias.grad, g_bn_weight=gam.grad, g_bn_bias=bet.grad, d_hlast=h.grad, running_mean=rm,
               running_var=rv, eval_bn_out=bn_e, eval_logits=logits_e)
    return {n: v.detach().double() for n, v in out.items()}


def _lc_head_inputs(dtype, B, SQ, D, NC, variant, seed):
    g = torch.Generator().manual_seed(seed)
    if variant == "offset":   # every clip's context = 0.9 +- LC_OFFSET_SPREAD per channel; the spatial part has zero mean
        e = torch.randn(B, SQ, D, generator=g) * 1e-3
        h = 0.9 + LC_OFFSET_SPREAD * torch.randn(B, 1, D, generator=g) + (e - e.mean(1, keepdim=True))
    else:
        h = torch.randn(B, SQ, D, generator=g) * 0.3
    inp = dict(B=B, SQ=SQ, D=D, NC=NC, h=q(h.reshape(B * SQ, D), dtype), gamma=torch.rand(D, generator=g) + 0.5,
               beta=torch.randn(D, generator=g) * 0.3, rm=torch.randn(D, generator=g) * 0.2, rv=torch.rand(D, generator=g) + 0.5,
               W=torch.randn(NC, D, generator=g) / D ** 0.5, bias=torch.randn(NC, generator=g) * 0.1,
               target=torch.randint(0, NC, (B,), generator=g), keep=(torch.rand(B, D, generator=g) > 0.5).float() / 0.5)
    if variant == "dead_channel":
        inp["gamma"][1] = 0.0
        inp["beta"][1] = 0.0          # channel 1: BatchNorm output exactly 0 for every clip
        inp["beta"][2] = 0.0          # channel 2: zero shift only
        inp["keep"][0::2, 1], inp["keep"][1::2, 1] = 2.0, 0.0   # the dead channel keeps every other clip: its gradients are not 0
    elif variant == "ties":
        lo, hi = 3, 7
        inp["W"][hi] = inp["W"][lo]
        inp["bias"][lo] = inp["bias"][hi] = 12.0                 # the tied pair is the maximum of every row (asserted on the reference)
        inp["target"] = torch.tensor([lo, hi, lo, 0, NC - 1])[torch.arange(B) % 5]   # more rows at the lower index than at the higher
    elif variant == "hot":
        lg = _lc_head_chain(inp, torch.float64, True)["logits"]
        inp["W"] = inp["W"] * (80.0 / lg.abs().max().item())    # logits span about +-80
    else:
        assert variant in ("centred", "offset")
    return inp


def lc_head_reference(dtype, B, SQ, D, NC, variant, seed=51):
    """inputs, f64 expectation, and the bound of every compared quantity: 8 x the error of the f32 torch chain against the f64
    expectation (max-abs relative to the tensor's max-abs, as relerr), floor 1e-6 -- from the reference alone"""
    inp = _lc_head_inputs(dtype, B, SQ, D, NC, variant, seed)
    want = _lc_head_chain(inp, torch.float64, True)
    f32 = _lc_head_chain(inp, torch.float32, False)
    if variant == "dead_channel":   # the dead channel on its own, relative to ITS reference value: against the tensor's max-abs it can hide
        for r in (want, f32):
            r["g_bn_weight_dead"], r["g_bn_bias_dead"] = r["g_bn_weight"][1:2], r["g_bn_bias"][1:2]
        assert want["g_bn_weight_dead"].abs().item() > 1e-3 and want["g_bn_bias_dead"].abs().item() > 1e-3
    e32 = {n: relerr(f32[n], want[n]) for n in want}
    bound = {n: max(8.0 * e, 1e-6) for n, e in e32.items()}
    lg = want["logits"].clone()
    if variant == "ties":
        assert (lg[:, 3] - lg[:, 7]).abs().max().item() < 1e-12 and bool((lg[:, 3:4] > lg[:, [c for c in range(NC) if c not in (3, 7)]]).all())
        lg[:, 7] = lg[:, 3]       # bit-exact in the expectation too, whatever the matmul's summation order
    first_max = (lg == lg.max(1, keepdim=True).values).double().argmax(1)   # the first maximum wins (torch.max, eval/test.py:250)
    hits = (first_max == inp["target"]).double()
    if variant == "ties":   # rows target the lower and the higher index in different numbers: "last maximum wins" gives another accuracy
        n_lo, n_hi = int((inp["target"] == 3).sum()), int((inp["target"] == 7).sum())
        assert n_lo > n_hi > 0 and hits.sum().item() == n_lo
    return inp, want, e32, bound, hits


def _lc_head_desc(k: K, dtype, inp, p_drop, keep=None, step=None, seed=667, nbt0=7):
    B, SQ, D, NC = inp["B"], inp["SQ"], inp["D"], inp["NC"]
    t = {n: k.poison(*s) for n, s in (("ctx", (B, D)), ("xhat", (B, D)), ("bn_out", (B, D)), ("y", (B, D)), ("dctx", (B, D)), ("stat", (2, D)),
                                    ("logits", (B, NC)), ("dlogits", (B, NC)), ("row_ws", (B, 2)), ("result", (2,)), ("g_fc_weight", (NC, D)),
                                    ("g_fc_bias", (NC,)), ("g_bn_weight", (D,)), ("g_bn_bias", (D,)), ("d_hlast", (B * SQ, D)))}
    t.update(h_last=k.t(inp["h"], dtype), bn_weight=k.t(inp["gamma"]), bn_bias=k.t(inp["beta"]), bn_running_mean=k.t(inp["rm"].clone()),
             bn_running_var=k.t(inp["rv"].clone()), bn_num_batches=torch.full((), nbt0, dtype=torch.int64, device=k.dev),
             fc_weight=k.t(inp["W"]), fc_bias=k.t(inp["bias"]), target=k.t(inp["target"]))
    d = L.LcHeadDesc()
    d.dtype, d.B, d.SQ, d.D, d.num_class, d.train = L.dtype_code(dtype), B, SQ, D, NC, 1
    d.p_drop, d.momentum, d.eps, d.seed = p_drop, LC_MOMENTUM, LC_EPS, seed
    if keep is not None:
        t["drop_mask"] = k.t(keep)
    if step is not None:
        t["step_dev"] = step
    for n, v in t.items():
        setattr(d, n, v.data_ptr())
    return d, t


def case_lc_head(k: K, dtype, B, SQ, D, NC, variant):
    """dpc_lc_head_fwd (train) -> dpc_lc_head_bwd -> dpc_lc_head_fwd (eval) against f64 autograd over spatial mean -> BatchNorm1d ->
    keep mask -> Linear -> cross_entropy (lc_head_reference).  h_last is quantised to `dtype` first; everything after it is f32 in
    the kernel, so both dtypes get the same bound: per quantity 8 x the error of the f32 torch chain (F.batch_norm, F.linear,
    F.cross_entropy, autograd) on the same inputs against the f64 expectation, floor 1e-6; the case asserts that no bound exceeds
    tol(f32).  The margin of 8 covers another summation order over up to 300 channels / 1024 classes.

    Worst f32-torch error over the compared quantities, measured on the CPU, f32 [bf16] input (worst quantity of the f32 run):
      at (16, 16, 256, 101): centred 6.0e-7 [6.4e-7] (eval_logits), offset 5.2e-6 [1.6e-6] (y), dead_channel 6.4e-7 [5.7e-7] (d_hlast),
        ties 3.6e-7 [4.9e-7] (g_bn_weight), hot 1.9e-6 [1.8e-6] (dlogits);
      at (6, 3, 40, 11): centred 1.9e-7 [2.4e-7], offset 6.2e-6 [6.1e-6] (xhat), dead_channel 2.1e-7 [5.1e-7], ties 1.6e-7 [1.3e-7],
        hot 2.7e-7 [5.6e-7].
    `offset`: every clip's context is 0.9 +- LC_OFFSET_SPREAD per channel.  At a spread of 0.003 torch's own f32 BatchNorm chain is
    NOT within 1e-5 (3.1e-5 at (16, 16, 256, 101), g_bn_weight; 1.6e-5 at (6, 3, 40, 11), xhat: ctx is an f32 mean of values near
    0.9, half an ulp of it is 3e-8 = 1e-5 of the spread), which would put 8 x that above tol(f32).  The spread is therefore widened:
    of 0.005 / 0.008 / 0.01 / 0.015 / 0.02, 0.015 is the first within 1e-5 at both shapes and both dtypes (<= 7.6e-6); 0.02
    (<= 6.2e-6) is used, for headroom on a CPU whose torch sums in another order (the case asserts 8 x the error <= tol(f32)).
    |mean| / std is still 45: s2/B - mean^2 in f32 misses invstd by 1.5e-3 at (6, 3, 40, 11), where the bound is 8e-6."""
    inp, want, e32, bound, hits = lc_head_reference(dtype, B, SQ, D, NC, variant)
    worst = max(bound.values())
    assert worst <= tol(torch.float32), (worst, max(e32, key=e32.get))
    d, t = _lc_head_desc(k, dtype, inp, 0.5, keep=inp["keep"])
    k.call("dpc_lc_head_fwd", C.byref(d))
    k.call("dpc_lc_head_bwd", C.byref(d))
    k.sync()
    all_finite(*(t[n] for n in _LC_BUFS))                                     # the whole output dictionary was written
    got = {n: t[n].detach().cpu().clone() for n in _LC_BUFS}
    got.update(stat_mean=got["stat"][0], stat_invstd=got["stat"][1], loss=got["result"][:1], running_mean=t["bn_running_mean"].cpu().clone(),
               running_var=t["bn_running_var"].cpu().clone())
    assert int(t["bn_num_batches"]) == 8
    d.train = 0
    k.call("dpc_lc_head_fwd", C.byref(d))
    k.sync()
    got.update(eval_bn_out=t["bn_out"].cpu(), eval_logits=t["logits"].cpu())
    assert int(t["bn_num_batches"]) == 8                                       # unchanged by eval, as are the running buffers
    assert torch.equal(t["bn_running_mean"].cpu(), got["running_mean"]) and torch.equal(t["bn_running_var"].cpu(), got["running_var"])
    if variant == "dead_channel":
        got["g_bn_weight_dead"], got["g_bn_bias_dead"] = got["g_bn_weight"][1:2], got["g_bn_bias"][1:2]
        assert got["bn_out"][:, 1].abs().max().item() == 0
    errs = {n: relerr(got[n], want[n]) for n in want}
    bad = {n: (errs[n], bound[n]) for n in want if not errs[n] < bound[n]}
    assert not bad, f"(error, bound) {bad}"
    assert torch.isfinite(got["loss"]).all() and torch.isfinite(got["dlogits"]).all()
    assert torch.equal(got["row_ws"][:, 1].double(), hits)                      # the top-1 hit of every clip: the first maximum wins
    assert got["result"][1].item() == pytest_approx(hits.mean().item())
    if variant == "ties":
        assert torch.equal(got["logits"][:, 3], got["logits"][:, 7])            # the tie is bit-exact in the kernel
    return errs, e32


def case_lc_head_rejects(k: K):
    """the class scratch holds 1024 logits: num_class = 1025 is an argument error, not a launch"""
    import pytest
    inp = _lc_head_inputs(torch.float32, 2, 1, 8, 1025, "centred", 5)
    d, t = _lc_head_desc(k, torch.float32, inp, 0.5, keep=inp["keep"])
    with pytest.raises(L.DpcError, match=f"code {L.ERR_ARG}$"):
        k.call("dpc_lc_head_fwd", C.byref(d))


def case_lc_head_philox(k: K, B, SQ, D, NC, p, seed=667):
    """drop_mask = NULL, step_dev set: the head draws its keep mask from Philox stream 1 of (seed, step) -- the bits
    dropout_mask_np(B*D, p, seed, step, stream=1) gives, not those of the recurrence's stream 0; forward and backward equal the
    run with that mask injected explicitly bit for bit; another step draws another mask"""
    import numpy as np
    f32 = torch.float32
    inp = _lc_head_inputs(f32, B, SQ, D, NC, "centred", 52)
    step = torch.tensor([4], dtype=torch.int32, device=k.dev)
    d1, t1 = _lc_head_desc(k, f32, inp, p, step=step, seed=seed)
    k.call("dpc_lc_head_fwd", C.byref(d1))
    k.call("dpc_lc_head_bwd", C.byref(d1))
    k.sync()
    m1 = dropout_mask_np(B * D, p, seed, 4, stream=1).reshape(B, D)
    m0 = dropout_mask_np(B * D, p, seed, 4, stream=0).reshape(B, D)
    assert not np.array_equal(m1, m0)
    y, bn = t1["y"].cpu(), t1["bn_out"].cpu()
    nz = (bn != 0).numpy()
    assert nz.mean() > 0.99
    assert np.array_equal((y.numpy() != 0)[nz], (m1 != 0)[nz]) and not np.array_equal((y.numpy() != 0)[nz], (m0 != 0)[nz])
    assert torch.equal(y, bn * torch.from_numpy(m1))                             # the keep VALUE too: one f32 product
    assert abs(float((m1 != 0).mean()) - (1 - p)) < 4 * (p * (1 - p) / (B * D)) ** 0.5 + 1e-9
    d2, t2 = _lc_head_desc(k, f32, inp, p, keep=torch.from_numpy(m1), seed=seed)
    k.call("dpc_lc_head_fwd", C.byref(d2))
    k.call("dpc_lc_head_bwd", C.byref(d2))
    k.sync()
    for n in _LC_BUFS + ("bn_running_mean", "bn_running_var", "bn_num_batches"):
        assert torch.equal(t1[n], t2[n]), n
    assert t1["g_bn_weight"].abs().max().item() > 0 and t1["d_hlast"].abs().max().item() > 0
    step.fill_(5)
    k.call("dpc_lc_head_fwd", C.byref(d1))
    k.sync()
    m5 = dropout_mask_np(B * D, p, seed, 5, stream=1).reshape(B, D)
    assert not np.array_equal(m5, m1)
    assert torch.equal(t1["y"].cpu(), t1["bn_out"].cpu() * torch.from_numpy(m5))


def case_relu_tpool(k: K, dtype, B, N, T, SQ, D, seed=61):
    """dpc_relu_tpool_fwd / _bwd (ReLU BEFORE the temporal mean, eval/model_3d_lc.py:52-54) against f64 relu(x).mean(1) and its
    autograd, output layout [N][B*SQ][D], d_feat f32.  Planted in x: exact +0.0 and -0.0, negatives, and for bf16 subnormals of both
    signs; dx must be exactly 0 wherever x <= 0 (torch's ReLU gradient at 0 is 0) and within tol(dtype) elsewhere."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * N, T, SQ, D, generator=g)
    flat = x.view(-1)
    n = flat.numel()
    flat[0::7] = 0.0
    flat[3::11] = -0.0
    flat[5::13] = -flat[5::13].abs() - 0.25
    if dtype == torch.bfloat16:
        flat[1::17] = 2.0 ** -130     # bf16 subnormals (the smallest normal is 2^-126): positive ones pass the ReLU
        flat[2::19] = -(2.0 ** -130)
    flat[n - 1] = 0.0                  # the last element of the last unit
    x = q(x, dtype)
    xd = x.double().requires_grad_()
    feat = torch.relu(xd).view(B, N, T, SQ, D).mean(2).permute(1, 0, 2, 3).reshape(N, B * SQ, D)
    d_feat = torch.randn(N, B * SQ, D, generator=g)
    gx = torch.autograd.grad(feat, xd, d_feat.double())[0]
    xk = k.t(x, dtype)
    fk = k.empty(N, B * SQ, D, dtype=dtype)
    k.call("dpc_relu_tpool_fwd", xk, L.dtype_code(dtype), B, N, T, SQ, D, fk)
    dx = k.empty(B * N, T, SQ, D, dtype=dtype)
    k.call("dpc_relu_tpool_bwd", xk, k.t(d_feat), L.dtype_code(dtype), B, N, T, SQ, D, dx)
    k.sync()
    assert relerr(fk, feat.detach()) < tol(dtype)
    dxc = dx.float().cpu()
    nonpos = x <= 0
    assert nonpos.float().mean().item() > 0.5 and bool((x[nonpos] == 0).any())
    assert bool((dxc[nonpos] == 0).all())
    assert bool((gx[nonpos] == 0).all())                                        # the expectation agrees on the planted zeros
    assert relerr(dxc, gx) < tol(dtype)
    if dtype == torch.bfloat16:
        sub = (x > 0) & (x < 2.0 ** -126)
        assert bool(sub.any()) and bool((dxc[sub] != 0).all())                  # a positive subnormal is > 0


def case_bn_finalize_running(k: K, rows, Cc, count=None, misalign=0, momentum=0.1, seed=11):
    """dpc_bn_finalize_running on case_bn_finalize's table: mean / invstd / scale / shift bit-equal to dpc_bn_finalize's, the running
    buffers (non-trivial start) against the f64 momentum update with the UNBIASED variance (count = 1: the biased one), rtol 1e-6
    of the result (the momentum is the f32 value the C ABI passes), num_batches_tracked + 1 per launch whatever the grid, NULL
    accepted; then dpc_bn_eval_coeffs from those buffers against f64, rtol 1e-6 of the result, shift included."""
    g = torch.Generator().manual_seed(seed)
    parts = torch.randn(rows, 2, Cc, generator=g)
    parts[:, 1] = parts[:, 1].abs() * 3 + parts[:, 0] ** 2
    count = float(rows * 7) if count is None else float(count)
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g)
    rm0, rv0 = torch.randn(Cc, generator=g) * 0.5, torch.rand(Cc, generator=g) + 0.5
    buf = k.zeros(rows * 2 * Cc + 4)   # real input: the table the finalize kernels READ (filled below)
    pk = buf[misalign:misalign + rows * 2 * Cc].view(rows, 2, Cc)
    pk.copy_(parts)
    s1, s2 = parts[:, 0].double().sum(0), parts[:, 1].double().sum(0)
    m = s1 / count
    var = (s2 / count - m * m).clamp_min(0)
    unb = var * count / (count - 1.0) if count > 1.0 else var
    base = [k.empty(Cc) for _ in range(4)]
    k.call("dpc_bn_finalize", pk, rows, Cc, count, k.t(gamma), k.t(beta), 1e-5, *base)
    out = [k.empty(Cc) for _ in range(4)]
    rm, rv = k.t(rm0.clone()), k.t(rv0.clone())
    nbt = torch.full((), 5, dtype=torch.int64, device=k.dev)
    k.call("dpc_bn_finalize_running", pk, rows, Cc, count, k.t(gamma), k.t(beta), 1e-5, *out, rm, rv, nbt, momentum)
    k.sync()
    for a, b_, n in zip(out, base, ("mean", "invstd", "scale", "shift")):
        assert torch.equal(a, b_), n
    assert int(nbt) == 6
    f = lambda t: t.cpu().double()  # noqa: E731
    close = lambda got, exp: torch.allclose(f(got), exp, rtol=1e-6, atol=0)  # noqa: E731
    mo = torch.tensor(momentum, dtype=torch.float32).double().item()
    r1, r2 = (1 - mo) * rm0.double() + mo * m, (1 - mo) * rv0.double() + mo * unb
    assert close(rm, r1), "running_mean"
    assert close(rv, r2), "running_var"
    if count > 1.0:   # teeth: the biased variance must not pass for the unbiased one
        assert not close(rv, (1 - mo) * rv0.double() + mo * var)
    rm1, rv1 = f(rm).clone(), f(rv).clone()   # the second update starts from the f32 values the first one stored
    out2 = [k.empty(Cc) for _ in range(4)]
    k.call("dpc_bn_finalize_running", pk, rows, Cc, count, k.t(gamma), k.t(beta), 1e-5, *out2, rm, rv, None, momentum)   # NULL counter
    k.sync()
    assert int(nbt) == 6 and all(torch.equal(a, b_) for a, b_ in zip(out2, base))
    assert close(rm, (1 - mo) * rm1 + mo * m), "running_mean, second launch"
    assert close(rv, (1 - mo) * rv1 + mo * unb), "running_var, second launch"
    # eval: coefficients from the running buffers as they now stand on the device
    rmd, rvd = f(rm), f(rv)
    ev = [k.empty(Cc) for _ in range(4)]
    k.call("dpc_bn_eval_coeffs", k.t(gamma), k.t(beta), rm, rv, 1e-5, Cc, *ev)
    k.sync()
    inv = 1.0 / torch.sqrt(rvd + 1e-5)
    sc = gamma.double() * inv
    assert torch.equal(ev[0], rm)
    assert close(ev[1], inv) and close(ev[2], sc)
    assert close(ev[3], beta.double() - rmd * sc), "shift"
