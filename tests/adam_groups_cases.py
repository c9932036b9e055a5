"""dpc_adam_groups_dev (csrc/loss.hip) against an f64 Adam, shared by the CPU tier (host SIMT simulator,
tests/test_adam_groups_emu.py) and the GPU tier (tests/test_lc_groups_gpu.py).

Arena: 130 segments, 126 of them 4 floats long, alternating between two (lr, weight_decay) pairs so that no two neighbours could be
merged; one segment of 1028 floats that straddles the boundary between two of the kernel's tiles (4096 floats each); one frozen
segment in the middle whose g, m and v are NaN; one active segment with lr = 0; one gap (3500 floats, so that the segments lie
in three tiles and the table search starts past the gap).

Bounds, all from the number format (f32, unit roundoff u = 2^-24):
  p : 1e-7 * max(1, max|p|)            -- the project's own bound for one Adam step (tests/test_engine_emu.py:214)
  m : 8 u * (|b1 m| + |(1-b1) s g| + |(1-b1) wd p|)              -- a sum of at most three products, at most eight roundings on the
  v : 8 u * (|b2 v| + (1-b2) (|s g| + |wd p|)^2)                    longest path, constants included
"""
import ctypes as C

import torch

from dpc_amd import _lib as L
from kcases import K

B1, B2, EPS = 0.9, 0.999, 1e-8
PAIRS = ((1e-3, 1e-5), (1e-4, 1e-3))
U8 = 8.0 * 2.0 ** -24
TILE = 4096   # floats per tile of adam_groups_kernel (ADAM_TILE4 * 4)


def layout():
    """[(begin, end, lr, wd, active)], the arena size, and the indices of the special segments"""
    segs, off = [], 0
    special = {}
    for i in range(130):
        n = 4
        lr, wd = PAIRS[i % 2]
        active = 1
        if i == 30:
            off += 3500                      # the gap: padding nobody may touch
            n = 1028
            special["big"] = i
        elif i == 65:
            n, active = 8, 0
            special["frozen"] = i
        elif i == 90:
            n, lr = 8, 0.0
            special["lr0"] = i
        segs.append((off, off + n, lr, wd, active))
        off += n
    special["gap"] = (segs[29][1], segs[30][0])
    b, e = segs[special["big"]][:2]
    assert b // TILE != (e - 1) // TILE, "the long segment is meant to straddle two tiles"
    assert len({s[0] // TILE for s in segs}) >= 2
    return segs, off, special


def table(k: K, segs):
    tab = (L.AdamSegment * len(segs))()
    for i, (b, e, lr, wd, a) in enumerate(segs):
        tab[i] = L.AdamSegment(b, e, lr, wd, a, 0)
    return k.t(torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).clone())


def adam_f64(p, g, m, v, lr, wd, bc, gscale):
    """one Adam step in f64 from f32 state (lr, wd: per-element tensors); returns new p, m, v and the m / v bounds"""
    p, g, m, v, lr, wd = (t.double() for t in (p, g, m, v, lr, wd))
    bc1, bc2 = float(bc[0]), float(bc[1])
    gg = g * gscale + wd * p
    m2 = B1 * m + (1 - B1) * gg
    v2 = B2 * v + (1 - B2) * gg * gg
    p2 = p - (lr / bc1) * m2 / (v2.sqrt() / bc2 ** 0.5 + EPS)
    bm = U8 * ((B1 * m).abs() + (1 - B1) * (g * gscale).abs() + (1 - B1) * (wd * p).abs())
    bv = U8 * ((B2 * v).abs() + (1 - B2) * ((g * gscale).abs() + (wd * p).abs()) ** 2)
    return p2, m2, v2, bm, bv


def case_adam_groups(k: K, report=print):
    segs, n, sp = layout()
    gen = torch.Generator().manual_seed(11)
    p0, g0 = torch.randn(n, generator=gen) * 0.5, torch.randn(n, generator=gen)
    m0, v0 = torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 1e-2
    fb, fe = segs[sp["frozen"]][:2]
    gscale = 0.5
    # bias corrections of step 3, as the engine gets them: dpc_step_advance on the device
    step, bc = k.t(torch.tensor([2], dtype=torch.int32)), k.t(torch.ones(2))
    k.call("dpc_step_advance", step, bc, B1, B2)
    k.sync()
    bc_h = bc.cpu()
    assert int(step.cpu()) == 3 and abs(bc_h[0].item() - (1 - B1 ** 3)) < 1e-7

    # ---- (1) the segment table
    g1, m1, v1 = g0.clone(), m0.clone(), v0.clone()
    for t in (g1, m1, v1):
        t[fb:fe] = float("nan")
    dev = [k.t(t.clone()) for t in (p0, g1, m1, v1)]
    tab = table(k, segs)
    k.call("dpc_adam_groups_dev", *dev, n, tab, len(segs), B1, B2, EPS, bc, gscale)
    k.sync()
    p, _, m, v = (t.cpu() for t in dev)
    lr_e, wd_e, act = torch.zeros(n), torch.zeros(n), torch.zeros(n, dtype=torch.bool)
    for b, e, lr, wd, a in segs:
        lr_e[b:e], wd_e[b:e], act[b:e] = lr, wd, bool(a)
    gz = torch.where(act, g1, torch.zeros(()))   # the reference never looks at what a frozen segment or the gap hold
    mz, vz = torch.where(act, m1, torch.zeros(())), torch.where(act, v1, torch.zeros(()))
    p2, m2, v2, bm, bv = adam_f64(p0, gz, mz, vz, lr_e, wd_e, bc_h, gscale)
    bp = 1e-7 * max(1.0, p0.abs().max().item())
    ep = (p.double() - p2.float().double()).abs()[act].max().item()
    em = ((m.double() - m2.float().double()).abs() / bm)[act].max().item()
    ev = ((v.double() - v2.float().double()).abs() / bv)[act].max().item()
    report(f"adam_groups vs f64: p {ep:.3g} (bound {bp:.3g}), m {em:.3g} of its bound, v {ev:.3g} of its bound")
    assert ep <= bp and em <= 1.0 and ev <= 1.0
    # frozen segment and gap: bit-identical before and after, NaNs included; nothing outside the segments moved either
    as_bits = lambda t: t.view(torch.int32)   # noqa: E731
    for new, old in ((p, p0), (m, m1), (v, v1), (dev[1].cpu(), g1)):
        assert torch.equal(as_bits(new)[~act], as_bits(old)[~act])
    assert torch.isnan(m[fb:fe]).all() and torch.isnan(v[fb:fe]).all() and torch.isfinite(p).all()
    ga, gb = sp["gap"]
    assert gb - ga == 3500 and not act[ga:gb].any()
    # lr = 0: the moments moved, the parameter did not
    zb, ze = segs[sp["lr0"]][:2]
    assert torch.equal(p[zb:ze], p0[zb:ze]) and not torch.equal(m[zb:ze], m0[zb:ze]) and not torch.equal(v[zb:ze], v0[zb:ze])
    assert not torch.equal(p[act & (lr_e > 0)], p0[act & (lr_e > 0)])

    # ---- (2) one active segment over the whole arena == dpc_adam_dev on the same inputs, within the same bounds
    lr, wd = PAIRS[0]
    one = [k.t(t.clone()) for t in (p0, g0, m0, v0)]
    k.call("dpc_adam_groups_dev", *one, n, table(k, [(0, n, lr, wd, 1)]), 1, B1, B2, EPS, bc, gscale)
    ref = [k.t(t.clone()) for t in (p0, g0, m0, v0)]
    k.call("dpc_adam_dev", *ref, n, lr, B1, B2, EPS, wd, bc, gscale)
    k.sync()
    _, _, _, bm, bv = adam_f64(p0, g0, m0, v0, torch.full((n,), lr), torch.full((n,), wd), bc_h, gscale)
    dp = (one[0].cpu().double() - ref[0].cpu().double()).abs().max().item()
    dm = ((one[2].cpu().double() - ref[2].cpu().double()).abs() / bm).max().item()
    dv = ((one[3].cpu().double() - ref[3].cpu().double()).abs() / bv).max().item()
    same = all(torch.equal(as_bits(a.cpu()), as_bits(b.cpu())) for a, b in zip(one, ref))
    report(f"adam_groups (one segment) vs dpc_adam_dev: bit-identical = {same}; p {dp:.3g}, m {dm:.3g}, v {dv:.3g} of the bounds")   # reported, not asserted
    assert dp <= bp and dm <= 1.0 and dv <= 1.0

    # ---- (3) the C entry checks pointers and counts
    import pytest
    for bad in (lambda: k.call("dpc_adam_groups_dev", *one, n, tab, 0, B1, B2, EPS, bc, gscale),
                lambda: k.call("dpc_adam_groups_dev", *one, n, tab, L.ADAM_MAX_SEGMENTS + 1, B1, B2, EPS, bc, gscale),
                lambda: k.call("dpc_adam_groups_dev", *one, n, None, 1, B1, B2, EPS, bc, gscale),
                lambda: k.call("dpc_adam_groups_dev", *one, n + 2, tab, len(segs), B1, B2, EPS, bc, gscale)):
        with pytest.raises(L.DpcError, match=f"code {L.ERR_ARG}$"):
            bad()
    return same


def case_table_capacity():
    """the table holds at least as many segments as the resnet34 LC has parameters"""
    from dpc_amd.lc import lc_param_shapes
    assert len(lc_param_shapes("resnet34", 101)) <= L.ADAM_MAX_SEGMENTS
    assert C.sizeof(L.AdamSegment) == 32
