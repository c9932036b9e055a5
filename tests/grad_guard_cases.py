"""The gradient guard (csrc/grad_guard.hip, the _ex entries of csrc/loss.hip, BackboneEngine.set_grad_guard, optim.clip_grad_norm_),
shared by the CPU tier (host SIMT simulator, tests/test_grad_guard_emu.py) and the GPU tier (tests/test_grad_guard_gpu.py).

Bounds, all from the number formats:
  sumsq on integer data : exact (every g^2 and every partial sum is an integer far below 2^53)
  norm                  : one f32 rounding of the f64 value, 2^-23 relative (the f64 accumulation adds n * 2^-53, far below)
  coef                  : the same, of max_norm / (norm + 1e-6) formed in f64
  p / m / v             : those of tests/adam_groups_cases.py
  g * coef              : bit-exact against torch's f32 product
"""
import ctypes as C
import math

import pytest
import torch

import adam_groups_cases as ac
from dpc_amd import _lib as L
from kcases import K

U23 = 2.0 ** -23
B1, B2, EPS = ac.B1, ac.B2, ac.EPS
TILE = ac.TILE
bits = lambda t: t.view(torch.int32)   # noqa: E731


# ------------------------------------------------------------------ the device record
def new_state(k: K, **fields):
    return k.t(torch.frombuffer(bytearray(bytes(L.GradState(**fields))), dtype=torch.uint8).clone())


def read_state(k: K, st) -> L.GradState:
    k.sync()
    return L.GradState.from_buffer_copy(bytes(st.cpu().numpy().tobytes()))


def verdict(k: K, g, tab, nseg, max_norm, skip_nonfinite, st=None, partials=None):
    """dpc_grad_sumsq + dpc_grad_verdict over g; returns (state tensor, GradState, partials on the host)"""
    st = new_state(k) if st is None else st
    partials = k.t(torch.full((L.GRAD_PARTIALS,), float("nan"), dtype=torch.float64)) if partials is None else partials
    k.call("dpc_grad_sumsq", g, g.numel(), tab, nseg, partials)
    k.call("dpc_grad_verdict", partials, L.GRAD_PARTIALS, float(max_norm), int(skip_nonfinite), st)
    return st, read_state(k, st), partials.cpu()


def live_mask(segs, n):
    act = torch.zeros(n, dtype=torch.bool)
    for b, e, _, _, a in segs:
        act[b:e] = bool(a)
    return act


def poisoned_layout(g, segs, sp):
    """NaN in the frozen segment, Inf in the gap: neither may be read"""
    fb, fe = segs[sp["frozen"]][:2]
    ga, gb = sp["gap"]
    g[fb:fe] = float("nan")
    g[ga:gb] = float("inf")
    return g


# ------------------------------------------------------------------ K1
def case_exact_sum(k: K):
    gen = torch.Generator().manual_seed(5)
    segs, n, sp = ac.layout()
    big = (L.GRAD_PARTIALS + 1) * TILE + 8   # one workgroup takes a second tile; the last tile is partial
    layouts = [(8, None, 0, torch.ones(8, dtype=torch.bool)),
               (n, ac.table(k, segs), len(segs), live_mask(segs, n)),
               (big, None, 0, torch.ones(big, dtype=torch.bool))]
    for n_, tab, nseg, act in layouts:
        g = torch.randint(-3, 4, (n_,), generator=gen).float()
        if tab is not None:
            poisoned_layout(g, segs, sp)
        ref = float((g[act].double() ** 2).sum().item())
        gd = k.t(g)
        _, s1, p1 = verdict(k, gd, tab, nseg, 0.0, 1)
        _, s2, p2 = verdict(k, gd, tab, nseg, 0.0, 1)
        assert s1.sumsq == ref and s1.skip == 0, (n_, s1.sumsq, ref)
        assert torch.equal(p1.view(torch.int64), p2.view(torch.int64)) and s2.sumsq == s1.sumsq   # every slot written, the same bits
        assert float(p1.sum().item()) == ref
        assert torch.equal(bits(gd.cpu()), bits(g))   # the gradient is only read


# ------------------------------------------------------------------ K2
def case_rounding(k: K, report=print):
    segs, n, sp = ac.layout()
    tab, act = ac.table(k, segs), live_mask(segs, n)
    g = poisoned_layout(torch.randn(n, generator=torch.Generator().manual_seed(6)), segs, sp)
    ref = math.sqrt((g[act].double() ** 2).sum().item())
    _, s, _ = verdict(k, k.t(g), tab, len(segs), 0.0, 1)
    report(f"grad norm vs f64: {abs(s.norm - ref) / ref:.3g} relative (bound {U23:.3g})")
    assert abs(s.norm - ref) <= U23 * ref and s.skip == 0 and s.coef == 1.0
    # (2e19)^2 overflows f32, not f64
    h = torch.full((8,), 2e19)
    ref = math.sqrt((h.double() ** 2).sum().item())
    _, s, _ = verdict(k, k.t(h), None, 0, 0.0, 1)
    assert math.isfinite(s.norm) and abs(s.norm - ref) <= U23 * ref and s.skip == 0 and s.n_skipped == 0


# ------------------------------------------------------------------ K3
def case_verdict_table(k: K):
    g = torch.randn(4096 + 64, generator=torch.Generator().manual_seed(7))
    norm = math.sqrt((g.double() ** 2).sum().item())
    gd = k.t(g)
    _, s, _ = verdict(k, gd, None, 0, 2.0 * norm, 1)                    # norm < max_norm
    assert s.coef == 1.0 and s.skip == 0 and s.n_clipped == 0 and s.n_skipped == 0
    _, s, _ = verdict(k, gd, None, 0, 0.5 * norm, 1)                    # norm > max_norm
    want = 0.5 * norm / (norm + 1e-6)
    assert abs(s.coef - want) <= U23 * want and s.coef < 1.0 and s.skip == 0 and s.n_clipped == 1
    _, s, _ = verdict(k, gd, None, 0, 0.0, 1)                           # max_norm = 0
    assert s.coef == 1.0 and s.n_clipped == 0
    for bad in (float("nan"), float("inf"), float("-inf")):
        h = g.clone()
        h[1234] = bad
        _, s, _ = verdict(k, k.t(h), None, 0, 0.5 * norm, 1)            # guard on
        assert s.skip == 1 and s.coef == 0.0 and s.n_skipped == 1 and s.n_clipped == 0
        assert not math.isfinite(s.sumsq)
        _, s, _ = verdict(k, k.t(h), None, 0, 0.5 * norm, 0)            # guard off: the step proceeds as it does today
        assert s.skip == 0 and s.coef == 1.0 and s.n_skipped == 0 and s.n_clipped == 0
    # the counters accumulate over successive calls on one record
    st = new_state(k)
    h = g.clone()
    h[7] = float("nan")
    hd = k.t(h)
    for src, mx in ((gd, 0.5 * norm), (hd, 0.5 * norm), (gd, 2.0 * norm), (gd, 0.25 * norm), (hd, 0.0)):
        _, s, _ = verdict(k, src, None, 0, mx, 1, st=st)
    assert (s.n_clipped, s.n_skipped, s.skip) == (2, 2, 1)
    _, s, _ = verdict(k, gd, None, 0, 0.0, 1, st=st)
    assert (s.n_clipped, s.n_skipped, s.skip, s.coef) == (2, 2, 0, 1.0)


# ------------------------------------------------------------------ K4
def _adam_inputs():
    segs, n, sp = ac.layout()
    gen = torch.Generator().manual_seed(11)
    p0, g0 = torch.randn(n, generator=gen) * 0.5, torch.randn(n, generator=gen)
    m0, v0 = torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 1e-2
    return segs, n, sp, p0, g0, m0, v0


def case_gated_update(k: K, report=print):
    segs, n, sp, p0, g0, m0, v0 = _adam_inputs()
    act = live_mask(segs, n)
    fb, fe = segs[sp["frozen"]][:2]
    g1, m1, v1 = g0.clone(), m0.clone(), v0.clone()
    for t in (g1, m1, v1):
        t[fb:fe] = float("nan")
    tab = ac.table(k, segs)
    gscale = 0.5
    lr, wd = ac.PAIRS[0]
    step, bc = k.t(torch.tensor([2], dtype=torch.int32)), k.t(torch.ones(2))
    k.call("dpc_step_advance", step, bc, B1, B2)
    k.sync()
    bc_h = bc.cpu()

    def grouped(state, g=g1):
        dev = [k.t(t.clone()) for t in (p0, g, m1, v1)]
        if state is None:
            k.call("dpc_adam_groups_dev", *dev, n, tab, len(segs), B1, B2, EPS, bc, gscale)
        else:
            k.call("dpc_adam_groups_dev_ex", *dev, n, tab, len(segs), B1, B2, EPS, bc, gscale, state)
        k.sync()
        return [t.cpu() for t in dev]

    def plain(state, g=g0):
        dev = [k.t(t.clone()) for t in (p0, g, m0, v0)]
        if state is None:
            k.call("dpc_adam_dev", *dev, n, lr, B1, B2, EPS, wd, bc, gscale)
        else:
            k.call("dpc_adam_dev_ex", *dev, n, lr, B1, B2, EPS, wd, bc, gscale, state)
        k.sync()
        return [t.cpu() for t in dev]

    def untouched(out, g):   # (iv) the frozen segment and the gap keep their bits in all four arenas
        for new, old in zip(out, (p0, g, m1, v1)):
            assert torch.equal(bits(new)[~act], bits(old)[~act])

    # (i) coef 1, skip 0: the bits of the plain entries
    one = new_state(k, coef=1.0)
    for a, b in zip(grouped(one), grouped(None)):
        assert torch.equal(bits(a), bits(b))
    for a, b in zip(plain(one), plain(None)):
        assert torch.equal(bits(a), bits(b))
    untouched(grouped(one), g1)

    # (ii) coef 0.25: an f64 Adam with gscale * coef
    coef = 0.25
    quarter = new_state(k, coef=coef)
    lr_e, wd_e = torch.zeros(n), torch.zeros(n)
    for b, e, lr_s, wd_s, _ in segs:
        lr_e[b:e], wd_e[b:e] = lr_s, wd_s
    bp = 1e-7 * max(1.0, p0.abs().max().item())
    zero = torch.zeros(())
    for out, ref_in, sel in ((grouped(quarter), (p0, torch.where(act, g1, zero), torch.where(act, m1, zero), torch.where(act, v1, zero), lr_e, wd_e), act),
                             (plain(quarter), (p0, g0, m0, v0, torch.full((n,), lr), torch.full((n,), wd)), torch.ones(n, dtype=torch.bool))):
        p2, m2, v2, bm, bv = ac.adam_f64(*ref_in, bc_h, gscale * coef)
        p, _, m, v = out
        ep = (p.double() - p2.float().double()).abs()[sel].max().item()
        em = ((m.double() - m2.float().double()).abs() / bm)[sel].max().item()
        ev = ((v.double() - v2.float().double()).abs() / bv)[sel].max().item()
        report(f"adam _ex, coef 0.25, vs f64: p {ep:.3g} (bound {bp:.3g}), m {em:.3g} of its bound, v {ev:.3g} of its bound")
        assert ep <= bp and em <= 1.0 and ev <= 1.0
    untouched(grouped(quarter), g1)
    assert not torch.equal(grouped(quarter)[0], grouped(one)[0])

    # (iii) skip 1 with NaN in a live gradient: p, m, v, the step and the bias corrections keep their bits
    skip = new_state(k, coef=0.0, skip=1)
    gn = g1.clone()
    gn[segs[0][0]] = float("nan")
    out = grouped(skip, gn)
    for new, old in zip(out, (p0, gn, m1, v1)):
        assert torch.equal(bits(new), bits(old))
    gn0 = g0.clone()
    gn0[5] = float("nan")
    for new, old in zip(plain(skip, gn0), (p0, gn0, m0, v0)):
        assert torch.equal(bits(new), bits(old))
    step_b, bc_b = step.cpu().clone(), bc.cpu().clone()
    k.call("dpc_step_advance_gated", step, bc, B1, B2, skip)
    k.sync()
    assert torch.equal(step.cpu(), step_b) and torch.equal(bits(bc.cpu()), bits(bc_b))
    k.call("dpc_step_advance_gated", step, bc, B1, B2, one)
    k.sync()
    assert int(step.cpu()) == int(step_b) + 1 == 4
    assert abs(bc.cpu()[0].item() - (1 - B1 ** 4)) < 1e-7 and abs(bc.cpu()[1].item() - (1 - B2 ** 4)) < 1e-7


# ------------------------------------------------------------------ K5
def case_grad_scale(k: K):
    segs, n, sp = ac.layout()
    tab, act = ac.table(k, segs), live_mask(segs, n)
    g = poisoned_layout(torch.randn(n, generator=torch.Generator().manual_seed(8)), segs, sp)
    coef = 0.3
    cf = torch.tensor(coef, dtype=torch.float32)
    for tab_, nseg, live, src in ((tab, len(segs), act, g), (None, 0, torch.ones(n, dtype=torch.bool), torch.where(act, g, torch.ones(())))):
        gd = k.t(src.clone())
        k.call("dpc_grad_scale", gd, n, tab_, nseg, new_state(k, coef=coef))
        k.sync()
        out = gd.cpu()
        assert torch.equal(bits(out)[live], bits(src * cf)[live])        # the f32 product, bit for bit
        assert torch.equal(bits(out)[~live], bits(src)[~live])           # dead floats untouched
        gd = k.t(src.clone())
        k.call("dpc_grad_scale", gd, n, tab_, nseg, new_state(k, coef=0.0, skip=1))
        k.sync()
        assert torch.equal(bits(gd.cpu()), bits(src))                    # skip: untouched


# ------------------------------------------------------------------ K6
def case_argument_checks(k: K):
    segs, n, _ = ac.layout()
    tab = ac.table(k, segs)
    g = k.t(torch.zeros(n + 4))
    part = k.t(torch.zeros(L.GRAD_PARTIALS, dtype=torch.float64))
    st = new_state(k, coef=1.0)
    four = [k.t(torch.zeros(n + 4)) for _ in range(4)]
    step, bc = k.t(torch.zeros(1, dtype=torch.int32)), k.t(torch.ones(2))
    S = len(segs)
    bad = [
        lambda: k.call("dpc_grad_sumsq", None, n, tab, S, part),
        lambda: k.call("dpc_grad_sumsq", g, n, tab, S, None),
        lambda: k.call("dpc_grad_sumsq", g, n + 2, tab, S, part),
        lambda: k.call("dpc_grad_sumsq", g[1:], n, tab, S, part),
        lambda: k.call("dpc_grad_sumsq", g, n, tab, 0, part),
        lambda: k.call("dpc_grad_sumsq", g, n, tab, L.ADAM_MAX_SEGMENTS + 1, part),
        lambda: k.call("dpc_grad_verdict", None, L.GRAD_PARTIALS, 1.0, 1, st),
        lambda: k.call("dpc_grad_verdict", part, L.GRAD_PARTIALS, 1.0, 1, None),
        lambda: k.call("dpc_grad_verdict", part, 0, 1.0, 1, st),
        lambda: k.call("dpc_grad_verdict", part, L.GRAD_PARTIALS + 1, 1.0, 1, st),
        lambda: k.call("dpc_step_advance_gated", step, bc, B1, B2, None),
        lambda: k.call("dpc_step_advance_gated", None, bc, B1, B2, st),
        lambda: k.call("dpc_grad_scale", None, n, tab, S, st),
        lambda: k.call("dpc_grad_scale", g, n, tab, S, None),
        lambda: k.call("dpc_grad_scale", g, n + 2, tab, S, st),
        lambda: k.call("dpc_grad_scale", g[1:], n, tab, S, st),
        lambda: k.call("dpc_grad_scale", g, n, tab, 0, st),
        lambda: k.call("dpc_grad_scale", g, n, tab, L.ADAM_MAX_SEGMENTS + 1, st),
        lambda: k.call("dpc_adam_groups_dev_ex", *four, n, tab, 0, B1, B2, EPS, bc, 1.0, st),
        lambda: k.call("dpc_adam_groups_dev_ex", *four, n, tab, L.ADAM_MAX_SEGMENTS + 1, B1, B2, EPS, bc, 1.0, st),
        lambda: k.call("dpc_adam_groups_dev_ex", *four, n, None, 1, B1, B2, EPS, bc, 1.0, st),
        lambda: k.call("dpc_adam_groups_dev_ex", *four, n + 2, tab, S, B1, B2, EPS, bc, 1.0, st),
        lambda: k.call("dpc_adam_groups_dev_ex", four[0][1:], *four[1:], n, tab, S, B1, B2, EPS, bc, 1.0, st),
        lambda: k.call("dpc_adam_dev_ex", None, *four[1:], n, 1e-3, B1, B2, EPS, 0.0, bc, 1.0, st),
    ]
    for f in bad:
        with pytest.raises(L.DpcError, match=f"code {L.ERR_ARG}$"):
            f()
    assert C.sizeof(L.GradState) == 32 and L.GradState.norm.offset == 8 and L.GradState.n_clipped.offset == 24


# ====================================================================== engine, module boundary, entries
from dataclasses import dataclass   # noqa: E402
from typing import Any, Sequence   # noqa: E402


@dataclass
class Cfg:
    """where the engine cases run: the simulator at WIDTHS, or the HIP device at the reference's widths"""
    device: str
    simulator: Any
    widths: Sequence[int]
    size: int = 64
    B: int = 2
    N: int = 4
    SL: int = 5
    P: int = 1


def f64_norm(g, mask=None):
    g = g.detach().cpu().double()
    return math.sqrt(((g if mask is None else g[mask]) ** 2).sum().item())


def dpc_engine(cfg: Cfg, dtype=torch.float32):
    from dpc_amd.engine import DPCEngine
    from oracle import dpc_oracle as O
    eng = DPCEngine("resnet18", cfg.size, cfg.N, cfg.SL, cfg.P, cfg.B, cfg.device, dtype, cfg.widths, lib=cfg.simulator)
    eng.load_params(O.make_params_pcg("resnet18", cfg.widths))
    return eng


def dpc_input(cfg: Cfg):
    from oracle import dpc_oracle as O
    return O.make_input_pcg(cfg.B, cfg.N, cfg.SL, cfg.size).to(cfg.device)


def arenas(eng):
    return [t.detach().clone() for t in (eng.flat_p, eng.flat_m, eng.flat_v, eng.dev_step, eng.dev_bc)]


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


_TWINS = {}


def twin(cfg: Cfg, dtype=torch.float32):
    """the unguarded twin, computed once per configuration and never changed afterwards: p0 and, after each of two train steps, the
    gradient and the arenas"""
    key = (cfg.device, tuple(cfg.widths), dtype)
    if key not in _TWINS:
        eng, x = dpc_engine(cfg, dtype), dpc_input(cfg)
        rec = {"p0": eng.flat_p.detach().clone(), "steps": []}
        for _ in range(2):
            eng.train_step(x)
            rec["steps"].append({"g": eng.flat_g.detach().clone(), "arenas": arenas(eng)})
        assert eng.grad_guard is None and eng._guard_state is None   # guard off: nothing allocated, today's launches
        _TWINS[key] = rec
    return _TWINS[key]


def case_guard_that_never_bites(cfg: Cfg, dtype=torch.float32):   # E1
    ref = twin(cfg, dtype)
    eng, x = dpc_engine(cfg, dtype), dpc_input(cfg)
    eng.set_grad_guard(max_norm=1e30, skip_nonfinite=True)
    for _ in range(2):
        eng.train_step(x)
    assert same_bits(arenas(eng), ref["steps"][1]["arenas"]) and int(eng.dev_step.item()) == 2 == eng.step_count
    st = eng.grad_stats()
    want = f64_norm(ref["steps"][1]["g"])
    assert abs(st["norm"] - want) <= U23 * want and st["coef"] == 1.0 and (st["skip"], st["n_skipped"], st["n_clipped"]) == (0, 0, 0)
    assert st["sumsq"] == pytest.approx(want * want, rel=1e-12)


def case_clip(cfg: Cfg, report=print):   # E2
    ref = twin(cfg)
    n0 = f64_norm(ref["steps"][0]["g"])
    eng, x = dpc_engine(cfg), dpc_input(cfg)
    eng.set_grad_guard(max_norm=n0 / 2)
    eng.train_step(x)
    st = eng.grad_stats()
    want = (n0 / 2) / (n0 + 1e-6)
    assert abs(st["coef"] - want) <= U23 * want and st["n_clipped"] == 1 and st["skip"] == 0 and abs(st["norm"] - n0) <= U23 * n0
    assert torch.equal(eng.flat_g.view(torch.int32), ref["steps"][0]["g"].view(torch.int32))   # the factor lives in the update: g is not rewritten
    n = eng.numel
    p0 = ref["p0"].cpu()
    p2, _, _, _, _ = ac.adam_f64(p0, eng.flat_g.cpu(), torch.zeros(n), torch.zeros(n), torch.full((n,), eng.lr), torch.full((n,), eng.wd),
                                 eng.dev_bc.cpu(), want)
    err, bound = (eng.flat_p.cpu().double() - p2).abs().max().item(), 1e-7 * max(1.0, p0.abs().max().item())
    report(f"clipped step vs f64 Adam on g * coef: {err:.3g} (bound {bound:.3g})")
    assert err <= bound
    assert not torch.equal(eng.flat_p, ref["steps"][0]["arenas"][0])   # ... and it did clip


def case_skip(cfg: Cfg, dtype=torch.float32):   # E3
    from dpc_amd import checkpoint as ckpt
    eng, x = dpc_engine(cfg, dtype), dpc_input(cfg)
    eng.set_grad_guard(skip_nonfinite=True)
    before = arenas(eng)
    eng._forward_loss(x, True)
    eng.backward()
    o, _ = eng.offsets["backbone.layer2.0.conv1.weight"]
    eng.flat_g[o + 5] = float("nan")
    eng.adam_step()
    assert same_bits(arenas(eng), before) and int(eng.dev_step.item()) == 0
    st = eng.grad_stats()
    assert (st["skip"], st["n_skipped"], st["coef"]) == (1, 1, 0.0)
    eng.train_step(x)
    after = arenas(eng)
    assert int(eng.dev_step.item()) == 1 and not torch.equal(after[0], before[0]) and after[1].abs().max().item() > 0
    assert eng.grad_stats()["skip"] == 0 and eng.grad_stats()["n_skipped"] == 1
    state = ckpt.build_state(eng, 1, "resnet18", 0.0, 2)
    assert float(state["optimizer"]["state"][0]["step"]) == 1.0 and eng.step_count == 1   # two attempts, one optimizer step
    assert torch.isfinite(eng.flat_p).all()
    with pytest.raises(ValueError):
        eng.set_grad_guard(max_norm=0.0)
    with pytest.raises(ValueError):
        eng.set_grad_guard(max_norm=float("inf"))
    eng.set_grad_guard()
    assert eng.grad_guard is None


def lc_engine(cfg: Cfg, num_class: int):
    from dpc_amd.lc import LCEngine
    from oracle import dpc_oracle as O
    eng = LCEngine("resnet18", cfg.size, cfg.N, cfg.SL, cfg.B, cfg.device, torch.float32, cfg.widths, lib=cfg.simulator, num_class=num_class)
    eng.load_params(O.make_lc_params_pcg("resnet18", num_class, cfg.widths))
    return eng


def case_groups(cfg: Cfg, num_class: int = 11):   # E4
    eng, x = lc_engine(cfg, num_class), dpc_input(cfg)
    head = [k for k in eng.offsets if k.startswith(("final_bn.", "final_fc."))]   # lc_main --train_what head
    eng.set_param_groups([{"params": head, "lr": 1e-3, "weight_decay": 1e-3}])
    eng.set_grad_guard(max_norm=1e30, skip_nonfinite=True)
    target = (torch.arange(cfg.B) % num_class).to(cfg.device)
    eng.forward(x, target, train=True)
    eng.backward()
    o, n = eng.offsets["backbone.layer1.0.conv1.weight"]
    eng.flat_g[o:o + n] = float("nan")   # a frozen parameter's slot: not the guard's business
    live = torch.zeros(eng.numel, dtype=torch.bool)
    for k in head:
        ko, kn = eng.offsets[k]
        live[ko:ko + kn] = True
    want = f64_norm(eng.flat_g, live)
    p_before = eng.flat_p.detach().clone()
    eng.adam_step()
    st = eng.grad_stats()
    assert st["skip"] == 0 and st["n_skipped"] == 0 and want > 0 and abs(st["norm"] - want) <= U23 * want
    assert int(eng.dev_step.item()) == 1 and not torch.equal(eng.flat_p[live.to(cfg.device)], p_before[live.to(cfg.device)])
    assert torch.equal(eng.flat_p[~live.to(cfg.device)], p_before[~live.to(cfg.device)])


def case_captured_step(cfg: Cfg):   # E5, HIP device only
    x = dpc_input(cfg)
    nan_x = torch.full_like(x, float("nan"))
    a, b = dpc_engine(cfg), dpc_engine(cfg)
    for e in (a, b):
        e.set_grad_guard(max_norm=1e30, skip_nonfinite=True)
        for _ in range(2):   # eager steps size every lazy buffer; both engines take them
            e.train_step(x)
    block = x.clone()
    replay = a.capture_train_step(block, warmup=0)
    replay()
    after1 = arenas(a)
    block.copy_(nan_x)
    replay()
    assert same_bits(arenas(a), after1)
    block.copy_(x)
    replay()
    for inp in (x, nan_x, x):
        b.train_step(inp)
    assert same_bits(arenas(a), arenas(b)) and not same_bits(arenas(a), after1)
    sa, sb = a.grad_stats(), b.grad_stats()
    assert sa["n_skipped"] == 1 == sb["n_skipped"] and sa["skip"] == 0 and sa == sb
    assert a.step_count == 4 == int(a.dev_step.item())
    a.set_grad_guard(max_norm=3.0, skip_nonfinite=True)
    with pytest.raises(RuntimeError):
        replay()
    a.set_grad_guard(max_norm=1e30, skip_nonfinite=True)
    a.release_captures()


def case_module_boundary(cfg: Cfg, num_class: int = 11, report=print):   # M1
    import lc_loop_cases as lc
    from dpc_amd.optim import Adam, clip_grad_norm_
    c = lc.Cfg(device=cfg.device, simulator=cfg.simulator, widths=cfg.widths, num_class=num_class, size=cfg.size, B=cfg.B, N=cfg.N, SL=cfg.SL)
    m = lc.module(c, pcg=True)
    m._forced_masks = lc.masks(c)[0]
    x = dpc_input(cfg)
    target = (torch.arange(cfg.B) % num_class).to(cfg.device)
    out, _ = m(x)
    m.zero_grad()
    torch.nn.functional.cross_entropy(out.view(cfg.B, -1), target).backward()
    params = [q for q in m.parameters() if q.grad is not None]
    assert params
    g0 = [q.grad.detach().cpu().double().clone() for q in params]
    n0 = math.sqrt(sum((g ** 2).sum().item() for g in g0))
    eng = m.engine
    snap = [t.detach().clone() for t in (eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v)]
    # clip_grad_norm_: torch's contract
    norm = clip_grad_norm_(params, n0 / 2)
    assert norm.dim() == 0 and norm.dtype == torch.float32 and norm.device.type == torch.device(cfg.device).type
    assert abs(norm.item() - n0) <= U23 * n0
    coef = (n0 / 2) / (n0 + 1e-6)
    worst = 0.0
    for q, g in zip(params, g0):
        want = g * coef
        err = ((q.grad.detach().cpu().double() - want).abs() - 4 * 2.0 ** -24 * want.abs()).max().item()
        worst = max(worst, err)
    report(f"clip_grad_norm_: norm {norm.item():.6g} (f64 {n0:.6g}); worst excess over 4 u |g coef|: {worst:.3g}")
    assert worst <= 0.0
    big = clip_grad_norm_(params, 1e30)   # no clip: the gradients keep their bits
    g1 = [q.grad.detach().clone() for q in params]
    assert abs(big.item() - n0 * coef) <= 2 * U23 * n0 * coef
    clip_grad_norm_(params, 1e30)
    assert all(torch.equal(q.grad.view(torch.int32), g.view(torch.int32)) for q, g in zip(params, g1))
    other = lc.module(c, seed=5)
    with pytest.raises(RuntimeError):
        clip_grad_norm_(params + [next(other.parameters())], 1.0)
    with pytest.raises(RuntimeError):
        clip_grad_norm_([next(other.parameters())], 1.0)
    # Adam(max_grad_norm=...) == the engine's guarded step (E2) from the same engine state, bit for bit
    def restore():
        for t, s in zip((eng.flat_p, eng.flat_g, eng.flat_m, eng.flat_v), snap):
            t.copy_(s)
        eng.step_count = 0
    restore()
    opt = Adam(m.parameters(), lr=1e-3, weight_decay=1e-3, max_grad_norm=n0 / 2)
    opt.step()
    via_optim = arenas(eng)
    st = eng.grad_stats()
    assert abs(st["coef"] - coef) <= U23 * coef and st["n_clipped"] == 1
    restore()
    eng.set_grad_guard()
    groups, lr, wd = eng.param_groups, eng.lr, eng.wd
    eng.set_grad_guard(max_norm=n0 / 2)
    assert (eng.param_groups, eng.lr, eng.wd) == (groups, lr, wd)
    eng.adam_step()
    assert same_bits(arenas(eng), via_optim) and not torch.equal(eng.flat_p, snap[0])
    with pytest.raises(ValueError):
        Adam(m.parameters(), max_grad_norm=-1.0)


# ---------------------------------------------------------------------- entries (simulator)
def case_entries(emu, widths, capsys):   # C1
    from dpc_amd import lc_main, main as dpc_main
    common = ["--net", "resnet18", "--img_dim", "64", "--batch_size", "1", "--gpu", "0", "--synthetic", "1", "--print_freq", "1",
              "--dtype", "f32", "--num_seq", "4", "--epochs", "1"]
    flags = ["--clip_grad", "1.0", "--skip_nonfinite"]
    import re
    for entry, extra in ((dpc_main, ["--pred_step", "1"]), (lc_main, ["--train_what", "head"])):
        entry.main(common + extra + flags, _simulator=emu, _widths=widths)
        out = capsys.readouterr().out
        line = [ln for ln in out.splitlines() if ln.startswith("Epoch: [0][0/1]")]
        assert len(line) == 1 and re.search(r" gnorm \d+\.\d{4}$", line[0]), out
        assert float(line[0].rsplit(" ", 1)[1]) > 0
        assert re.search(r"^Grad guard: 0 skipped, [01] clipped of 1 steps$", out, re.M), out
        entry.main(common + extra, _simulator=emu, _widths=widths)
        out = capsys.readouterr().out
        assert "Epoch: [0][0/1]" in out and " gnorm " not in out and "Grad guard:" not in out


def case_two_ranks(emu, widths, tmp_path):   # C2
    import os
    from dpc_amd import main as dpc_main
    pr = str(tmp_path / "probe")
    os.makedirs(pr)
    dpc_main.main(["--net", "resnet18", "--img_dim", "64", "--batch_size", "2", "--gpu", "0,1", "--synthetic", "2", "--print_freq", "1",
                   "--dtype", "f32", "--num_seq", "4", "--pred_step", "1", "--epochs", "1", "--clip_grad", "1.0", "--skip_nonfinite"],
                  _simulator=emu, _widths=widths, _probe=pr)
    r = [torch.load(os.path.join(pr, f"rank{i}.pt")) for i in range(2)]
    assert torch.equal(r[0]["flat_p"], r[1]["flat_p"]) and torch.equal(r[0]["flat_m"], r[1]["flat_m"])
    assert all(x["step"] == 2 for x in r) and torch.isfinite(r[0]["flat_p"]).all() and r[0]["flat_m"].abs().sum() > 0
