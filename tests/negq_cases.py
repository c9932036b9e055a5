"""The negative queue (csrc/neg_queue.hip: dpc_negq_push / _clear / _fwd / _bwd; csrc/loss.hip: dpc_ce_topk_ext / dpc_ce_topk_bf16_ext;
DPCEngine.set_neg_queue; main --neg_queue), shared by the CPU tier (host SIMT simulator, tests/test_negq_emu.py) and the GPU tier
(tests/test_negq_gpu.py).

Kernel data is exact by construction, as loss_cases.score_data does it: pred and every key hold entries from {0, +-1/2}, a pred row at
most four of them, so every logit is a multiple of 1/4 with |s| <= 1, exact under any accumulation order: max, rank and every
comparison are integer facts and the only rounding left is that of exp, the sums and log.

Bounds (no tolerance constants):
  push             bit identity of the whole ring, guard bands included; the record
  forward m, rk    equality with the f64 reference
  forward l        QUARTER (loss_cases) of what dropping the lightest live column changes: exp(s_min - m)
  _ext CE, empty   bit identity to dpc_ce_topk / dpc_ce_topk_bf16
  _ext CE, bank    loss term: QUARTER * -log1p(-p_min), p_min the lightest of the R + Q columns; rank: equality; f32 gradient element:
                   relative QUARTER * p_min; bf16 gradient element: relative 2^-8 (loss_cases); lse_out: the loss bound plus one f32
                   spacing
  backward         |out - ref|_id <= (2^-8 + N 2^-24) sum_c |dS_ic q_cd|: 2^-8 is the bf16 rounding of dS (half an ulp, 2^-9, and the
                   same again for an f32 value on the other side of a rounding boundary), N the number of f32 roundings an output
                   element goes through, counted from negq_bwd_kernel: at most one per product accumulated on the matrix cores (the
                   live columns, padded to whole 64-column tiles) plus one per slab summed by dpc_reduce_unpack
Dead slots, the rows >= R of a slot and the columns >= R of a transposed slot hold NaN in every kernel case: results are finite and
bit-identical to the same call on a ring that holds zeros there."""
import ctypes as C
import functools
import os
import re
import warnings
from collections import namedtuple

import numpy as np
import pytest
import torch

import grad_guard_cases as gc
import kcases as kc
import loss_cases as lc
from dpc_amd import _lib as L
from kcases import K

F32, BF16 = torch.float32, torch.bfloat16
QUARTER, GUARD = lc.QUARTER, lc.GUARD
EMPTY = (-1.0e30, 0.0, 0.0)
Cfg = gc.Cfg
bits = lc._bits
_t = lc._t

KERNEL_SHAPES = ((24, 32, 3), (200, 32, 2), (264, 32, 2), (136, 256, 2), (520, 32, 3))   # (R, D, K)
KERNEL_SHAPES_GPU = KERNEL_SHAPES + ((1100, 256, 4),)


def pitch_of(R):
    return L.negq_pitch(R)


# ---------------------------------------------------------------------------------------------------------------- data
Bank = namedtuple("Bank", "sd keys R D K")


@functools.lru_cache(maxsize=None)
def bank_data(R, D, K):
    """score_data(R, D) (pred, the in-batch keys, S) and K batches of bank keys with entries from {0, +-1/2}.  Planted in the bank for the
    row planted[n] of score_data (pred = p_n on four features, target logit 3/4): n keys equal to p_n (logit 1: above the target), spread
    over the slots at the ends and tile seams of a slot, and in every slot one copy of the row's own in-batch key (logit 3/4: a tie with
    the target, never counted).  Computed once, never written to."""
    sd = lc.score_data(R, D)
    rng = np.random.Generator(np.random.PCG64(11 * R + D + K))
    keys = np.zeros((K, R, D))
    for k in range(K):
        for i in range(R):
            nn = int(rng.integers(1, 5))
            keys[k, i, rng.choice(D, nn, replace=False)] = rng.choice([-0.5, 0.5], nn)
    seams = [c for c in (R - 1, 0, 63, 64, R - 2, 1, 65, 62) if 0 <= c < R]
    spots = [(k, c) for c in seams for k in range(K)]    # (slot, row) for the planted keys, no spot twice
    used = set()

    def take():
        while True:
            s = spots.pop(0) if spots else (int(rng.integers(0, K)), int(rng.integers(0, R)))
            if s not in used:
                used.add(s)
                return s
    for n, row in enumerate(sd.planted):
        for _ in range(n):
            k, c = take()
            keys[k, c] = sd.pred[row]
        for k in range(K):   # the tie
            while True:
                c = int(rng.integers(0, R))
                if (k, c) not in used:
                    used.add((k, c))
                    break
            keys[k, c] = sd.finf[row]
    keys.setflags(write=False)
    return Bank(sd, keys, R, D, K)


Ref = namedtuple("Ref", "Sq m l rk lbound")


def queue_ref(bank: Bank, slots):
    """f64 statistics of pred against the keys of the given slots (live, in any order)"""
    sd = bank.sd
    tgt = np.diagonal(sd.S)
    if not slots:
        R = bank.R
        return Ref(np.zeros((R, 0)), np.full(R, EMPTY[0]), np.zeros(R), np.zeros(R), np.zeros(R))
    Q = np.concatenate([bank.keys[k] for k in slots], 0)
    Sq = sd.pred @ Q.T
    assert np.abs(Sq).max() <= 1.0 and np.array_equal(Sq * 4, np.round(Sq * 4))
    m = Sq.max(1)
    e = np.exp(Sq - m[:, None])
    return Ref(Sq, m, e.sum(1), (Sq > tgt[:, None]).sum(1).astype(np.float64), QUARTER * e.min(1))


def make_ring(k: K, bank: Bank, live, fill=float("nan"), guard=GUARD):
    """device ring and transposed ring with the keys of the slots in `live` in place and `fill` everywhere else: dead slots, the rows
    >= R of a slot, the columns >= R of a transposed slot, and a guard band behind each allocation"""
    R, D, Kk = bank.R, bank.D, bank.K
    pitch = pitch_of(R)
    ring = torch.full((Kk * pitch * D + guard,), fill, dtype=BF16)
    ringT = torch.full((Kk * D * pitch + guard,), fill, dtype=BF16)
    rv, tv = ring[:Kk * pitch * D].view(Kk, pitch, D), ringT[:Kk * D * pitch].view(Kk, D, pitch)
    for s in live:
        q = _t(bank.keys[s]).to(BF16)
        rv[s, :R] = q
        tv[s, :, :R] = q.t()
    return k.t(ring), k.t(ringT)


def make_state(k: K, pushes, filled):
    return k.t(torch.tensor([pushes, filled, 0, 0], dtype=torch.int32))


def ws_sizes(k: K, R, D, Kk):
    nf, nb = C.c_int64(0), C.c_int64(0)
    n = k.lib.call("dpc_negq_ws_floats", R, D, Kk, C.byref(nf), C.byref(nb))
    assert n >= 1 and nf.value >= 4 * R and nb.value == n * R * D
    return nf.value, nb.value, n


def target_of(k: K, bank: Bank, dtype):
    """the target logits where the in-batch path keeps them: the diagonal of an [R][R] matrix of logits, NaN off the diagonal"""
    R = bank.R
    m = torch.full((R, R), float("nan"), dtype=dtype)
    m[torch.arange(R), torch.arange(R)] = _t(np.diagonal(bank.sd.S).copy()).to(dtype)
    return k.t(m)


def states_of(Kk):
    """(pushes, filled, live slots): empty, one slot, and a full bank after a wrap"""
    return [(0, 0, []), (1, 1, [0]), (Kk + 1, Kk, list(range(Kk)))] + ([(2, 2, [0, 1])] if Kk > 2 else [])


# ---------------------------------------------------------------------------------------------------------------- K1 push
def case_push(k: K, R, D, Kk):
    pitch, ldT = pitch_of(R), (R + 7) // 8 * 8
    rng = torch.Generator().manual_seed(3 * R + Kk)
    ring = torch.full((Kk * pitch * D + GUARD,), float("nan"), dtype=BF16)
    ringT = torch.full((Kk * D * pitch + GUARD,), float("nan"), dtype=BF16)
    dring, dringT, st = k.t(ring), k.t(ringT), make_state(k, 0, 0)
    for n in range(2 * Kk + 2):
        got = st.cpu().tolist()
        assert got[:2] == [n, min(n, Kk)], (n, got)
        assert torch.equal(bits(dring), bits(ring)) and torch.equal(bits(dringT), bits(ringT)), f"after {n} pushes"
        batch = torch.randn((R, D), generator=rng).to(BF16)
        finfT = torch.zeros((D, ldT), dtype=BF16)
        finfT[:, :R] = batch.t()
        k.call("dpc_negq_push", k.t(batch), k.t(finfT), ldT, dring, dringT, st, R, D, Kk)
        k.sync()
        s = n % Kk
        ring[:Kk * pitch * D].view(Kk, pitch, D)[s, :R] = batch            # the live rows; rows >= R stay what they were
        ringT[:Kk * D * pitch].view(Kk, D, pitch)[s, :, :ldT] = finfT      # columns [R, ldT) are finfT's zeros
    assert st.cpu().tolist()[:2] == [2 * Kk + 2, Kk]
    assert torch.equal(bits(dring), bits(ring)) and torch.equal(bits(dringT), bits(ringT))
    # clear: only on a guard record that says skip; always without one
    guard = torch.zeros(1, dtype=torch.uint8).repeat(C.sizeof(L.GradState))
    gd = k.t(guard)
    k.call("dpc_negq_clear", st, gd)
    k.sync()
    assert st.cpu().tolist()[:2] == [2 * Kk + 2, Kk]
    rec = L.GradState(skip=1)
    gd = k.t(torch.frombuffer(bytearray(bytes(rec)), dtype=torch.uint8).clone())
    k.call("dpc_negq_clear", st, gd)
    k.sync()
    assert st.cpu().tolist() == [0, 0, 0, 0]
    st = make_state(k, 5, 2)
    k.call("dpc_negq_clear", st, None)
    k.sync()
    assert st.cpu().tolist() == [0, 0, 0, 0]
    assert torch.equal(bits(dring), bits(ring)) and torch.equal(bits(dringT), bits(ringT))   # clearing touches the record alone


# ---------------------------------------------------------------------------------------------------------------- K2 forward
def run_fwd(k: K, bank: Bank, ring, st, tgt, tdt):
    R, D, Kk = bank.R, bank.D, bank.K
    nf, _, _ = ws_sizes(k, R, D, Kk)
    ws, stats = k.poison(nf + GUARD), k.poison(R * 4 + GUARD)
    k.call("dpc_negq_fwd", k.t(_t(bank.sd.pred), BF16), ring, st, R, D, Kk, tgt, R + 1, L.dtype_code(tdt), stats, ws)
    k.sync()
    assert bool(torch.isnan(ws[nf:]).all()) and bool(torch.isnan(stats[R * 4:]).all()), "written past the workspace / the statistics"
    return stats[:R * 4].view(R, 4)


def case_fwd(k: K, R, D, Kk):
    bank = bank_data(R, D, Kk)
    worst = 0.0
    for pushes, filled, live in states_of(Kk):
        ref = queue_ref(bank, live)
        st = make_state(k, pushes, filled)
        ring, _ = make_ring(k, bank, live)
        compact, _ = make_ring(k, bank, live, fill=0.0)
        for tdt in (F32, BF16):
            tgt = target_of(k, bank, tdt)
            got = run_fwd(k, bank, ring, st, tgt, tdt)
            kc.all_finite(got)
            assert torch.equal(bits(got), bits(run_fwd(k, bank, compact, st, tgt, tdt))), "NaN in dead slots / padding rows changes the bits"
            g = got.cpu().numpy().astype(np.float64)
            if not live:
                assert (g[:, 0] == np.float32(EMPTY[0])).all() and (g[:, 1] == 0).all() and (g[:, 2] == 0).all() and (g[:, 3] == 0).all()
                continue
            assert np.array_equal(g[:, 0], ref.m), f"max differs on rows {np.nonzero(g[:, 0] != ref.m)[0][:8].tolist()}"
            assert np.array_equal(g[:, 2], ref.rk), f"rank differs on rows {np.nonzero(g[:, 2] != ref.rk)[0][:8].tolist()}"
            e = np.abs(g[:, 1] - ref.l)
            assert (e < ref.lbound).all(), f"sum-exp of rows {np.nonzero(~(e < ref.lbound))[0][:8].tolist()}"
            worst = max(worst, float((e / ref.lbound).max()))
        if filled == Kk:   # the planted ranks and ties, with every slot live
            for n, row in enumerate(bank.sd.planted):
                assert ref.rk[row] == n and int((ref.Sq[row] == 0.75).sum()) >= Kk, (n, row, ref.rk[row])
    print(f"[negq-fwd] ({R}, {D}, {Kk}): sum-exp at most {worst:.3g} of its bound")
    return worst


# ---------------------------------------------------------------------------------------------------------------- K3 _ext CE
def empty_stats(k: K, rows):
    return k.t(torch.tensor(EMPTY + (0.0,), dtype=F32).repeat(rows, 1))


def case_ext_empty(k: K, entry, name, mode):
    """one shape of loss_cases.CE_SHAPES / CE16_SHAPES: the _ext entry with empty statistics against the older entry, bit for bit.  Modes
    as loss_cases.ce_rows_case: "f32", "bf16"; without a gradient (dscore = NULL, what a validation-style call passes) "null" and, for
    dpc_ce_topk with dtype_d = bf16, "bf16-null"""
    bf_logits = entry == "dpc_ce_topk_bf16"
    cols, ld, ld_d, off = (lc.CE16_SHAPES if bf_logits else lc.CE_SHAPES)[name]
    rc = lc.row_case(cols, 8 if bf_logits else 4, square="square" in name)
    rows = rc.s.shape[0]
    ld, ld_d = ld or cols, ld_d or cols
    keep, sview = lc._strided(k, rc.s, ld, BF16 if bf_logits else F32, off)
    gdt = {"f32": F32, "bf16": BF16}.get(mode)
    code = L.dtype_code(F32 if mode in ("f32", "null") else BF16)
    old, new = lc.Out(k, rows, ld_d, gdt), lc.Out(k, rows, ld_d, gdt)
    lc._launch(k, entry, sview, rows, cols, ld, old, code)
    lse = k.poison(rows + GUARD)
    qs = empty_stats(k, rows)
    if bf_logits:
        k.call(entry + "_ext", sview, rows, cols, ld, new.ws, new.res, new.d, new.ld_d, qs, lse)
    else:
        k.call(entry + "_ext", sview, rows, cols, ld, new.ws, new.res, new.d, code, new.ld_d, qs, lse)
    k.sync()
    assert torch.equal(bits(new.ws), bits(old.ws)) and torch.equal(bits(new.res), bits(old.res)), f"{entry}_ext {name} {mode}: other bits"
    if gdt is not None:
        assert torch.equal(bits(new.dbuf), bits(old.dbuf)), f"{entry}_ext {name} {mode}: other gradient bits"
    want = rc.term + np.diagonal(rc.s[:, :rows])   # lse = loss term + target
    e = np.abs(lse[:rows].cpu().numpy().astype(np.float64) - want)
    assert (e < rc.loss_bound + np.spacing(np.abs(want).astype(np.float32))).all() and bool(torch.isnan(lse[rows:]).all())
    del keep


def case_ext_bank(k: K, R, D, Kk, report=print):
    """the in-batch logits S of score_data (exact in f32 and bf16) with the statistics dpc_negq_fwd forms from a real, full bank"""
    bank = bank_data(R, D, Kk)
    sd = bank.sd
    live = list(range(Kk))
    ref = queue_ref(bank, live)
    ring, _ = make_ring(k, bank, live)
    st = make_state(k, Kk, Kk)
    qs = run_fwd(k, bank, ring, st, target_of(k, bank, F32), F32).contiguous()
    allS = np.concatenate([sd.S, ref.Sq], 1)
    tgt = np.diagonal(sd.S)
    mx = allS.max(1)
    e = np.exp(allS - mx[:, None])
    lse = np.log(e.sum(1)) + mx
    p = e / e.sum(1)[:, None]
    pmin = p.min(1)
    bound = QUARTER * -np.log1p(-pmin)
    rank = (allS > tgt[:, None]).sum(1).astype(np.float64)
    grad = p[:, :R].copy()
    grad[np.arange(R), np.arange(R)] -= 1.0
    grad /= R
    no_bank = np.abs(sd.term - (lse - tgt)) > bound   # the same reference without the bank
    report(f"[negq-ce] ({R}, {D}, {Kk}): the reference without the bank misses the bound on {no_bank.mean():.3f} of the rows")
    assert no_bank.mean() > 0.5
    arms = [("dpc_ce_topk_ext", F32, F32), ("dpc_ce_topk_ext", F32, BF16)] + ([("dpc_ce_topk_bf16_ext", BF16, BF16)] if R % 8 == 0 else [])
    for entry, sdt, gdt in arms:
        E = 8 if gdt == BF16 else 4
        ld_d = (R + E - 1) // E * E
        out = lc.Out(k, R, ld_d, gdt)
        lse_out = k.poison(R + GUARD)
        sdev = k.t(_t(sd.S), sdt)
        if entry == "dpc_ce_topk_ext":
            k.call(entry, sdev, R, R, R, out.ws, out.res, out.d, L.dtype_code(gdt), ld_d, qs, lse_out)
        else:
            k.call(entry, sdev, R, R, R, out.ws, out.res, out.d, ld_d, qs, lse_out)
        k.sync()
        kc.all_finite(out.ws, out.res, lse_out[:R])
        out.guard_untouched()
        w = out.ws.cpu().numpy().astype(np.float64)
        assert np.array_equal(w[:, 1], rank), f"{entry}: rank differs on rows {np.nonzero(w[:, 1] != rank)[0][:8].tolist()}"
        et = np.abs(w[:, 0] - (lse - tgt))
        assert (et < bound).all(), f"{entry}: loss term of rows {np.nonzero(~(et < bound))[0][:8].tolist()}"
        el = np.abs(lse_out[:R].cpu().numpy().astype(np.float64) - lse)
        assert (el < bound + np.spacing(lse.astype(np.float32))).all() and bool(torch.isnan(lse_out[R:]).all())
        r = out.res.cpu().numpy()
        for i, kk in enumerate((1, 3, 5)):
            assert r[1 + i] == np.float32(int((rank < kk).sum())) / np.float32(R)
        assert abs(float(r[0]) - (lse - tgt).mean()) < bound.max()
        g = out.d[:, :R].float().cpu().numpy().astype(np.float64)
        rel = np.abs(g - grad) / np.abs(grad)
        gb = QUARTER * pmin if gdt == F32 else np.full(R, 2.0 ** -8)
        assert (rel.max(1) < gb).all(), f"{entry} {gdt}: gradient rows {np.nonzero(~(rel.max(1) < gb))[0][:8].tolist()}"
        if ld_d > R:
            assert float(out.d[:, R:].float().abs().max()) == 0.0
        report(f"[negq-ce] {entry} ({R}, {D}, {Kk}) {'f32' if gdt == F32 else 'bf16'} gradient: loss {float((et / bound).max()):.3g}, "
               f"gradient {float((rel.max(1) / gb).max()):.3g} of their bounds")


# ---------------------------------------------------------------------------------------------------------------- K4 backward
def run_bwd(k: K, bank: Bank, ring, ringT, st, lse32):
    R, D, Kk = bank.R, bank.D, bank.K
    _, nb, nslab = ws_sizes(k, R, D, Kk)
    ws, out = k.poison(nb + GUARD), k.poison(R * D + GUARD)
    n = k.call("dpc_negq_bwd", k.t(_t(bank.sd.pred), BF16), ring, ringT, st, R, D, Kk, k.t(lse32), ws)
    assert n == nslab
    k.call("dpc_reduce_unpack", ws, n, out, R, 1, D, D, 0, 1, 0)
    k.sync()
    assert bool(torch.isnan(ws[nb:]).all()) and bool(torch.isnan(out[R * D:]).all())
    return out[:R * D].view(R, D), n


def case_bwd(k: K, R, D, Kk, report=print):
    bank = bank_data(R, D, Kk)
    sd = bank.sd
    worst = 0.0
    for pushes, filled, live in states_of(Kk):
        ref = queue_ref(bank, live)
        allS = np.concatenate([sd.S, ref.Sq], 1)
        mx = allS.max(1)
        lse32 = torch.from_numpy((np.log(np.exp(allS - mx[:, None]).sum(1)) + mx).astype(np.float32))   # the kernel's input, as it is
        lse = lse32.numpy().astype(np.float64)
        st = make_state(k, pushes, filled)
        ring, ringT = make_ring(k, bank, live)
        cring, cringT = make_ring(k, bank, live, fill=0.0)
        got, nslab = run_bwd(k, bank, ring, ringT, st, lse32)
        kc.all_finite(got)
        again, _ = run_bwd(k, bank, cring, cringT, st, lse32)
        assert torch.equal(bits(got), bits(again)), "NaN in dead slots / padding changes the bits"
        g = got.cpu().numpy().astype(np.float64)
        if not live:
            assert not bits(got).any(), "an empty bank must give +0 everywhere"
            continue

        def want_of(slots):
            r = queue_ref(bank, slots)
            dS = np.exp(r.Sq - lse[:, None]) / R
            Q = np.concatenate([bank.keys[s] for s in slots], 0)
            return dS @ Q, np.abs(dS) @ np.abs(Q)
        want, mag = want_of(live)
        N = len(live) * pitch_of(R) + nslab   # f32 roundings: one per product at most, one per slab
        bound = (2.0 ** -8 + N * 2.0 ** -24) * mag
        e = np.abs(g - want)
        assert (e <= bound).all(), f"({R}, {D}, {Kk}) filled {filled}: {int((~(e <= bound)).sum())} elements outside the bound"
        worst = max(worst, float((e[mag > 0] / bound[mag > 0]).max()))
        if len(live) > 1:   # the reference with one live slot left out misses the bound
            short, _ = want_of(live[:-1])
            miss = np.abs(g - short) > bound
            report(f"[negq-bwd] ({R}, {D}, {Kk}): the reference without one live slot misses the bound on {miss[mag > 0].mean():.3f} of the elements")
            assert miss[mag > 0].mean() > 0.5
    report(f"[negq-bwd] ({R}, {D}, {Kk}): at most {worst:.3g} of the bound")
    return worst


# ---------------------------------------------------------------------------------------------------------------- K5 refused calls
def case_refused(k: K):
    R, D, Kk = 24, 32, 2
    bank = bank_data(R, D, 3)
    pitch, ldT = pitch_of(R), 24
    ring0 = torch.full((Kk * pitch * D,), float("nan"), dtype=BF16)
    ring, ringT, st = k.t(ring0), k.t(ring0), make_state(k, 1, 1)
    pred, finfT = k.t(_t(bank.sd.pred), BF16), k.zeros(D, ldT, dtype=BF16)
    tgt, lse = k.zeros(R * R), k.zeros(R)
    stats, ws, out = k.poison(R * 4), k.poison(1 << 16), k.poison(4)
    arg, uns = f"code {L.ERR_ARG}$", f"code {L.ERR_UNSUPPORTED}$"
    call = k.call
    bad = [
        (arg, lambda: call("dpc_negq_push", None, finfT, ldT, ring, ringT, st, R, D, Kk)),
        (arg, lambda: call("dpc_negq_push", pred, finfT, ldT, None, ringT, st, R, D, Kk)),
        (arg, lambda: call("dpc_negq_push", pred, finfT, ldT, ring, ringT, None, R, D, Kk)),
        (arg, lambda: call("dpc_negq_push", pred, None, ldT, ring, ringT, st, R, D, Kk)),
        (arg, lambda: call("dpc_negq_push", pred, finfT, ldT, ring, ringT, st, R, D, 0)),
        (arg, lambda: call("dpc_negq_push", pred, finfT, ldT, ring, ringT, st, R, D, L.NEGQ_MAX_SLOTS + 1)),
        (arg, lambda: call("dpc_negq_push", pred, finfT, 20, ring, ringT, st, R, D, Kk)),
        (uns, lambda: call("dpc_negq_push", pred, finfT, ldT, ring, ringT, st, R, 64, Kk)),
        (arg, lambda: call("dpc_negq_clear", None, None)),
        (arg, lambda: call("dpc_negq_fwd", None, ring, st, R, D, Kk, tgt, R + 1, L.F32, stats, ws)),
        (arg, lambda: call("dpc_negq_fwd", pred, None, st, R, D, Kk, tgt, R + 1, L.F32, stats, ws)),
        (arg, lambda: call("dpc_negq_fwd", pred, ring, None, R, D, Kk, tgt, R + 1, L.F32, stats, ws)),
        (arg, lambda: call("dpc_negq_fwd", pred, ring, st, R, D, Kk, None, R + 1, L.F32, stats, ws)),
        (arg, lambda: call("dpc_negq_fwd", pred, ring, st, R, D, Kk, tgt, R + 1, L.F32, None, ws)),
        (arg, lambda: call("dpc_negq_fwd", pred, ring, st, R, D, Kk, tgt, R + 1, L.F32, stats, None)),
        (arg, lambda: call("dpc_negq_fwd", pred, ring, st, R, D, 0, tgt, R + 1, L.F32, stats, ws)),
        (arg, lambda: call("dpc_negq_fwd", pred, ring, st, R, D, Kk, tgt, R + 1, 7, stats, ws)),
        (uns, lambda: call("dpc_negq_fwd", pred, ring, st, R, 64, Kk, tgt, R + 1, L.F32, stats, ws)),
        (arg, lambda: call("dpc_negq_bwd", None, ring, ringT, st, R, D, Kk, lse, ws)),
        (arg, lambda: call("dpc_negq_bwd", pred, ring, None, st, R, D, Kk, lse, ws)),
        (arg, lambda: call("dpc_negq_bwd", pred, ring, ringT, st, R, D, Kk, None, ws)),
        (arg, lambda: call("dpc_negq_bwd", pred, ring, ringT, st, R, D, Kk, lse, None)),
        (arg, lambda: call("dpc_negq_bwd", pred, ring, ringT, st, R, D, 0, lse, ws)),
        (uns, lambda: call("dpc_negq_bwd", pred, ring, ringT, st, R, 64, Kk, lse, ws)),
        (arg, lambda: call("dpc_ce_topk_ext", tgt, R, R, R, stats, out, None, L.F32, R, None, lse)),
        (arg, lambda: call("dpc_ce_topk_ext", tgt, R, R, R, stats, out, None, L.F32, R, ws, None)),
        (arg, lambda: call("dpc_ce_topk_bf16_ext", ring, R, R, R, stats, out, None, R, None, lse)),
    ]
    for code, f in bad:
        with pytest.raises(L.DpcError, match=code):
            f()
    k.sync()
    assert torch.equal(bits(ring), bits(ring0)) and torch.equal(bits(ringT), bits(ring0)) and st.cpu().tolist() == [1, 1, 0, 0]
    assert bool(torch.isnan(stats).all()) and bool(torch.isnan(ws).all()) and bool(torch.isnan(out).all())
    nf, nb = C.c_int64(0), C.c_int64(0)
    for Rr, Dd, Kq, code in ((0, D, Kk, L.ERR_ARG), (R, D, 0, L.ERR_ARG), (R, 64, Kk, L.ERR_UNSUPPORTED)):
        assert k.lib._fn("dpc_negq_ws_floats")(Rr, Dd, Kq, C.byref(nf), C.byref(nb)) == code


# ================================================================================================================ engine
ARMS = {"f32 logits": dict(size=64, B=2), "bf16 logits": dict(size=128, B=4)}   # r18, num_seq 4, pred_step 1: R = 8 and R = 64


def arm_cfg(cfg: Cfg, arm: str) -> Cfg:
    return Cfg(device=cfg.device, simulator=cfg.simulator, widths=cfg.widths, **ARMS[arm])


def inputs(cfg: Cfg, count: int):
    shape = gc.dpc_input(cfg).shape
    return [torch.randn(shape, generator=torch.Generator().manual_seed(700 + j)).to(cfg.device) for j in range(count)]


def engine(cfg: Cfg, k_slots=0):
    eng = gc.dpc_engine(cfg, BF16)
    if k_slots:
        eng.set_neg_queue(k_slots)
    return eng


def all_arenas(eng):
    return [t.detach().clone() for t in (eng.flat_p, eng.flat_m, eng.flat_v, eng.dev_step, eng.dev_bc)]


def ring_state(eng):
    return [eng._negq_ring.detach().clone(), eng._negq_ringT.detach().clone(), eng._negq_state.detach().clone()]


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def case_empty_bank_is_no_bank(cfg: Cfg, arm: str):   # E1
    c = arm_cfg(cfg, arm)
    a, b = engine(c), engine(c, 2)
    assert b.neg_queue == 2 and b.neg_queue_filled() == 0 and ("negq", 2) in b._baked_scalars() and a.neg_queue == 0
    assert b._baked_scalars() == a._baked_scalars() + (("negq", 2),)
    assert (b.score16 is not None) == (arm == "bf16 logits")
    x = inputs(c, 1)[0]
    ra, rb = a.train_step(x).clone(), b.train_step(x).clone()
    assert torch.equal(bits(ra), bits(rb)) and torch.equal(bits(a.flat_g), bits(b.flat_g)) and same(all_arenas(a), all_arenas(b))
    assert b.neg_queue_filled() == 1


def hand_reference(pred, finf, s_in, bank_keys, bf16_logits):
    """f64 loss, ranks, d_pred, d_finf of one training step from the step's own pred / feat_inf (bf16 values), its in-batch logits as the
    loss kernel read them (s_in: rounded, held against pred @ finf^T here) and the keys the bank held, oldest slot first"""
    P, F = pred.double().numpy(), finf.double().numpy()
    R = P.shape[0]
    S = s_in.double().numpy()
    exact = P @ F.T
    tol = (np.abs(P) @ np.abs(F).T) * (2.0 ** -8 if bf16_logits else P.shape[1] * 2.0 ** -23) + 1e-30   # an f32-accumulated product, rounded once
    assert (np.abs(S - exact) <= tol).all(), "the in-batch logits are not pred @ finf^T"
    Q = np.concatenate([q.double().numpy() for q in bank_keys], 0) if bank_keys else np.zeros((0, P.shape[1]))
    allS = np.concatenate([S, P @ Q.T], 1)
    tgt = np.diagonal(S)
    mx = allS.max(1)
    e = np.exp(allS - mx[:, None])
    lse = np.log(e.sum(1)) + mx
    p = e / e.sum(1)[:, None]
    dS = p.copy()
    dS[np.arange(R), np.arange(R)] -= 1.0
    dS /= R
    keys = np.concatenate([F, Q], 0)
    N = keys.shape[0] + 64 + 32   # f32 roundings per output element: one per product at most, padding and slab sums included
    f = 2.0 ** -8 + N * 2.0 ** -24
    # What f32 itself adds on real logits (the kernel cases' logits are at most 1 in size; a network's reach tens, and a row's lightest
    # column then weighs nothing): a row's loss term is log(se) + mx - tgt in f32, four roundings at the size of the largest of them, and
    # the mean is ce_finalize_kernel's f32 sum, at most ceil(R / 256) + 10 roundings at the size of the partial sums.  The probability of
    # the target is an f32 (spacing 2^-24 below 1) before the one-hot is subtracted: two roundings there reach the diagonal term.
    term = lse - tgt
    big = np.maximum(np.maximum(np.abs(mx), np.abs(tgt)), np.maximum(np.abs(lse), np.abs(term)))
    # A queue logit is the f32 accumulator of the matrix cores, at most one rounding per product: it is off by at most D 2^-24 sum_d
    # |p_d q_cd|, and a row's log-sum-exp moves by no more than its worst logit does.
    acc = P.shape[1] * 2.0 ** -24 * (np.abs(P) @ np.abs(Q).T).max(1) if Q.shape[0] else np.zeros(R)
    rbound = QUARTER * -np.log1p(-p.min(1)) + 2.0 ** -24 * 4 * big + acc       # per row: the kernel cases' bound plus what f32 adds
    lbound = float(rbound.max()) + 2.0 ** -24 * (-(-R // 256) + 10) * float(np.abs(term).mean())
    diag = 2.0 ** -23 / R
    return dict(loss=float(term.mean()), lbound=lbound, term=term, rbound=rbound, rank=(allS > tgt[:, None]).sum(1),
                d_pred=dS @ keys, b_pred=f * (np.abs(dS) @ np.abs(keys)) + diag * np.abs(F),
                d_finf=dS[:, :R].T @ P, b_finf=f * (np.abs(dS[:, :R]).T @ np.abs(P)) + diag * np.abs(P))


def hand_step(eng, x, bank_keys, report, tag):
    """one training step taken apart: forward + loss, the clones, backward, the checks against hand_reference, the update"""
    R, D = eng.R, eng.D
    eng._forward_loss(x, True)
    pred, finf = eng.pred.detach().reshape(R, D).cpu().clone(), eng.feat_inf.detach().reshape(R, D).cpu().clone()
    s_in = (eng.score16 if eng._score16_live else eng.score).detach().cpu().clone()
    res = eng.result.detach().cpu().clone()
    rows = eng.row_ws.detach().cpu().double().numpy().reshape(R, 2).copy()
    eng.backward()
    d_pred, d_finf = eng.d_pred.detach().reshape(R, D).cpu().double().numpy(), eng.d_finf.detach().reshape(R, D).cpu().double().numpy()
    ref = hand_reference(pred, finf, s_in, bank_keys, eng._score16_live)
    er = np.abs(rows[:, 0] - ref["term"])   # every row's loss term and rank, then the mean
    assert (er < ref["rbound"]).all(), (tag, np.nonzero(~(er < ref["rbound"]))[0][:8].tolist(), float((er / ref["rbound"]).max()))
    assert np.array_equal(rows[:, 1], ref["rank"].astype(np.float64)), (tag, np.nonzero(rows[:, 1] != ref["rank"])[0][:8].tolist())
    assert abs(float(res[0]) - ref["loss"]) < ref["lbound"], (tag, float(res[0]), ref["loss"], ref["lbound"])
    for i, kk in enumerate((1, 3, 5)):
        assert float(res[1 + i]) == float(np.float32(int((ref["rank"] < kk).sum())) / np.float32(R)), (tag, kk)
    ep, ef = np.abs(d_pred - ref["d_pred"]), np.abs(d_finf - ref["d_finf"])
    assert (ep <= ref["b_pred"]).all() and (ef <= ref["b_finf"]).all(), (tag, float((ep / ref["b_pred"]).max()), float((ef / ref["b_finf"]).max()))
    report(f"[negq-engine] {tag}: {len(bank_keys)} slots live, loss {float(res[0]):.5f} (f64 {ref['loss']:.5f}, bound {ref['lbound']:.3g}), rows "
           f"{float((er / ref['rbound']).max()):.3g}, d_pred "
           f"{float((ep / ref['b_pred']).max()):.3g}, d_finf {float((ef / ref['b_finf']).max()):.3g} of their bounds")
    return finf, ref


def check_ring(eng, batches):
    """the ring holds batch j in slot j % K for the last K batches, rows and transposed"""
    Kk, R = eng.neg_queue, eng.R
    n = len(batches)
    st = eng._negq_state.cpu().tolist()
    assert st[:2] == [n, min(n, Kk)] and eng.neg_queue_filled() == min(n, Kk)
    for j in range(max(0, n - Kk), n):
        assert torch.equal(bits(eng._negq_ring[j % Kk, :R].cpu()), bits(batches[j])), f"slot {j % Kk} is not batch {j}"
        assert torch.equal(bits(eng._negq_ringT[j % Kk, :, :R].cpu()), bits(batches[j].t().contiguous()))


def live_keys(batches, Kk):
    """the keys a step reads, in slot order, after len(batches) pushes"""
    n = len(batches)
    slot = {j % Kk: batches[j] for j in range(max(0, n - Kk), n)}
    return [slot[s] for s in sorted(slot)]


def case_by_hand(cfg: Cfg, arm: str, report=print):   # E2
    c = arm_cfg(cfg, arm)
    eng = engine(c, 2)
    batches = []
    losses = []
    for j, x in enumerate(inputs(c, 4)):
        finf, ref = hand_step(eng, x, live_keys(batches, 2), report, f"{arm} step {j}")
        eng.adam_step()
        batches.append(finf)
        check_ring(eng, batches)   # the wrap: step 2 overwrites slot 0, step 3 slot 1
        losses.append(ref["loss"])
    assert eng.step_count == 4


def case_eval_between(cfg: Cfg, arm: str):   # E3
    c = arm_cfg(cfg, arm)
    eng, plain = engine(c, 2), engine(c)
    xs = inputs(c, 2)
    eng.train_step(xs[0])
    plain.flat_p.copy_(eng.flat_p)
    plain.packed_for_step = -1
    before = ring_state(eng)
    for e in (eng, plain):
        e.forward(xs[1], train=False, materialise=False)
        e.loss_topk(with_grad=False)
    assert torch.equal(bits(eng.result), bits(plain.result)) and same(ring_state(eng), before)
    s = eng.forward(xs[1], train=True)   # the module boundary's forward returns the score and leaves the bank alone as well
    assert s is not None and same(ring_state(eng), before) and not eng._negq_live


def case_nan_empties_the_bank(cfg: Cfg):   # E4
    c = arm_cfg(cfg, "f32 logits")
    eng, plain = engine(c, 2), engine(c)
    xs = inputs(c, 3)
    for e in (eng, plain):
        e.set_grad_guard(skip_nonfinite=True)
        e.train_step(xs[0])
    assert eng.neg_queue_filled() == 1 and same(all_arenas(eng), all_arenas(plain))
    before = all_arenas(eng)
    for e in (eng, plain):
        e._forward_loss(xs[1], True)
        e.backward()
        o, _ = e.offsets["backbone.layer2.0.conv1.weight"]
        e.flat_g[o + 5] = float("nan")
        e.adam_step()
    assert eng.neg_queue_filled() == 0 and eng._negq_state.cpu().tolist() == [0, 0, 0, 0] and eng.grad_stats()["skip"] == 1
    assert same(all_arenas(eng), before)
    ra, rb = eng.train_step(xs[2]).clone(), plain.train_step(xs[2]).clone()   # the next step equals a no-bank step
    assert torch.equal(bits(ra), bits(rb)) and torch.equal(bits(eng.flat_g), bits(plain.flat_g)) and same(all_arenas(eng), all_arenas(plain))
    assert eng.neg_queue_filled() == 1


def case_accumulation(cfg: Cfg, report=print):   # E5
    c = arm_cfg(cfg, "f32 logits")
    eng = engine(c, 2)
    eng.set_grad_accum(2)
    xs = inputs(c, 2)
    eng.train_step(xs[0])
    with pytest.raises(RuntimeError):
        eng.set_neg_queue(3)   # refused in the middle of a cycle
    first = eng.feat_inf.detach().reshape(eng.R, eng.D).cpu().clone()
    assert eng.accum_pending == 1 and eng.neg_queue_filled() == 1
    check_ring(eng, [first])
    # the second micro-batch of the cycle competes against the first one's keys, computed with the same weights
    finf, _ = hand_step(eng, xs[1], [first], report, "accumulation, micro-batch 1")
    eng._accum_launch(L.ACCUM_FINISH, 0, eng.numel)
    eng._accum_pos = 0
    eng.adam_step()
    check_ring(eng, [first, finf])
    assert int(eng.dev_step.item()) == 1


def case_checkpoint(cfg: Cfg, tmp_path):   # E6
    from dpc_amd import checkpoint as ckpt
    c = arm_cfg(cfg, "f32 logits")
    a, b, plain = engine(c, 2), engine(c, 2), engine(c)
    x = inputs(c, 1)[0]
    a.train_step(x)
    state = ckpt.build_state(a, 1, "resnet18", 0.0, 1)
    assert state["neg_queue"] == 2 and "neg_queue" not in ckpt.build_state(plain, 1, "resnet18", 0.0, 1)
    ring_bytes = a._negq_ring.numel() * 2

    def tensors(o):
        if isinstance(o, torch.Tensor):
            yield o
        elif isinstance(o, dict):
            for v in o.values():
                yield from tensors(v)
        elif isinstance(o, (list, tuple)):
            for v in o:
                yield from tensors(v)
    assert not any(t.data_ptr() == a._negq_ring.data_ptr() or (t.dtype == BF16 and t.numel() * 2 == ring_bytes) for t in tensors(state))
    path = str(tmp_path / "epoch1.pth.tar")
    ckpt.save_checkpoint(state, filename=path)
    b.train_step(x)
    assert b.neg_queue_filled() == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ckpt.resume(b, path)            # the same K: silent, and the bank starts empty
    assert b.neg_queue_filled() == 0 and b.neg_queue == 2
    b.set_neg_queue(3)
    assert ("negq", 3) in b._baked_scalars() and ("negq_ring", 2) in b._baked_scalars()   # a second allocation: older captures must not replay
    with pytest.warns(UserWarning, match="negative queue of 2 batches") as rec:
        ckpt.resume(b, path)
    assert sum("negative queue" in str(w.message) for w in rec) == 1
    with pytest.warns(UserWarning, match="negative queue of 2 batches"):
        ckpt.resume(plain, path)
    a.reset_neg_queue()
    assert a.neg_queue_filled() == 0
    a.train_step(x)
    a.load_params(a.state_dict())
    assert a.neg_queue_filled() == 0
    a.set_neg_queue(0)
    assert a.neg_queue == 0 and a._negq_ring is None and ("negq", 2) not in a._baked_scalars() and a.neg_queue_filled() == 0


def case_refusals(cfg: Cfg):   # E7
    from dpc_amd.engine import DPCEngine
    c = arm_cfg(cfg, "f32 logits")
    f32 = gc.dpc_engine(c, F32)
    with pytest.raises(L.DpcError, match="bf16"):
        f32.set_neg_queue(2)
    eng = engine(c)
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="1 .. 64"):
            eng.set_neg_queue(bad)
    fused = DPCEngine("resnet18", c.size, c.N, c.SL, c.P, c.B, c.device, BF16, c.widths, lib=c.simulator, score_path="fused")
    with pytest.raises(L.DpcError, match="fused"):
        fused.set_neg_queue(2)
    if c.simulator is not None:   # a feature size the kernels do not serve (the GPU tier runs the reference's widths: D = 256)
        odd = DPCEngine("resnet18", c.size, c.N, c.SL, c.P, c.B, c.device, BF16, (8, 16, 32, 64), lib=c.simulator)
        with pytest.raises(L.DpcError, match="256 or 32"):
            odd.set_neg_queue(2)
    eng.set_grad_accum(2)
    eng.train_step(inputs(c, 1)[0])
    with pytest.raises(RuntimeError, match="accumulation cycle is open"):
        eng.set_neg_queue(2)
    eng.reset_accum()
    eng.set_neg_queue(2)
    assert eng.neg_queue == 2
    if c.device != "cpu":
        t = torch.zeros(8, device=c.device)
        torch.cuda.synchronize()
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            t.add_(1.0)
            with pytest.raises(L.DpcError, match="captured"):
                eng.set_neg_queue(3)
        assert eng.neg_queue == 2


# ---------------------------------------------------------------------- two ranks over gloo (simulator)
def _gloo_rank(rank: int, world: int, port: int, out_dir: str, widths):
    import torch.distributed as dist
    from dpc_amd.parallel import make_allreduce
    torch.set_num_threads(2)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    cfg = arm_cfg(Cfg(device="cpu", simulator=L.load_emulator(), widths=widths), "f32 logits")
    eng = engine(cfg, 2)
    ex = make_allreduce(dist, world)
    gen = torch.Generator().manual_seed(900 + rank)   # every rank its own shard, so its own keys
    for _ in range(3):
        eng.train_step(torch.randn(gc.dpc_input(cfg).shape, generator=gen), allreduce=ex)
    torch.save({"p": eng.flat_p.clone(), "ring": eng._negq_ring.clone(), "state": eng._negq_state.clone()}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def case_two_ranks(widths, tmp_path):   # E8
    import torch.multiprocessing as mp
    mp.spawn(_gloo_rank, args=(2, 29900 + os.getpid() % 90, str(tmp_path), tuple(widths)), nprocs=2, join=True)
    a, b = (torch.load(os.path.join(str(tmp_path), f"rank{i}.pt")) for i in range(2))
    assert torch.equal(bits(a["p"]), bits(b["p"]))                              # the gradient is all that is exchanged
    assert a["state"].tolist() == b["state"].tolist() == [3, 2, 0, 0]
    assert not torch.equal(bits(a["ring"]), bits(b["ring"]))                     # each rank keeps its own bank


# ---------------------------------------------------------------------- the entry (simulator)
def case_entry(emu, widths, capsys):   # C1
    from dpc_amd import main as dpc_main
    common = ["--net", "resnet18", "--img_dim", "64", "--batch_size", "2", "--gpu", "0", "--print_freq", "1", "--num_seq", "4", "--epochs", "1",
              "--pred_step", "1", "--synthetic", "1"]
    run = lambda flags: (dpc_main.main(common + flags, _simulator=emu, _widths=widths), capsys.readouterr().out)[1]   # noqa: E731
    on = run(["--neg_queue", "3"])
    assert on.splitlines().count("Negative queue: 3 batches (24 keys of 32, per GPU)") == 1, on
    off, zero = run([]), run(["--neg_queue", "0"])
    strip = lambda s: re.sub(r"T:\d+\.\d+", "T:", s)   # noqa: E731
    assert "Negative queue" not in off and strip(off) == strip(zero)
    for flags in (["--neg_queue", "-1"], ["--neg_queue", "65"], ["--neg_queue", "2", "--dtype", "f32"]):
        with pytest.raises(ValueError, match="--neg_queue"):   # before a rank starts: nothing is printed
            dpc_main.main(common + flags, _simulator=emu, _widths=widths)
        assert capsys.readouterr().out == ""


# ---------------------------------------------------------------------- captured steps (HIP device only)
EXTRA_LAUNCHES = 4   # per training step with the bank on: dpc_negq_fwd, dpc_negq_bwd, its dpc_reduce_unpack, dpc_negq_push


def case_captured(cfg: Cfg, arm: str, accum: int = 1):   # E9
    """a captured step with K = 2 replayed five times across the fill boundary (one slot is live at the capture, the second replay
    wraps) against an eager twin, bit for bit; the capture holds the no-bank capture's launches plus EXTRA_LAUNCHES per step"""
    c = arm_cfg(cfg, arm)
    xs = inputs(c, 6 * accum)
    a, b, plain = engine(c, 2), engine(c, 2), engine(c)
    for e in (a, b, plain):
        if accum > 1:
            e.set_grad_accum(accum)
        for x in xs[:accum]:   # an eager step (cycle) sizes every lazy buffer
            e.train_step(x)
    block = xs[0].clone()
    ref = plain.capture_train_step(block, warmup=0)
    replay = a.capture_train_step(block, warmup=0)
    if accum > 1:
        assert replay.micro.kernels == [ref.micro.kernels[0] + EXTRA_LAUNCHES] and replay.last.kernels == [ref.last.kernels[0] + EXTRA_LAUNCHES]
    else:
        assert replay.kernels == [ref.kernels[0] + EXTRA_LAUNCHES]
    assert a.neg_queue_filled() == min(accum, 2)
    for j, x in enumerate(xs[accum:6 * accum]):
        block.copy_(x)
        ra = replay().clone()
        rb = b.train_step(x).clone()
        assert torch.equal(bits(ra), bits(rb)), j
        assert torch.equal(bits(a.flat_p), bits(b.flat_p)) and same(ring_state(a), ring_state(b)), j
    assert a._negq_state.cpu().tolist()[:2] == [6 * accum, 2] and a.step_count == b.step_count == 6
    a.set_neg_queue(3)
    with pytest.raises(RuntimeError):
        replay()
    a.release_captures()
    plain.release_captures()
