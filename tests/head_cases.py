"""the head-backward check shared by tests/test_head_grads_gpu.py (the MI355X at the block tests' and the benchmarked batches) and
tests/test_engine_emu.py (the SIMT simulator at a width-reduced net): one train-mode step of a DPCEngine, its head backward alone
(DPCEngine._head_backward), and every tensor of the head against oracle.head_rounded + score_ce_backward_chunked, chunk by chunk."""
import time

import torch

from dpc_amd.engine import DPCEngine
from oracle import dpc_oracle as O

TOL = 0.02          # bf16 (tests/test_block_grads_gpu.py, tests/test_stem_grads_gpu.py)
TOL32 = 1e-4        # f32
FTOL, FTOL32 = 5e-3, 2e-5   # forward tensors
HEAD = O.HEAD_PARAMS
NAN = float("nan")


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def engine(net, size, P, B, dtype, score_path="auto", device="cuda:0", widths=None, lib=None):
    kw = dict(widths=widths) if widths is not None else {}
    e = DPCEngine(net, size, 8, 5, P, B, device, dtype, score_path=score_path, lib=lib, **kw)
    p = O.init_params_reference_style(net, seed=0, **kw)
    g = torch.Generator().manual_seed(17)
    for k in HEAD:   # biases away from 0: a bias that is dropped or mis-sliced shows
        if k.endswith("bias"):
            p[k] = 0.1 * torch.randn(p[k].shape, generator=g)
    e.load_params(p)
    return e


def sync(e):
    if e.device.type == "cuda":
        torch.cuda.synchronize()


def step(e, materialise, seed=3):
    """a train-mode forward + loss on a fresh input, then the head backward alone; returns the dropout masks of the step"""
    x = torch.randn((e.B, 8, 3, 5, e.size, e.size), generator=torch.Generator().manual_seed(seed)).to(e.device)
    e.forward(x, train=True, materialise=materialise)
    del x
    e.loss_topk(True)
    masks = e.dropout_masks_of_step()
    for k in HEAD:
        e.G[k].fill_(NAN)   # a gradient that is never written fails
    for t in (e.d_feat, e.d_featrelu, e.d_pred, e.d_finf):
        t.fill_(NAN)
    d = e._head_backward()
    sync(e)
    assert d is e.d_feat
    return masks


def oracle(e, masks):
    """the oracle twice: free-running (its own forward: what the forward tensors are held to) and pinned to the engine's stored forward
    values (oracle.head_rounded(pin=...): the backward differentiated at the engine's own operands, as its kernels do -- a bf16
    rounding flip in the forward, another accumulation order, then does not feed the backward or move a near-tie rank)"""
    bf = e.cdtype == torch.bfloat16
    R, D = e.R, e.D
    feat = e.blocks[-1].out.detach().cpu().double()
    m64 = masks.cpu().double()
    lv = {k: e.PRM[k].detach().cpu().double() for k in HEAD}
    with torch.no_grad():
        free = O.head_rounded(feat, lv, m64, e.P, rounded=bf, num_seq=e.N)
    pin = {"X_all": e.X_all.cpu(), "H_all": e.H_all.cpu(), "HR_all": e.HR_all.cpu(), "P1_all": e.P1_all.cpu(),
           "pred": e.pred.view(R, D).cpu(), "feat_inf": e.feat_inf.view(R, D).cpu()}
    feat.requires_grad_()
    for v in lv.values():
        v.requires_grad_()
    h = O.head_rounded(feat, lv, m64, e.P, rounded=bf, num_seq=e.N, pin=pin)
    h["feat_relu"].retain_grad()
    logits = "bf16" if e._score16_live else "f32"
    sc = O.score_ce_backward_chunked(h["pred"].detach(), h["feat_inf"].detach(), logits=logits, round_ds=bf, chunk=1024)
    torch.autograd.backward([h["pred"], h["feat_inf"]], [sc["d_pred"], sc["d_finf"]])
    return free, h, sc, feat.grad, {k: v.grad for k, v in lv.items()}


def wg_mutations(e, h, sc, og, tol):
    """mutations of the engine's own results; each must miss the oracle by > 5 x tol on the check that holds it"""
    R, D, P, M = e.R, e.D, e.P, e.M
    out = {}
    if e._score16_live or e._score_fused:
        raise AssertionError("the mutations read the materialised f32-logit form's dscore")
    dS = e.dscore[:, :R].double().cpu()
    pred_e = e.pred.view(R, D).double().cpu()
    out["d_finf = dS @ pred"] = rel(dS @ pred_e, sc["d_finf"])
    gu, gr = e.G[HEAD[2]].detach().cpu().clone(), e.G[HEAD[0]].detach().cpu().clone()   # update, reset gate weights
    gu[:, D:], gr[:, D:] = e.G[HEAD[0]].detach().cpu()[:, D:], e.G[HEAD[2]].detach().cpu()[:, D:]
    out["dWh update <-> reset"] = max(rel(gu, og[HEAD[2]]), rel(gr, og[HEAD[0]]))
    dP1 = e.dP1.double().cpu().view(P, M, D)[:P - 1].reshape(-1, D)
    Hp = e.Hpred.double().cpu().view(P, M, D)[:P - 1].reshape(-1, D)
    out["network_pred.0 without the last step"] = rel((dP1.t() @ Hp).view(D, D, 1, 1), og["network_pred.0.weight"])
    return out


def _d_feat_of(e, d_featrelu, d_finf):
    """dpc_tpool_split_bwd restated: d_feat from (a possibly mutated) d_featrelu and d_finf"""
    B, N, P, SQ, D = e.B, e.N, e.P, e.SQ, e.D
    T = e.feat_shape[1]
    x = e.blocks[-1].out.float().cpu().view(B, N, T, SQ, D)
    m = x.mean(2)
    g = torch.zeros(B, N, SQ, D, dtype=torch.float64)
    na = N - P
    g[:, :na] = (d_featrelu.double().view(na, B, SQ, D).permute(1, 0, 2, 3) * (m[:, :na] > 0)) / T
    g[:, na:] = d_finf.double().view(B, P, SQ, D) / T
    return g.view(B * N, 1, SQ, D).expand(B * N, T, SQ, D).reshape(tuple(e.d_feat.shape))


def check(e, tag, t0, free, h, sc, d_feat_o, og, mutations=None):
    """every tensor of the head against the oracle, chunk by chunk; returns the errors"""
    bf = e.cdtype == torch.bfloat16
    tol, ftol = (TOL, FTOL) if bf else (TOL32, FTOL32)
    R, D, M, P, ns, na = e.R, e.D, e.M, e.P, e.n_steps, e.n_agg
    worst = {}

    def hold(name, where, got, ref):
        err = rel(got, ref)
        if err > worst.get(name, (-1.0, None))[0]:
            worst[name] = (err, where)

    def by_rows(name, got, ref, rows=1024, tail=32):   # [n, ...] chunks of `rows` along dim 0, the last `tail` rows on their own
        n = got.shape[0]
        tail = min(tail, n)
        for i0 in range(0, n, rows):
            hold(name, f"[{i0}:{min(i0 + rows, n)}]", got[i0:i0 + rows], ref[i0:i0 + rows])
        hold(name, f"[{n - tail}:{n}]", got[n - tail:], ref[n - tail:])

    def by_steps(name, got, ref, s0=0):   # [steps, M, D]: per step, per 1024 rows, the last 32 rows of M
        for s in range(s0, got.shape[0]):
            for i0, i1 in [(i, min(i + 1024, M)) for i in range(0, M, 1024)] + [(max(M - 32, 0), M)]:
                hold(name, f"step {s} [{i0}:{i1}]", got[s, i0:i1], ref[s, i0:i1])

    # forward
    by_steps("X_all", e.X_all.cpu(), free["X_all"])
    by_steps("H_all", e.H_all.cpu(), free["H_all"], s0=1)
    by_rows("feat_inf", e.feat_inf.view(R, D).cpu(), free["feat_inf"])
    by_rows("pred", e.pred.view(R, D).cpu(), free["pred"])
    fwd = [k for k in worst]
    if e._score16_live:
        if R <= 8192:
            S = O._to_bf16(free["pred"] @ free["feat_inf"].t())
            hold("score16", "", e.score16.cpu(), S)
            fwd.append("score16")
    elif not e._score_fused and R <= 8192:
        hold("score", "", e.score.cpu(), free["pred"] @ free["feat_inf"].t())
        fwd.append("score")
    # loss and top-k: per-row loss terms and ranks (row_ws), the reduced result
    rw = e.row_ws.cpu().double()
    errs = {"loss terms": rel(rw[:, 0], sc["terms"])}
    res = e.result.cpu().double()
    errs["loss"] = abs(res[0].item() - sc["loss"].item()) / abs(sc["loss"].item())
    dr = (rw[:, 1] - sc["rank"].double()).abs()
    # bf16 logits: a target logit within f32 accumulation noise of a bf16 rounding boundary may be stored one bf16 step up or down by
    # the engine and the oracle (which rounds the f64 value); the rank then moves by the number of logits in that step.  Such rows are
    # told apart from the others by the target's own value; every other row may differ by one (a near tie), as in case_score_fused.
    boundary = torch.zeros(R, dtype=torch.bool)
    if e._score16_live:
        st = (e.pred.view(R, D).double().cpu() * e.feat_inf.view(R, D).double().cpu()).sum(1)
        boundary = O._to_bf16(st * (1 + 2.0 ** -17)) != O._to_bf16(st * (1 - 2.0 ** -17))
    n_boundary = int((boundary & (dr > 1)).sum())
    rank_max, rank_frac = dr[~boundary].max().item(), (dr > 0).double().mean().item()
    ranks_e = rw[:, 1]
    acc_e = [(ranks_e < kk).double().mean().item() for kk in (1, 3, 5)]
    # backward
    by_rows("d_pred", e.d_pred.view(R, D).cpu(), sc["d_pred"])
    by_rows("d_finf", e.d_finf.view(R, D).cpu(), sc["d_finf"])
    dfr_o = h["feat_relu"].grad[:na]
    by_steps("d_featrelu", e.d_featrelu.cpu(), dfr_o)
    dfe = e.d_feat.cpu()
    # d_feat per 8 clips (one batch item), its aggregation clips (from d_featrelu) and its inference clips (from d_finf) apart
    by_rows("d_feat", dfe, d_feat_o, rows=8, tail=8)
    clips = lambda t, lo, hi: t.reshape(e.B, e.N, -1)[:, lo:hi]
    by_rows("d_feat[agg clips]", clips(dfe, 0, na), clips(d_feat_o, 0, na), rows=1, tail=1)
    by_rows("d_feat[inf clips]", clips(dfe, na, e.N), clips(d_feat_o, na, e.N), rows=1, tail=1)
    for k in HEAD:
        errs[k] = rel(e.G[k], og[k])
    errs.update({k: v[0] for k, v in worst.items()})
    # mutation 4: the last recurrence workgroup's rows of d_featrelu zeroed, seen by the per-8-clip d_feat check
    teeth = dict(mutations or {})
    dfr_m = e.d_featrelu.cpu().clone()
    m0 = (M - 1) // 32 * 32
    dfr_m[:, m0:] = 0
    dfm = _d_feat_of(e, dfr_m, e.d_finf.cpu())
    teeth[f"d_featrelu rows [{m0}:{M}] zeroed"] = max(rel(clips(dfm, 0, na)[b], clips(d_feat_o, 0, na)[b]) for b in range(e.B))
    assert rel(_d_feat_of(e, e.d_featrelu.cpu(), e.d_finf.cpu()), dfe) < (5e-3 if bf else 1e-6)   # the restatement is the kernel's
    print(f"\n[head] {tag} ({e.score_mode}, tn_splits={e._tn_splits}): loss {res[0].item():.5f} (oracle {sc['loss'].item():.5f}), "
          f"top-1/3/5 {acc_e[0]:.4f}/{acc_e[1]:.4f}/{acc_e[2]:.4f} (oracle {sc['accs'][0]:.4f}/{sc['accs'][1]:.4f}/{sc['accs'][2]:.4f}), "
          f"ranks off by <= {rank_max:.0f} on {rank_frac:.4%} of rows (+ {n_boundary} rows whose bf16 target logit lies on a rounding "
          f"boundary, off by {dr[boundary].max().item() if n_boundary else 0:.0f})")
    print("  " + ", ".join(f"{k.replace('agg.ConvGRUCell_00.', '')} {v:.2e}" for k, v in errs.items()))
    print("  worst chunk: " + ", ".join(f"{k} {v[0]:.2e} @ {v[1]}" for k, v in worst.items()))
    print("  mutations: " + ", ".join(f"{k} {v:.3f} ({v / tol:.0f} x tol)" for k, v in teeth.items()) + f"; {time.time() - t0:.1f} s")
    for k in fwd:
        assert errs[k] < ftol, (k, worst[k])
    assert errs["loss terms"] < ftol and errs["loss"] < (1e-3 if bf else 1e-5), errs
    assert rank_max <= 1 and rank_frac < 5e-3 and n_boundary <= max(1, R // 1000), (rank_max, rank_frac, n_boundary)
    assert max(abs(a - b) for a, b in zip(acc_e, res[1:].tolist())) < 1e-6   # the result is the reduction of these ranks
    for k in ("d_pred", "d_finf", "d_featrelu", "d_feat", "d_feat[agg clips]", "d_feat[inf clips]") + HEAD:
        assert errs[k] < tol, (k, errs[k], worst.get(k))
    for k, v in teeth.items():
        assert v > 5 * tol, (k, v)
    return errs


def case(e, tag, materialise, mutate=False):
    t0 = time.time()
    masks = step(e, materialise)
    free, h, sc, d_feat_o, og = oracle(e, masks)
    muts = wg_mutations(e, h, sc, og, TOL if e.cdtype == torch.bfloat16 else TOL32) if mutate else None
    return check(e, tag, t0, free, h, sc, d_feat_o.view(tuple(e.d_feat.shape)), og, muts)
