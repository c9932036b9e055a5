"""CPU tier: the head oracle (oracle.head_rounded + score_ce_backward_chunked) that tests/test_head_grads_gpu.py holds the engine's
head backward to.  With the rounding off it must BE the reference's head: f64 autograd of the lines of DPC_RNN.forward after the
backbone (oracle.dpc_head, restating dpc/model_3d.py:53-84) plus CrossEntropyLoss / top-k (loss_and_topk), within 1e-10 --
P = 1, 3, 5, SQ = 4 and 49, a row chunk that does not divide R.  The closed-form score backward keeps the engine's tie rule (a
logit equal to the target's ranks behind it), and each rounding helper rounds in one direction only."""
import pytest
import torch

from oracle import dpc_oracle as O

f64 = torch.float64


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


def _head_params(D, seed):
    g = torch.Generator().manual_seed(seed)
    p = {}
    for k in O.HEAD_PARAMS:
        if k.endswith("bias"):
            p[k] = 0.1 * torch.randn(D, generator=g, dtype=f64)
        elif k.startswith("agg."):
            p[k] = torch.randn(D, 2 * D, 1, 1, generator=g, dtype=f64) / (2 * D) ** 0.5
        else:
            p[k] = torch.randn(D, D, 1, 1, generator=g, dtype=f64) / D ** 0.5
    return p


def _case(B, N, P, T, ls, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(B * N, T, ls, ls, D, generator=g, dtype=f64)
    masks = ((torch.rand(N - 1, B * ls * ls, D, generator=g) > 0.1).to(f64) / 0.9)
    return feat, masks, _head_params(D, seed + 1)


@pytest.mark.parametrize("P,ls,chunk", [(1, 2, 5), (3, 2, 7), (3, 7, 37), (5, 7, 100)])
def test_unrounded_oracle_is_the_reference_head(P, ls, chunk):
    B, N, T, D = 2, 8, 2, 16
    feat, masks, p = _case(B, N, P, T, ls, D, seed=P + ls)
    SQ, M = ls * ls, B * ls * ls
    # ---- the reference: conv2d / NCTHW formulation of dpc_head, autograd of the mean CE
    lr = {k: v.clone().requires_grad_() for k, v in p.items()}
    fr = feat.permute(0, 4, 1, 2, 3).clone().requires_grad_()
    mref = [masks[i].view(B, ls, ls, D).permute(0, 3, 1, 2) for i in range(N - 1)] + [torch.ones(B, D, ls, ls, dtype=f64)]
    score, inter = O.dpc_head(lr, fr, B, P, mref, return_intermediates=True)
    inter["pred"].retain_grad()
    inter["feature_inf"].retain_grad()
    loss, accs = O.loss_and_topk(score)
    loss.backward()
    # ---- the oracle: row formulation, closed-form chunked score backward
    lo = {k: v.clone().requires_grad_() for k, v in p.items()}
    fo = feat.clone().requires_grad_()
    h = O.head_rounded(fo, lo, masks, P, rounded=False)
    h["feat_relu"].retain_grad()
    sc = O.score_ce_backward_chunked(h["pred"].detach(), h["feat_inf"].detach(), round_ds=False, chunk=chunk)
    torch.autograd.backward([h["pred"], h["feat_inf"]], [sc["d_pred"], sc["d_finf"]])
    R = B * P * SQ
    assert h["pred"].shape == (R, D) and h["feat_inf"].shape == (R, D)
    assert h["H_all"].shape == (N, M, D) and h["X_all"].shape == (N - 1, M, D) and h["P1_all"].shape == (P, M, D)
    assert rel(h["pred"].detach(), inter["pred"].detach()) < 1e-12
    assert rel(h["feat_inf"].detach(), inter["feature_inf"].detach()) < 1e-12
    assert abs(sc["loss"].item() - loss.item()) < 1e-10 * abs(loss.item())
    assert sc["accs"] == pytest.approx([a.item() for a in accs], abs=1e-6)   # (the reference sums f32 hits; 1/R >= 2e-3)
    Sd = score.detach().reshape(R, R)
    assert torch.equal(sc["rank"], (Sd > Sd.diagonal()[:, None]).sum(1))
    assert rel(sc["d_pred"], inter["pred"].grad) < 1e-10
    assert rel(sc["d_finf"], inter["feature_inf"].grad) < 1e-10
    assert rel(fo.grad, fr.grad.permute(0, 2, 3, 4, 1)) < 1e-10
    for k in O.HEAD_PARAMS:
        assert rel(lo[k].grad, lr[k].grad) < 1e-10, k
    # d_featrelu: the aggregation inputs' gradient; the ReLU'd features of the last P blocks are not used
    assert h["feat_relu"].grad[N - P:].abs().max().item() == 0
    assert h["feat_relu"].grad[:N - P].abs().max().item() > 0


@pytest.mark.parametrize("logits", ["f32", "bf16"])
def test_score_backward_ties_rank_behind_and_chunks_agree(logits):
    R, D = 53, 8
    g = torch.Generator().manual_seed(3)
    pred = torch.randn(R, D, generator=g).to(torch.bfloat16).double()
    finf = torch.randn(R, D, generator=g).to(torch.bfloat16).double()
    finf[7] = finf[4]                     # row 4: column 7 ties the target exactly
    finf[11] = finf[12]                   # row 12: column 11 ties the target exactly ...
    finf[13] = 2 * finf[12]               # ... and column 13 beats it whenever the target logit is positive
    pred[12] = finf[12]                   # (it is: |finf[12]|^2 > 0)
    S = pred @ finf.t()
    assert S[4, 7] == S[4, 4] and S[12, 11] == S[12, 12] and S[12, 13] > S[12, 12]
    whole = O.score_ce_backward_chunked(pred, finf, logits=logits, round_ds=False, chunk=R)
    parts = O.score_ce_backward_chunked(pred, finf, logits=logits, round_ds=False, chunk=10)
    for k in ("d_pred", "d_finf"):
        assert rel(parts[k], whole[k]) < 1e-14
    assert torch.equal(parts["rank"], whole["rank"])
    Sl = O._to_bf16(S) if logits == "bf16" else S
    assert torch.equal(whole["rank"], (Sl > Sl.diagonal()[:, None]).sum(1))
    assert int(whole["rank"][12]) == int((Sl[12] > Sl[12, 12]).sum()) >= 1
    assert int((Sl[4] == Sl[4, 4]).sum()) >= 2 and int(whole["rank"][4]) == int((Sl[4] > Sl[4, 4]).sum())
    # loss and gradient against autograd of CrossEntropyLoss on the same logits
    sd = Sl.clone().requires_grad_()
    ce = torch.nn.functional.cross_entropy(sd, torch.arange(R))
    ce.backward()
    assert abs(whole["loss"].item() - ce.item()) < 1e-12 * ce.item()
    assert rel(whole["d_pred"], sd.grad @ finf) < 1e-12 and rel(whole["d_finf"], sd.grad.t() @ pred) < 1e-12
    # round_ds: dS passes through bf16 once, before both products
    rd = O.score_ce_backward_chunked(pred, finf, logits=logits, round_ds=True, chunk=10)
    dsq = O._to_bf16(sd.grad)
    assert rel(rd["d_pred"], dsq @ finf) < 1e-12 and rel(rd["d_finf"], dsq.t() @ pred) < 1e-12


def test_rounding_helpers_round_in_one_direction_each():
    x = torch.tensor([1.0 + 2.0 ** -10, -3.0 - 2.0 ** -9, 0.1], dtype=f64, requires_grad=True)
    gout = torch.tensor([1.0 + 2.0 ** -11, 2.0 ** -20 * (1 + 2.0 ** -12), -7.0 - 2.0 ** -8], dtype=f64)
    bf = O._to_bf16
    y = O.ste_round_bf16(x)
    assert torch.equal(y.detach(), bf(x.detach())) and not torch.equal(y.detach(), x.detach())
    y.backward(gout)
    assert torch.equal(x.grad, gout)                  # the value is rounded, its gradient is not
    x.grad = None
    y = O.ste_round_grad_bf16(x)
    assert torch.equal(y.detach(), x.detach())
    y.backward(gout)
    assert torch.equal(x.grad, bf(gout)) and not torch.equal(x.grad, gout)   # the gradient is rounded, the value is not


def test_rounded_head_stores_bf16_values():
    B, N, P, T, ls, D = 2, 8, 3, 2, 2, 16
    feat, masks, p = _case(B, N, P, T, ls, D, seed=9)
    h = O.head_rounded(O._to_bf16(feat), p, masks, P, rounded=True)
    for k in ("pred", "feat_inf", "feat_relu", "X_all", "H_all", "HR_all", "P1_all"):
        v = h[k].detach()
        assert torch.equal(v, O._to_bf16(v)), k
    u = O.head_rounded(O._to_bf16(feat), p, masks, P, rounded=False)
    e = rel(h["pred"].detach(), u["pred"].detach())
    assert 1e-4 < e < 3e-2, e                         # the rounding is there, and it is rounding-sized
