"""GPU tier: the head's backward (DPCEngine._head_backward: the score backward in its three forms, dpc_gru_chain_bwd,
dpc_tpool_split_bwd and the side-stream ConvGRU / network_pred parameter gradients) against an oracle that rounds where the engine
rounds (oracle.head_rounded + score_ce_backward_chunked), held to the 2 % of the block and stem tests in bf16 and 1e-4 in f32.

(a) the block tests' engines (r18 / 128^2 / B = 16, r34 / 224^2 / B = 4): f32 logits, bf16 logits, the fused score, the score backward
    on the loader / compute split-K GEMM (DPC_GEMM_WS_MIN lowered before the engine is built), and the f32 mode.  Four mutations
    computed from the engine's own results must miss the oracle by more than 5 x the tolerance.
(b) the benchmarked batches (cfg2, cfg4, cfg5) in the forms the train step runs: d_feat per 8 clips, H_all and d_featrelu per step and
    per 1024 rows with the last 32 rows of M on their own, d_pred / d_finf per 1024 rows and the last rows on their own -- a wrong
    last workgroup cannot hide in a global norm.
(c) cfg2: the head parameter gradients of a whole backward() (side stream, beside layer4, sharing the split-K slabs with the backbone's
    weight gradients) are bit-identical to those of _head_backward() alone.

Every step runs train-mode: the recurrence regenerates its Philox dropout masks, the oracle reads them from dropout_masks_of_step().
The forward tensors are held to the free-running oracle; the backward to the oracle pinned to the engine's stored forward values
(tests/head_cases.py: with the oracle's own forward, bf16 rounding flips alone put d_feat at 2 %, with the stored values at 0.25 %)."""
import time

import pytest
import torch

from head_cases import HEAD, NAN, case, engine, step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# ---------------------------------------------------------------------------------------------------- (a) small batch
SMALL = {"r18": ("resnet18", 128, 16), "r34": ("resnet34", 224, 4)}


# (r34 / 224^2 / B = 4 has R = 588, not a multiple of 64: no bf16 logits there, its train step runs f32 logits)
@pytest.mark.parametrize("net,form", [(n, f) for n in ("r18", "r34") for f in ("f32 logits", "bf16 logits", "fused", "gemm_ws", "f32")
                                      if not (n == "r34" and f == "bf16 logits")])
def test_head_backward_small_batch(net, form, monkeypatch):
    name, size, B = SMALL[net]
    if form == "gemm_ws":   # the benchmark's score-backward kernels at small R: decided when the head is built (_tn_splits)
        monkeypatch.setenv("DPC_GEMM_WS_MIN", "64")
    dtype = torch.float32 if form == "f32" else torch.bfloat16
    e = engine(name, size, 3, B, dtype, "fused" if form == "fused" else "auto")
    assert (e._tn_splits is not None) == (form == "gemm_ws"), e._tn_splits
    materialise = form in ("f32 logits", "f32")
    case(e, f"{name}/{size}/B={B} {form}", materialise, mutate=form in ("f32 logits", "f32"))
    want = {"f32 logits": "materialised", "f32": "materialised", "fused": "fused", "bf16 logits": "materialised (bf16 logits)",
            "gemm_ws": "materialised (bf16 logits)" if e.score16 is not None else "materialised"}[form]
    assert e.score_mode == want, e.score_mode
    del e
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- (b) benchmarked batch
@pytest.mark.parametrize("cfg,form", [("cfg2", "train"), ("cfg2", "fused"), ("cfg2", "f32"), ("cfg4", "train"), ("cfg5", "train"),
                                      ("cfg5", "fused")])
def test_head_backward_full_batch(cfg, form):
    net, size, B, P = {"cfg2": ("resnet18", 128, 128, 3), "cfg4": ("resnet34", 224, 44, 3), "cfg5": ("resnet34", 224, 64, 5)}[cfg]
    dtype = torch.float32 if form == "f32" else torch.bfloat16
    e = engine(net, size, P, B, dtype, "fused" if form == "fused" else "auto")
    if dtype == torch.bfloat16:
        assert e._tn_splits is not None   # d_feature_inf on the loader / compute split-K GEMM, as the benchmark runs it
    if cfg == "cfg4":
        assert e.M % 32 and e.ld_d != e.R and e.score16 is None   # partial last recurrence tile, padded dscore rows, f32 logits
    case(e, f"{cfg} {form}", materialise=(form == "f32"))
    del e
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- (c) side stream
def test_head_grads_of_the_whole_backward_are_the_head_backwards_cfg2():
    e = engine("resnet18", 128, 3, 128, torch.bfloat16)
    assert e._side is not None
    step(e, materialise=False)
    alone = {k: e.G[k].detach().clone() for k in HEAD}
    for k in HEAD:
        e.G[k].fill_(NAN)
    e.backward()
    torch.cuda.synchronize()
    for k in HEAD:
        assert torch.equal(e.G[k], alone[k]), k
    print("\n[head] cfg2: the ten head parameter gradients of backward() are bit-identical to _head_backward()'s")
    del e
    torch.cuda.empty_cache()
