"""GPU tier: the grouped Adam kernel, torch autograd through dpc_amd.lc.LC, and the reference's training lines (eval/test.py:229-255)
under parameter groups and with a frozen extractor, on the MI355X: resnet18 at the reference's widths, 64 px, B = 2,
num_class = 101, f32 unless said otherwise.  The cases are those of the CPU tier (tests/adam_groups_cases.py,
tests/lc_upstream_cases.py, tests/lc_loop_cases.py)."""
import pytest
import torch
import torch.nn.functional as F

import adam_groups_cases as ac
import kcases as kc
import lc_loop_cases as lc
import lc_upstream_cases as uc
from dpc_amd import _lib as L
from dpc_amd.optim import Adam
from dpc_amd.plan import LAYER_WIDTH
from oracle import dpc_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def cfg():
    return lc.Cfg(device=DEV, simulator=None, widths=LAYER_WIDTH, num_class=101)


def test_adam_groups_kernel():
    k = kc.K(L.load_hip(), DEV)
    ac.case_adam_groups(k)
    ac.case_table_capacity()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lc_head_bwd_from_upstream_gradient(dtype):
    k = kc.K(L.load_hip(), DEV)
    uc.case_lc_head_upstream(k, dtype, 16, 16, 256, 101)
    uc.case_lc_head_upstream(k, dtype, 6, 3, 40, 11)


# The largest per-parameter difference, relative to that parameter gradient's max, between the engine's own backward (the CE kernel's
# d loss / d logits) and loss.backward() through the module (torch's softmax).  Measured on the MI355X: 2.959e-6 (backbone.bn1.bias).
# The bound is 10 x that, never looser than 2e-3.
AUTOGRAD_VS_ENGINE_MEASURED = 2.959e-6
AUTOGRAD_VS_ENGINE_BOUND = min(10 * AUTOGRAD_VS_ENGINE_MEASURED, 2e-3)


def test_autograd_against_the_engine(cfg):
    """same engine, same input, same forced masks: forward(train=True) + eng.backward(), then the module path with F.cross_entropy +
    loss.backward().  The forward is deterministic, so the two differ only by torch's softmax against the CE kernel's."""
    forced, _ = lc.masks(cfg)
    m = lc.module(cfg)
    m._forced_masks = forced
    x = O.make_input_pcg(cfg.B, cfg.N, cfg.SL, cfg.size).to(DEV)
    target = torch.tensor([3, 77], device=DEV)
    m(x)   # builds the engine
    eng = m.engine
    out_e, _ = eng.forward(x, target, train=True, gru_masks=forced[0], fc_mask=forced[1])
    out_e = out_e.clone()
    eng.backward()
    want = eng.flat_g.clone()
    out, _ = m(x, target)
    assert torch.equal(out, out_e)
    loss = F.cross_entropy(out.view(cfg.B, -1), target)
    m.zero_grad()
    loss.backward()
    assert abs(loss.item() - eng.result[0].item()) < 1e-5
    worst = ("", 0.0)
    for k, (o, n) in eng.offsets.items():
        e = (eng.flat_g[o:o + n] - want[o:o + n]).abs().max().item() / max(want[o:o + n].abs().max().item(), 1e-12)
        worst = max(worst, (k, e), key=lambda t: t[1])
    print(f"AUTOGRAD_VS_ENGINE worst {worst[1]:.3e} ({worst[0]})")
    assert worst[1] <= AUTOGRAD_VS_ENGINE_BOUND, worst


def test_reference_loop_with_one_group_per_parameter(cfg):
    lc.case_reference_loop_grouped(cfg)


def test_reference_loop_with_a_frozen_extractor(cfg):
    lc.case_frozen(cfg, "filter_requires_grad")


def test_autograd_decides_the_truncation(cfg):
    lc.case_autograd_decides_the_truncation(cfg)


def test_bf16_head_mode_lowers_the_loss():
    """bf16, B = 4, 128 px, linear probe (`head`): six steps of the reference's loop on one fixed batch (in-kernel Philox dropouts, as
    tests/test_lc_gpu.py::test_lc_bf16_training_and_module) lower the loss; the extractor's slices keep their bits.

    The loss is read before the first and after the sixth step from a train-mode forward with both dropouts switched off (keep
    masks of ones), i.e. from one fixed function of the parameters.  The loop's own loss values are no measure of progress here:
    every step draws new masks, and with Dropout(0.5) on 256 features, four clips and only the head learning, the draw moves the
    loss by more than six steps do -- measured on the MI355X: 5.0476 6.0275 4.9734 4.6900 4.6493 4.3756 6.1403."""
    B = 4
    c = lc.Cfg(device=DEV, simulator=None, widths=LAYER_WIDTH, num_class=101, size=128, B=B, dtype=torch.bfloat16)
    m = lc.module(c, seed=0)
    for k, q in m.named_parameters():
        if k.startswith(lc.EXTRACTOR):
            q.requires_grad_(False)
    opt = Adam(filter(lambda q: q.requires_grad, m.parameters()), lr=1e-3, weight_decay=1e-3)
    x = torch.randn(B, 8, 3, 5, 128, 128, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    target = (torch.arange(B, device=DEV) % 101).view(B, 1)
    crit = torch.nn.CrossEntropyLoss()
    init = {k: q.detach().clone() for k, q in m.named_parameters()}
    ones = (torch.ones(8, B * 16, 256, device=DEV), torch.ones(B, 256, device=DEV))

    def loss_without_dropout():
        m._forced_masks = ones
        with torch.no_grad():
            out, _ = m(x)
        m._forced_masks = None
        return crit(out.view(B, -1), target.view(-1)).item()

    before = loss_without_dropout()
    losses = [lc.ref_loop_step(m, opt, x, target, crit).item() for _ in range(6)]
    after = loss_without_dropout()
    print(f"bf16 head-mode: loss without dropout {before:.4f} -> {after:.4f}; the loop's own (fresh masks per step):",
          " ".join(f"{v:.4f}" for v in losses))
    assert all(torch.isfinite(torch.tensor(losses + [before, after]))) and after < before
    eng = m.engine
    for k, q in m.named_parameters():   # the extractor keeps its initial bits, the head moved
        assert torch.equal(q.detach().view(torch.int32), init[k].view(torch.int32)) == k.startswith(lc.EXTRACTOR), k
        o, n = eng.offsets[k]
        if k.startswith(lc.EXTRACTOR):
            assert eng.flat_m[o:o + n].abs().max().item() == 0 and eng.flat_v[o:o + n].abs().max().item() == 0, k
    assert eng.step_count == 6 and int(m.backbone.bn1.num_batches_tracked) == 8
