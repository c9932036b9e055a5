"""GPU tier: the symmetric InfoNCE on the MI355X -- the column pass and the _sym arms of the CE row kernels at every size of the CPU tier
and at 1 100, 2 056 (second register trip of the bf16 row form) and 8 200 (its NV = 8 form, the f32 form's NV = 16), the engine step at
the reference's widths (resnet18, num_seq 4, pred_step 2: 64 px / B = 2 with f32 logits, 128 px / B = 2 with bf16 logits) and the
captured step, with and without the bank and accumulation.  The cases are those of the CPU tier (tests/sym_cases.py)."""
import pytest
import torch

import kcases as kc
import loss_cases as lc
import sym_cases as sc
from dpc_amd import _lib as L
from dpc_amd.plan import LAYER_WIDTH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SQUARE_LIMIT = 2056


@pytest.fixture(scope="module")
def k():
    return kc.K(L.load_hip(), DEV)


@pytest.fixture(scope="module")
def cfg():
    return sc.Cfg(device=DEV, simulator=None, widths=LAYER_WIDTH)


@pytest.mark.parametrize("n", sc.KERNEL_N_GPU[:-1])   # (row_case at 8 200 square is gigabytes of f64 on the host: the size runs below)
def test_column_pass(k, n):
    sc.case_colpass(k, n)


@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("name", sc.square_shapes(lc.CE_SHAPES, SQUARE_LIMIT))
@pytest.mark.parametrize("mode", ["f32", "bf16", "null", "bf16-null"])
def test_zero_is_the_old_entry(k, name, mode, bank):
    sc.case_zero_is_the_old_entry(k, "dpc_ce_topk", name, mode, bank)


@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("name", sc.square_shapes(lc.CE16_SHAPES, SQUARE_LIMIT))
@pytest.mark.parametrize("mode", ["bf16", "null"])
def test_zero16_is_the_old_entry(k, name, mode, bank):
    sc.case_zero_is_the_old_entry(k, "dpc_ce_topk_bf16", name, mode, bank)


@pytest.mark.parametrize("entry,cols,gdt", [("dpc_ce_topk", 8196, torch.float32), ("dpc_ce_topk", 8196, torch.bfloat16),
                                            ("dpc_ce_topk_bf16", 8200, torch.bfloat16)])
def test_zero_is_the_old_entry_wide(k, entry, cols, gdt):
    sc.case_zero_big(k, entry, cols, gdt)


@pytest.mark.parametrize("W", sc.WEIGHTS)
@pytest.mark.parametrize("n", sc.KERNEL_N_GPU)
def test_weighted_loss_and_gradient(k, n, W):
    sc.case_weighted(k, n, W)


@pytest.mark.parametrize("n", sc.KERNEL_N_GPU)
def test_hot_cross(k, n):
    sc.case_hot_cross(k, n)


def test_refused_calls(k):
    sc.case_refused(k)


@pytest.mark.parametrize("arm", list(sc.ARMS))
def test_engine_off_is_off(cfg, arm):
    sc.case_off_is_off(cfg, arm)


@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("k_slots", [0, 2])
@pytest.mark.parametrize("arm", list(sc.ARMS))
def test_engine_by_hand(cfg, arm, k_slots, cosine):
    sc.case_by_hand(cfg, arm, k_slots, cosine)


@pytest.mark.parametrize("arm", list(sc.ARMS))
def test_engine_eval_between_train_steps(cfg, arm):
    sc.case_eval_between(cfg, arm)


def test_engine_accumulation_and_guard(cfg):
    sc.case_accum_and_guard(cfg)


def test_engine_checkpoint(cfg, tmp_path):
    sc.case_checkpoint(cfg, tmp_path)


def test_engine_refusals(cfg):
    sc.case_refusals(cfg)


@pytest.mark.parametrize("accum", [1, 2])
@pytest.mark.parametrize("k_slots", [0, 2])
@pytest.mark.parametrize("arm", list(sc.ARMS))
def test_engine_captured_step(cfg, arm, k_slots, accum):
    sc.case_captured(cfg, arm, k_slots, accum)
