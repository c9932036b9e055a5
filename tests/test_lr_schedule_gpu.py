"""GPU tier: the per-step learning-rate schedule of the fused step on the MI355X -- the kernels, the engine (resnet18 at the reference's
widths, 64 px, B = 2, num_seq 4, pred_step 1; f32, plus bf16 where the case says so), the captured step, checkpoints,
optim.Adam(lr_schedule=) and lc_main --graph across an epoch milestone.  The cases are those of the CPU tier
(tests/lr_schedule_cases.py)."""
import pytest
import torch

import kcases as kc
import lr_schedule_cases as sc
from dpc_amd import _lib as L
from dpc_amd.plan import LAYER_WIDTH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def k():
    return kc.K(L.load_hip(), DEV)


@pytest.fixture(scope="module")
def cfg():
    return sc.Cfg(device=DEV, simulator=None, widths=LAYER_WIDTH)


def test_multiplier_table(k):
    sc.case_multiplier_table(k)


def test_identity(k):
    sc.case_identity(k)


def test_scaling_exact(k):
    sc.case_scaling_exact(k)


def test_scaling_rounding(k):
    sc.case_scaling_rounding(k)


def test_argument_checks(k):
    sc.case_argument_checks(k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_off_is_off(cfg, dtype):
    sc.case_off_is_off(cfg, dtype)


def test_host_driven_twin(cfg):
    sc.case_host_driven_twin(cfg)


def test_host_driven_twin_groups(cfg):
    sc.case_host_driven_twin_groups(cfg, num_class=101)


def test_with_the_guard(cfg):
    sc.case_with_the_guard(cfg)


def test_with_ema(cfg):
    sc.case_with_ema(cfg)


def test_checkpoint(cfg, tmp_path):
    sc.case_checkpoint(cfg, tmp_path)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_captured_step(cfg, dtype):
    sc.case_captured_step(cfg, dtype)


def test_module_boundary(cfg):
    sc.case_module_boundary(cfg, num_class=101)


def test_entry_lc_graph_across_an_epoch_milestone(capsys, tmp_path):
    sc.case_entry_lc(None, None, capsys, tmp_path, graph=True)
