"""GPU tier: the parameter average of the fused Adam on the MI355X -- the kernels, the engine (resnet18 at the reference's widths, 64 px,
B = 2, num_seq 4, pred_step 1; f32, plus one bf16 run of "the average does not change training"), the captured step, checkpoints and
optim.Adam(ema_decay=).  The cases are those of the CPU tier (tests/ema_cases.py)."""
import pytest
import torch

import ema_cases as ec
import kcases as kc
from dpc_amd import _lib as L
from dpc_amd.plan import LAYER_WIDTH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def k():
    return kc.K(L.load_hip(), DEV)


@pytest.fixture(scope="module")
def cfg():
    return ec.Cfg(device=DEV, simulator=None, widths=LAYER_WIDTH)


def test_exact(k):
    ec.case_exact(k)


def test_rounding(k):
    ec.case_rounding(k)


def test_warmup(k):
    ec.case_warmup(k)


def test_untouched(k):
    ec.case_untouched(k)


def test_swap_and_argument_checks(k):
    ec.case_swap_and_argument_checks(k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ema_does_not_change_training(cfg, dtype):
    ec.case_ema_does_not_change_training(cfg, dtype)


def test_matches_the_host_recurrence(cfg):
    ec.case_matches_the_host_recurrence(cfg)


def test_evaluating_with_the_averaged_weights(cfg):
    ec.case_evaluating_with_the_averaged_weights(cfg)


def test_groups(cfg):
    ec.case_groups(cfg, num_class=101)


def test_checkpoint_round_trip(cfg, tmp_path):
    ec.case_checkpoint_round_trip(cfg, tmp_path)


def test_captured_step(cfg):
    ec.case_captured_step(cfg)


def test_module_boundary(cfg):
    ec.case_module_boundary(cfg, num_class=101)
