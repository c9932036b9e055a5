"""GPU tier: the gradient guard on the MI355X -- the kernels, the guarded engine step (resnet18 at the reference's widths, 64 px, B = 2,
num_seq 4, pred_step 1; f32, plus one bf16 run of the never-biting guard and of the skip), the captured step and
optim.clip_grad_norm_.  The cases are those of the CPU tier (tests/grad_guard_cases.py)."""
import pytest
import torch

import grad_guard_cases as gc
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
    return gc.Cfg(device=DEV, simulator=None, widths=LAYER_WIDTH)


def test_exact_sum(k):
    gc.case_exact_sum(k)


def test_rounding(k):
    gc.case_rounding(k)


def test_verdict_table(k):
    gc.case_verdict_table(k)


def test_gated_update(k):
    gc.case_gated_update(k)


def test_grad_scale(k):
    gc.case_grad_scale(k)


def test_argument_checks(k):
    gc.case_argument_checks(k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_guard_that_never_bites(cfg, dtype):
    gc.case_guard_that_never_bites(cfg, dtype)


def test_clip(cfg):
    gc.case_clip(cfg)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_skip(cfg, dtype):
    gc.case_skip(cfg, dtype)


def test_groups(cfg):
    gc.case_groups(cfg, num_class=101)


def test_captured_step(cfg):
    gc.case_captured_step(cfg)


def test_module_boundary(cfg):
    gc.case_module_boundary(cfg, num_class=101)
