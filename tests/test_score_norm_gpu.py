"""GPU tier: the cosine score on the MI355X -- its two kernels at every shape of the CPU tier and (1100, 256), the engine step at the
reference's widths (resnet18, num_seq 4, pred_step 1: 64 px / B = 2 with f32 logits, 128 px / B = 4 with bf16 logits), the captured
steps (with and without the negative queue and accumulation) and a short training run.  The cases are those of the CPU tier
(tests/score_norm_cases.py)."""
import pytest
import torch

import kcases as kc
import score_norm_cases as sn
from dpc_amd import _lib as L
from dpc_amd.plan import LAYER_WIDTH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = sn.KERNEL_SHAPES_GPU
ARMS = list(sn.ARMS)
SMALL = "f32 logits"


@pytest.fixture(scope="module")
def k():
    return kc.K(L.load_hip(), DEV)


@pytest.fixture(scope="module")
def cfg():
    return sn.Cfg(device=DEV, simulator=None, widths=LAYER_WIDTH)


@pytest.mark.parametrize("dt", sn.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("R,D", SHAPES)
def test_fwd(k, R, D, dt):
    sn.case_fwd(k, R, D, dt)


@pytest.mark.parametrize("dt", sn.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("R,D", SHAPES)
def test_exact(k, R, D, dt):
    sn.case_exact(k, R, D, dt)


@pytest.mark.parametrize("dt", sn.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("R,D", SHAPES)
def test_edges(k, R, D, dt):
    sn.case_edges(k, R, D, dt)


@pytest.mark.parametrize("dt", sn.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("R,D", SHAPES)
def test_bwd(k, R, D, dt):
    sn.case_bwd(k, R, D, dt)


def test_refused_calls(k):
    sn.case_refused(k)


@pytest.mark.parametrize("arm", ARMS)
def test_off_is_off(cfg, arm):
    sn.case_off_is_off(cfg, arm)


def test_off_is_off_f32(cfg):
    sn.case_off_is_off(cfg, SMALL, torch.float32)


@pytest.mark.parametrize("T", [0.07, 0.5])
@pytest.mark.parametrize("arm", ARMS)
def test_by_hand(cfg, arm, T):
    sn.case_by_hand(cfg, arm, T)


def test_by_hand_f32(cfg):
    sn.case_by_hand(cfg, SMALL, 0.07, torch.float32)


@pytest.mark.parametrize("arm", ARMS)
def test_range_and_norms(cfg, arm):
    sn.case_range_and_norms(cfg, arm)


@pytest.mark.parametrize("arm", ARMS)
def test_predictor_scale(cfg, arm):
    sn.case_predictor_scale(cfg, arm)


@pytest.mark.parametrize("arm", ARMS)
def test_queue(cfg, arm):
    sn.case_queue(cfg, arm)


def test_module(cfg):
    sn.case_module(cfg, SMALL)


@pytest.mark.parametrize("arm", ARMS)
def test_combination(cfg, arm):
    sn.case_combination(cfg, arm)


def test_checkpoint(cfg, tmp_path):
    sn.case_checkpoint(cfg, SMALL, tmp_path)


def test_refusals(cfg):
    sn.case_refusals(cfg, SMALL)


@pytest.mark.parametrize("arm", ARMS)
def test_fused_route(cfg, arm):
    sn.case_fused_route(cfg, arm)


@pytest.mark.parametrize("accum", [1, 2])
@pytest.mark.parametrize("k_slots", [0, 2])
@pytest.mark.parametrize("arm", ARMS)
def test_captured_step(cfg, arm, k_slots, accum):
    sn.case_captured(cfg, arm, k_slots, accum)


def test_training(cfg):
    sn.case_training(cfg, SMALL)
