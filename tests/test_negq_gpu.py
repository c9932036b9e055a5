"""GPU tier: the negative queue on the MI355X -- its kernels at every shape of the CPU tier and (1100, 256, 4), the _ext arms of the CE row
kernels, the engine step at the reference's widths (resnet18, num_seq 4, pred_step 1: 64 px / B = 2 with f32 logits, 128 px / B = 4 with
bf16 logits) and the captured step, with and without accumulation.  The cases are those of the CPU tier (tests/negq_cases.py)."""
import pytest

import kcases as kc
import negq_cases as nq
from dpc_amd import _lib as L
from dpc_amd.plan import LAYER_WIDTH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = nq.KERNEL_SHAPES_GPU
EXT_FORMS = [("dpc_ce_topk", "sweep_37"), ("dpc_ce_topk", "nv8_1028"), ("dpc_ce_topk", "nv16_8196")]
EXT16_FORMS = ["vec16x4_2056", "vec16x8_8200"]


@pytest.fixture(scope="module")
def k():
    return kc.K(L.load_hip(), DEV)


@pytest.fixture(scope="module")
def cfg():
    return nq.Cfg(device=DEV, simulator=None, widths=LAYER_WIDTH)


@pytest.mark.parametrize("R,D,K", SHAPES)
def test_push(k, R, D, K):
    nq.case_push(k, R, D, K)


@pytest.mark.parametrize("R,D,K", SHAPES)
def test_fwd(k, R, D, K):
    nq.case_fwd(k, R, D, K)


@pytest.mark.parametrize("entry,name", EXT_FORMS)
@pytest.mark.parametrize("mode", ["f32", "bf16", "null", "bf16-null"])
def test_ext_empty_is_the_old_entry(k, entry, name, mode):
    nq.case_ext_empty(k, entry, name, mode)


@pytest.mark.parametrize("name", EXT16_FORMS)
@pytest.mark.parametrize("mode", ["bf16", "null"])
def test_ext16_empty_is_the_old_entry(k, name, mode):
    nq.case_ext_empty(k, "dpc_ce_topk_bf16", name, mode)


@pytest.mark.parametrize("R,D,K", SHAPES)
def test_ext_with_a_bank(k, R, D, K):
    nq.case_ext_bank(k, R, D, K)


@pytest.mark.parametrize("R,D,K", SHAPES)
def test_bwd(k, R, D, K):
    nq.case_bwd(k, R, D, K)


def test_refused_calls(k):
    nq.case_refused(k)


@pytest.mark.parametrize("arm", list(nq.ARMS))
def test_empty_bank_is_no_bank(cfg, arm):
    nq.case_empty_bank_is_no_bank(cfg, arm)


@pytest.mark.parametrize("arm", list(nq.ARMS))
def test_by_hand(cfg, arm):
    nq.case_by_hand(cfg, arm)


@pytest.mark.parametrize("arm", list(nq.ARMS))
def test_eval_between_train_steps(cfg, arm):
    nq.case_eval_between(cfg, arm)


def test_nan_empties_the_bank(cfg):
    nq.case_nan_empties_the_bank(cfg)


def test_accumulation(cfg):
    nq.case_accumulation(cfg)


def test_checkpoint(cfg, tmp_path):
    nq.case_checkpoint(cfg, tmp_path)


def test_refusals(cfg):
    nq.case_refusals(cfg)


@pytest.mark.parametrize("arm", list(nq.ARMS))
def test_captured_step(cfg, arm):
    nq.case_captured(cfg, arm)


@pytest.mark.parametrize("arm", list(nq.ARMS))
def test_captured_step_accumulation(cfg, arm):
    nq.case_captured(cfg, arm, accum=2)
