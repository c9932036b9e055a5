"""GPU tier: negative classes in the loss on the MI355X -- the _cls arms of the CE row kernels at every geometry of the CPU tier and
(11, 3, 256) with 800 rows (8 448 columns: the NV 16 / NV 8 arms), the engine step at the reference's widths (resnet18, num_seq 4,
pred_step 2: 64 px / B = 2 with f32 logits, 128 px / B = 2 with bf16 logits) and the captured step, with and without the bank and
accumulation.  The cases are those of the CPU tier (tests/negcls_cases.py)."""
import pytest

import kcases as kc
import loss_cases as lc
import negcls_cases as nc
from dpc_amd import _lib as L
from dpc_amd.plan import LAYER_WIDTH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GEOMS = nc.GEOMS + (nc.GEOM_GPU,)


@pytest.fixture(scope="module")
def k():
    return kc.K(L.load_hip(), DEV)


@pytest.fixture(scope="module")
def cfg():
    return nc.Cfg(device=DEV, simulator=None, widths=LAYER_WIDTH)


@pytest.mark.parametrize("geom", GEOMS)
def test_class_map(k, geom):
    nc.case_class_map(k, geom)


@pytest.mark.parametrize("geom", GEOMS)
def test_weighted_loss_and_gradient(k, geom):
    nc.case_weighted(k, geom)


@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("name", list(lc.CE_SHAPES))
@pytest.mark.parametrize("mode", ["f32", "bf16", "null", "bf16-null"])
def test_ones_is_the_old_entry(k, name, mode, bank):
    nc.case_ones_is_the_old_entry(k, "dpc_ce_topk", name, mode, bank)


@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("name", list(lc.CE16_SHAPES))
@pytest.mark.parametrize("mode", ["bf16", "null"])
def test_ones16_is_the_old_entry(k, name, mode, bank):
    nc.case_ones_is_the_old_entry(k, "dpc_ce_topk_bf16", name, mode, bank)


@pytest.mark.parametrize("geom", GEOMS)
def test_hot_column_of_weight_zero(k, geom):
    nc.case_hot_zero(k, geom)


@pytest.mark.parametrize("geom", GEOMS)
def test_report(k, geom):
    nc.case_report(k, geom)


@pytest.mark.parametrize("geom,D,K", nc.BANK_SHAPES)
def test_bank(k, geom, D, K):
    nc.case_bank(k, geom, D, K)


def test_refused_calls(k):
    nc.case_refused(k)


@pytest.mark.parametrize("arm", list(nc.ARMS))
def test_engine_off_is_off(cfg, arm):
    nc.case_off_is_off(cfg, arm)


@pytest.mark.parametrize("arm", list(nc.ARMS))
def test_engine_report_only(cfg, arm):
    nc.case_report_only(cfg, arm)


@pytest.mark.parametrize("k_slots", [0, 2])
@pytest.mark.parametrize("arm", list(nc.ARMS))
def test_engine_by_hand(cfg, arm, k_slots):
    nc.case_by_hand(cfg, arm, k_slots)


@pytest.mark.parametrize("arm", list(nc.ARMS))
def test_engine_temporal_off(cfg, arm):
    nc.case_temporal_off(cfg, arm)


@pytest.mark.parametrize("arm", list(nc.ARMS))
def test_engine_eval_between_train_steps(cfg, arm):
    nc.case_eval_between(cfg, arm)


def test_engine_combined(cfg):
    nc.case_combined(cfg)


def test_engine_checkpoint(cfg, tmp_path):
    nc.case_checkpoint(cfg, tmp_path)


def test_engine_refusals(cfg):
    nc.case_refusals(cfg)


@pytest.mark.parametrize("accum", [1, 2])
@pytest.mark.parametrize("k_slots", [0, 2])
@pytest.mark.parametrize("arm", list(nc.ARMS))
def test_engine_captured_step(cfg, arm, k_slots, accum):
    nc.case_captured(cfg, arm, k_slots, accum)
