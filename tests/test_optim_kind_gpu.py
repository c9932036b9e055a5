"""GPU tier: AdamW and LAMB in the fused step on the MI355X -- the kernels, the engine (resnet18 at the reference's widths, 64 px, B = 2,
num_seq 4, pred_step 1; f32, plus bf16 where the case says so), the captured step, checkpoints, optim.AdamW / optim.LAMB and
lc_main --graph --optimizer lamb across an epoch milestone.  The cases are those of the CPU tier (tests/optim_kind_cases.py)."""
import pytest
import torch

import kcases as kc
import optim_kind_cases as oc
from dpc_amd import _lib as L
from dpc_amd.plan import LAYER_WIDTH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def k():
    return kc.K(L.load_hip(), DEV)


@pytest.fixture(scope="module")
def cfg():
    return oc.Cfg(device=DEV, simulator=None, widths=LAYER_WIDTH)


def test_adamw_identity(k):
    oc.case_adamw_identity(k)


def test_adamw_f64(k):
    oc.case_adamw_f64(k)


def test_lamb_sum_p2_exact(k):
    oc.case_lamb_sum_p2_exact(k)


def test_lamb_f64(k):
    oc.case_lamb_f64(k)


def test_lamb_degenerate(k):
    oc.case_lamb_degenerate(k)


def test_skip_and_coef(k):
    oc.case_skip_and_coef(k)


def test_argument_checks(k):
    oc.case_argument_checks(k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_adam_is_adam(cfg, dtype):
    oc.case_adam_is_adam(cfg, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_adamw_without_decay(cfg, dtype):
    oc.case_adamw_without_decay(cfg, dtype)


def test_launch_counts(cfg):
    oc.case_launch_counts(cfg)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_recurrence(cfg, kind):
    oc.case_recurrence(cfg, kind)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_recurrence_groups(cfg, kind):
    oc.case_recurrence_groups(cfg, kind, num_class=101)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_combined(cfg, kind):
    oc.case_combined(cfg, kind)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_checkpoint(cfg, kind, tmp_path):
    oc.case_checkpoint(cfg, kind, tmp_path)


def test_torch_adamw_continuation(cfg, tmp_path):
    oc.case_torch_adamw_continuation(cfg, tmp_path)


@pytest.mark.parametrize("kind", oc.KINDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_captured_step(cfg, kind, dtype):
    oc.case_captured_step(cfg, kind, dtype)


def test_module_boundary(cfg):
    oc.case_module_boundary(cfg, num_class=101)


def test_entry_lc_graph_across_an_epoch_milestone(capsys, tmp_path):
    oc.case_entry_lc(None, None, capsys, tmp_path, graph=True)
