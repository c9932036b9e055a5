"""The loss family on the MI355X, held per row: the cases of tests/loss_cases.py on libdpc_hip.so -- every form and form boundary of the
row kernels behind dpc_ce_topk / dpc_ce_topk_bf16, dpc_ce_finalize on its own, and the forward of the fused score on exact operands
(here also at R = 1 100, D = 256: four column splits, the last one short).  Every case has at most 40 rows."""
import pytest
import torch

import kcases as kc
import loss_cases as lc
from dpc_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def k():
    assert torch.cuda.is_available(), "GPU tier needs an MI355X"
    return kc.K(L.load_hip(), "cuda:0")


@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16-null"])
@pytest.mark.parametrize("name", list(lc.CE_SHAPES))
def test_ce_rows(k, name, mode):
    lc.ce_rows_case(k, "dpc_ce_topk", name, mode)


@pytest.mark.parametrize("mode", ["bf16", "null"])
@pytest.mark.parametrize("name", list(lc.CE16_SHAPES))
def test_ce_rows_bf16_logits(k, name, mode):
    lc.ce_rows_case(k, "dpc_ce_topk_bf16", name, mode)


def test_ce_rejects(k):
    lc.ce_rejects_case(k)


@pytest.mark.parametrize("rows", lc.FINALIZE_ROWS)
def test_ce_finalize(k, rows):
    lc.ce_finalize_case(k, rows)


@pytest.mark.parametrize("rd", lc.SCORE_SHAPES_GPU)
def test_score_fwd_exact(k, rd):
    lc.score_fwd_case(k, *rd)
