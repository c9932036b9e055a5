"""The loss family on the host simulator, held per row: the row kernels behind dpc_ce_topk / dpc_ce_topk_bf16 in every form and at every
form boundary, dpc_ce_finalize on its own, and the forward of the fused score on exact operands.  The case bodies, the data and the
bounds are in tests/loss_cases.py; the MI355X runs the same ones (tests/test_loss_gpu.py)."""
import os
import subprocess

import pytest

import kcases as kc
import loss_cases as lc
from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def k():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return kc.K(L.load_emulator(), "cpu")


@pytest.mark.parametrize("cols,U", sorted({(v[0], 4) for v in lc.CE_SHAPES.values()} | {(v[0], 8) for v in lc.CE16_SHAPES.values()}))
def test_planted_rows_are_exact(cols, U):
    lc.data_is_exact_case(cols, U)


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


@pytest.mark.parametrize("rd", lc.SCORE_SHAPES)
def test_score_fwd_exact(k, rd):
    lc.score_fwd_case(k, *rd)
