"""The fused ConvGRU recurrence on the MI355X, held step by step: the cases of tests/gru_cases.py on libdpc_hip.so -- every gemm_acc
regime (D = 32 ... 256 in both dtypes), both wave counts at the engine's shape, 640 rows at D = 256, the three dropout sources, the LC
form, guard bands, poison, rejections and the two metamorphic row cases.  The largest case has 640 rows and 7 steps."""
import pytest
import torch

import gru_cases as gc
import kcases as kc
from dpc_amd import _lib as L

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def k():
    assert torch.cuda.is_available(), "GPU tier needs an MI355X"
    return kc.K(L.load_hip(), "cuda:0")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("name", list(gc.CASES))
def test_chain(k, name, dtype):
    gc.chain_case(k, "gpu", name, gc.CASES[name], dtype)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("waves", ["8", "4"])
def test_chain_engine_shape(k, monkeypatch, waves, dtype):
    monkeypatch.setenv("DPC_GRU_WAVES", waves)
    gc.chain_case(k, "gpu", f"engine waves {waves}", gc.ENGINE, dtype)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_chain_640_rows(k, dtype):
    gc.chain_case(k, "gpu", "rows640", gc.rows640(256), dtype)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_rows_are_independent(k, dtype):
    gc.rows_case(k, dtype)


def test_rejects(k):
    gc.gru_rejects_case(k)


def test_report(k):
    gc.report_case("gpu")
