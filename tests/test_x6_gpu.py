"""GPU tier: the f32 contraction kernels of libdpc_hip.so on a real MI355X in both arithmetics ("exact" f32 MFMA chains and "bf16x6",
include/dpc_hip.h: dpc_set_f32_matmul), held term by term to f64 references (tests/x6_cases.py: a bound of 1/4 of what the smallest
of the six piece products is worth, on random operands and on the three piece probes).  Run with -s to see error, bound and kernel of
every case and mode."""
import pytest
import torch

import x6_cases as xc
from dpc_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def k():
    assert torch.cuda.is_available(), "GPU tier needs an MI355X"
    k = xc.K(L.load_hip(), "cuda:0")
    k.mode_before = xc.current_mode(k)
    yield k
    xc.print_results()


@pytest.mark.parametrize("case,kind", xc.PARAMS, ids=[f"{c.name}-{kind}" for c, kind in xc.PARAMS])
def test_f32_contraction(k, case, kind):
    xc.run_case(k, case, kind, "MI355X")


def test_switch_is_left_as_found(k):
    """after every case above: the library multiplies as it did before, and lib._f32_mode -- which the engine trusts -- says so"""
    assert xc.current_mode(k) == k.mode_before == getattr(k.lib, "_f32_mode", 0)
