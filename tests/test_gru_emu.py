"""The fused ConvGRU recurrence on the host simulator, held step by step: every saved tensor of dpc_gru_chain_fwd / _bwd against an f64
reference recomputed from the kernel's own stored operands, per element.  The case bodies, the data and the bounds are in
tests/gru_cases.py; the MI355X runs the same ones (tests/test_gru_gpu.py)."""
import os
import subprocess

import pytest
import torch

import gru_cases as gc
import kcases as kc
from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def k():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return kc.K(L.load_emulator(), "cpu")


def test_slipped_mutation():
    gc.slipped_mutation_case()


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("name", list(gc.CASES))
def test_chain(k, name, dtype):
    gc.chain_case(k, "emu", name, gc.CASES[name], dtype)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("waves", ["8", "4"])
def test_chain_engine_shape(k, monkeypatch, waves, dtype):
    monkeypatch.setenv("DPC_GRU_WAVES", waves)
    gc.chain_case(k, "emu", f"engine waves {waves}", gc.ENGINE, dtype)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_chain_640_rows(k, dtype):
    gc.chain_case(k, "emu", "rows640", gc.rows640(64), dtype)   # the MI355X tier runs D = 256


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_rows_are_independent(k, dtype):
    gc.rows_case(k, dtype)


def test_rejects(k):
    gc.gru_rejects_case(k)


def test_report():
    gc.report_case("emu")
