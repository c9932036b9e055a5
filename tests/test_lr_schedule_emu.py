"""CPU tier (host SIMT simulator): the per-step learning-rate schedule of the fused step -- the kernels, the engine, checkpoints,
optim.Adam(lr_schedule=) and the two entries' --lr_schedule flags (tests/lr_schedule_cases.py).  The multi-step engine cases run the
simulator's engine in bf16 compute, where a step costs a third of an f32 one; the arenas and the update are f32 either way."""
import os
import subprocess

import pytest
import torch

import kcases as kc
import lr_schedule_cases as sc
from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (8, 16, 32, 32)
DT = torch.bfloat16


@pytest.fixture(scope="module")
def k():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return kc.K(L.load_emulator(), "cpu")


def test_multiplier_table(k):
    sc.case_multiplier_table(k)


def test_identity(k):
    sc.case_identity(k)


def test_scaling_exact(k):
    sc.case_scaling_exact(k)


def test_scaling_rounding(k):
    sc.case_scaling_rounding(k)


def test_argument_checks(k):
    sc.case_argument_checks(k)


@pytest.fixture(scope="module")
def cfg(k):
    return sc.Cfg(device="cpu", simulator=k.lib, widths=WIDTHS)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_off_is_off(cfg, dtype):
    sc.case_off_is_off(cfg, dtype)


def test_host_driven_twin(cfg):
    sc.case_host_driven_twin(cfg, DT)


def test_host_driven_twin_groups(cfg):
    sc.case_host_driven_twin_groups(cfg, dtype=DT)


def test_with_the_guard(cfg):
    sc.case_with_the_guard(cfg, DT)


def test_with_ema(cfg):
    sc.case_with_ema(cfg, DT)


def test_checkpoint(cfg, tmp_path):
    sc.case_checkpoint(cfg, tmp_path, DT)


def test_module_boundary(cfg):
    sc.case_module_boundary(cfg)


def test_entry_main(k, capsys, tmp_path):
    sc.case_entry_main(k.lib, WIDTHS, capsys, tmp_path)


def test_entry_lc(k, capsys, tmp_path):
    sc.case_entry_lc(k.lib, WIDTHS, capsys, tmp_path)


def test_flag_errors(k):
    sc.case_flag_errors(k.lib, WIDTHS)


def test_two_ranks(k, tmp_path):
    sc.case_two_ranks(k.lib, WIDTHS, tmp_path)
