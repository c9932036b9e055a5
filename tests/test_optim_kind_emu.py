"""CPU tier (host SIMT simulator): AdamW and LAMB in the fused step -- the kernels, the engine, checkpoints, optim.AdamW / optim.LAMB and
the two entries' --optimizer flags (tests/optim_kind_cases.py).  The multi-step engine cases run the simulator's engine in bf16 compute,
where a step costs a third of an f32 one; the arenas and the update are f32 either way."""
import os
import subprocess

import pytest
import torch

import kcases as kc
import optim_kind_cases as oc
from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (8, 16, 32, 32)
DT = torch.bfloat16


@pytest.fixture(scope="module")
def k():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return kc.K(L.load_emulator(), "cpu")


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


@pytest.fixture(scope="module")
def cfg(k):
    return oc.Cfg(device="cpu", simulator=k.lib, widths=WIDTHS)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_adam_is_adam(cfg, dtype):
    oc.case_adam_is_adam(cfg, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_adamw_without_decay(cfg, dtype):
    oc.case_adamw_without_decay(cfg, dtype)


def test_launch_counts(cfg):
    oc.case_launch_counts(cfg, DT)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_recurrence(cfg, kind):
    oc.case_recurrence(cfg, kind, DT)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_recurrence_groups(cfg, kind):
    oc.case_recurrence_groups(cfg, kind)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_combined(cfg, kind):
    oc.case_combined(cfg, kind, DT)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_checkpoint(cfg, kind, tmp_path):
    oc.case_checkpoint(cfg, kind, tmp_path, DT)


def test_torch_adamw_continuation(cfg, tmp_path):
    oc.case_torch_adamw_continuation(cfg, tmp_path)


def test_module_boundary(cfg):
    oc.case_module_boundary(cfg, dtype=DT)


def test_entry_main(k, capsys, tmp_path):
    oc.case_entry_main(k.lib, WIDTHS, capsys, tmp_path)


def test_entry_lc(k, capsys, tmp_path):
    oc.case_entry_lc(k.lib, WIDTHS, capsys, tmp_path)


def test_flag_errors(k):
    oc.case_flag_errors(k.lib, WIDTHS)


def test_two_ranks(k, tmp_path):
    oc.case_two_ranks(k.lib, WIDTHS, tmp_path)
