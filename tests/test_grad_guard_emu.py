"""CPU tier (host SIMT simulator): the gradient guard's kernels, the guarded engine step, optim.clip_grad_norm_ and the two entries'
--clip_grad / --skip_nonfinite (tests/grad_guard_cases.py)."""
import os
import subprocess

import pytest

import grad_guard_cases as gc
import kcases as kc
from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def k():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return kc.K(L.load_emulator(), "cpu")


def test_exact_sum(k):
    gc.case_exact_sum(k)


def test_rounding(k):
    gc.case_rounding(k)


def test_verdict_table(k):
    gc.case_verdict_table(k)


def test_gated_update(k):
    gc.case_gated_update(k)


def test_grad_scale(k):
    gc.case_grad_scale(k)


def test_argument_checks(k):
    gc.case_argument_checks(k)


WIDTHS = (8, 16, 32, 32)


@pytest.fixture(scope="module")
def cfg(k):
    return gc.Cfg(device="cpu", simulator=k.lib, widths=WIDTHS)


def test_guard_that_never_bites(cfg):
    gc.case_guard_that_never_bites(cfg)


def test_clip(cfg):
    gc.case_clip(cfg)


def test_skip(cfg):
    gc.case_skip(cfg)


def test_groups(cfg):
    gc.case_groups(cfg)


def test_module_boundary(cfg):
    gc.case_module_boundary(cfg)


def test_entries(k, capsys):
    gc.case_entries(k.lib, WIDTHS, capsys)


def test_two_ranks(k, tmp_path):
    gc.case_two_ranks(k.lib, WIDTHS, tmp_path)
