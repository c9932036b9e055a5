"""CPU tier (host SIMT simulator): the parameter average of the fused Adam -- the kernels, the engine, checkpoints, optim.Adam(ema_decay=)
and the two entries' --ema / --ema_eval / --use_ema (tests/ema_cases.py)."""
import os
import subprocess

import pytest

import ema_cases as ec
import kcases as kc
from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def k():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return kc.K(L.load_emulator(), "cpu")


def test_exact(k):
    ec.case_exact(k)


def test_rounding(k):
    ec.case_rounding(k)


def test_warmup(k):
    ec.case_warmup(k)


def test_untouched(k):
    ec.case_untouched(k)


def test_swap_and_argument_checks(k):
    ec.case_swap_and_argument_checks(k)


WIDTHS = (8, 16, 32, 32)


@pytest.fixture(scope="module")
def cfg(k):
    return ec.Cfg(device="cpu", simulator=k.lib, widths=WIDTHS)


def test_ema_does_not_change_training(cfg):
    ec.case_ema_does_not_change_training(cfg)


def test_matches_the_host_recurrence(cfg):
    ec.case_matches_the_host_recurrence(cfg)


def test_evaluating_with_the_averaged_weights(cfg):
    ec.case_evaluating_with_the_averaged_weights(cfg)


def test_groups(cfg):
    ec.case_groups(cfg)


def test_checkpoint_round_trip(cfg, tmp_path):
    ec.case_checkpoint_round_trip(cfg, tmp_path)


def test_module_boundary(cfg):
    ec.case_module_boundary(cfg)


def test_entry_main(k, capsys, tmp_path):
    ec.case_entry_main(k.lib, WIDTHS, capsys, tmp_path)


def test_entry_lc(k, capsys, tmp_path):
    ec.case_entry_lc(k.lib, WIDTHS, capsys, tmp_path)


def test_flag_errors(k):
    ec.case_flag_errors(k.lib, WIDTHS)


def test_two_ranks(k, tmp_path):
    ec.case_two_ranks(k.lib, WIDTHS, tmp_path)
