"""CPU tier (host SIMT simulator): dpc_grad_accumulate, the accumulating engine step of both heads, its checkpoint, two gloo ranks and
the two entries' --accum_steps (tests/accum_cases.py)."""
import os
import subprocess

import pytest

import accum_cases as acc
import kcases as kc
from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (8, 16, 32, 32)


@pytest.fixture(scope="module")
def k():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return kc.K(L.load_emulator(), "cpu")


@pytest.fixture(scope="module")
def cfg(k):
    return acc.Cfg(device="cpu", simulator=k.lib, widths=WIDTHS)


def test_bit_identity(k):
    acc.case_bit_identity(k)


def test_integer_data(k):
    acc.case_integer_data(k)


def test_segment_table(k):
    acc.case_segment_table(k)


def test_range(k):
    acc.case_range(k)


def test_refused_calls(k):
    acc.case_refused_calls(k)


def test_off_is_the_engine_as_it_was(cfg):
    acc.case_off_is_the_engine_as_it_was(cfg)


def test_against_a_by_hand_twin(cfg):
    acc.case_against_a_by_hand_twin(cfg)


def test_against_f64_adam(cfg):
    acc.case_against_f64_adam(cfg, check_rejection=True)


def test_dropped_cycle(cfg):
    acc.case_dropped_cycle(cfg)


def test_lc_head_groups(cfg):
    acc.case_lc_head_groups(cfg)


def test_checkpoint(cfg, tmp_path):
    acc.case_checkpoint(cfg, tmp_path)


def test_two_ranks(k, tmp_path):
    acc.case_two_ranks(WIDTHS, tmp_path)


def test_entries(k, capsys):
    acc.case_entries(k.lib, WIDTHS, capsys)
