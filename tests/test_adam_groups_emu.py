"""CPU tier (host SIMT simulator): the grouped Adam kernel against an f64 Adam (tests/adam_groups_cases.py), the head backward
from an upstream gradient against f64 torch autograd, and BackboneEngine.set_param_groups' table."""
import os
import subprocess

import pytest
import torch

import adam_groups_cases as ac
import kcases as kc
import lc_upstream_cases as uc
from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def k():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return kc.K(L.load_emulator(), "cpu")


def test_adam_groups_kernel(k):
    ac.case_adam_groups(k)
    ac.case_table_capacity()


def test_lc_head_bwd_from_upstream_gradient(k):
    uc.case_lc_head_upstream(k, torch.float32, 6, 3, 40, 11)
    uc.case_lc_head_upstream(k, torch.bfloat16, 6, 3, 40, 11)
