"""CPU tier (host SIMT simulator): the cosine score -- its two kernels at every shape and dtype, the engine step by hand, the negative
queue on normalised keys, the module boundary, the checkpoint and main --score_norm (tests/score_norm_cases.py).  The kernel shape
(1100, 256), the engine arm with bf16 logits (R = 64 needs 128 px at B = 4, minutes per step on the simulator), the captured steps and
the training run are on the GPU tier only."""
import os
import subprocess

import pytest
import torch

import kcases as kc
import score_norm_cases as sn
from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (8, 16, 32, 32)
SHAPES = sn.KERNEL_SHAPES
ARM = "f32 logits"


@pytest.fixture(scope="module")
def k():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return kc.K(L.load_emulator(), "cpu")


@pytest.fixture(scope="module")
def cfg(k):
    return sn.Cfg(device="cpu", simulator=k.lib, widths=WIDTHS)


@pytest.mark.parametrize("dt", sn.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("R,D", SHAPES)
def test_fwd(k, R, D, dt):
    sn.case_fwd(k, R, D, dt)


@pytest.mark.parametrize("dt", sn.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("R,D", SHAPES)
def test_exact(k, R, D, dt):
    sn.case_exact(k, R, D, dt)


@pytest.mark.parametrize("dt", sn.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("R,D", SHAPES)
def test_edges(k, R, D, dt):
    sn.case_edges(k, R, D, dt)


@pytest.mark.parametrize("dt", sn.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("R,D", SHAPES)
def test_bwd(k, R, D, dt):
    sn.case_bwd(k, R, D, dt)


def test_refused_calls(k):
    sn.case_refused(k)


def test_off_is_off(cfg):
    sn.case_off_is_off(cfg, ARM)


@pytest.mark.parametrize("T,dt", [(0.07, torch.bfloat16), (0.5, torch.bfloat16), (0.07, torch.float32)], ids=["T0.07-bf16", "T0.5-bf16", "T0.07-f32"])
def test_by_hand(cfg, T, dt):
    sn.case_by_hand(cfg, ARM, T, dt)


def test_range_and_norms(cfg):
    sn.case_range_and_norms(cfg, ARM)


def test_predictor_scale(cfg):
    sn.case_predictor_scale(cfg, ARM)


def test_queue(cfg):
    sn.case_queue(cfg, ARM)


def test_module(cfg):
    sn.case_module(cfg, ARM)


def test_combination(cfg):
    sn.case_combination(cfg, ARM)


def test_checkpoint(cfg, tmp_path):
    sn.case_checkpoint(cfg, ARM, tmp_path)


def test_refusals(cfg):
    sn.case_refusals(cfg, ARM)


def test_fused_route(cfg):
    sn.case_fused_route(cfg, ARM)


def test_entry(k, capsys):
    sn.case_entry(k.lib, WIDTHS, capsys)
