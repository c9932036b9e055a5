"""CPU tier (host SIMT simulator): the symmetric InfoNCE -- the column pass, the _sym arms of the CE row kernels in every dispatcher form
that a square matrix of up to 1 100 columns reaches, the engine step, its checkpoint entry and main --loss_sym (tests/sym_cases.py).
The wider forms (second register trip of the bf16 row form, NV = 16 / NV = 8) run on the GPU tier only, and so does the engine arm with
bf16 logits (R = 64 needs 128 px: minutes per step on the simulator); what that arm adds below the engine -- dpc_ce_topk_bf16_sym -- is
held by the kernel cases here."""
import os
import subprocess

import pytest

import kcases as kc
import loss_cases as lc
import sym_cases as sc
from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (8, 16, 32, 32)
ARMS = ["f32 logits"]
SQUARE_LIMIT = 1100


@pytest.fixture(scope="module")
def k():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return kc.K(L.load_emulator(), "cpu")


@pytest.fixture(scope="module")
def cfg(k):
    return sc.Cfg(device="cpu", simulator=k.lib, widths=WIDTHS)


@pytest.mark.parametrize("n", sc.KERNEL_N)
def test_column_pass(k, n):
    sc.case_colpass(k, n)


@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("name", sc.square_shapes(lc.CE_SHAPES, SQUARE_LIMIT))
@pytest.mark.parametrize("mode", ["f32", "bf16", "null", "bf16-null"])
def test_zero_is_the_old_entry(k, name, mode, bank):
    sc.case_zero_is_the_old_entry(k, "dpc_ce_topk", name, mode, bank)


@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("name", sc.square_shapes(lc.CE16_SHAPES, SQUARE_LIMIT))
@pytest.mark.parametrize("mode", ["bf16", "null"])
def test_zero16_is_the_old_entry(k, name, mode, bank):
    sc.case_zero_is_the_old_entry(k, "dpc_ce_topk_bf16", name, mode, bank)


@pytest.mark.parametrize("W", sc.WEIGHTS)
@pytest.mark.parametrize("n", sc.KERNEL_N)
def test_weighted_loss_and_gradient(k, n, W):
    sc.case_weighted(k, n, W)


@pytest.mark.parametrize("n", sc.KERNEL_N)
def test_hot_cross(k, n):
    sc.case_hot_cross(k, n)


def test_refused_calls(k):
    sc.case_refused(k)


@pytest.mark.parametrize("arm", ARMS)
def test_engine_off_is_off(cfg, arm):
    sc.case_off_is_off(cfg, arm)


@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("k_slots", [0, 2])
@pytest.mark.parametrize("arm", ARMS)
def test_engine_by_hand(cfg, arm, k_slots, cosine):
    sc.case_by_hand(cfg, arm, k_slots, cosine)


@pytest.mark.parametrize("arm", ARMS)
def test_engine_eval_between_train_steps(cfg, arm):
    sc.case_eval_between(cfg, arm)


def test_engine_accumulation_and_guard(cfg):
    sc.case_accum_and_guard(cfg)


def test_engine_checkpoint(cfg, tmp_path):
    sc.case_checkpoint(cfg, tmp_path)


def test_engine_refusals(cfg):
    sc.case_refusals(cfg)


def test_engine_entry(k, capsys, tmp_path):
    sc.case_entry(k.lib, WIDTHS, capsys, tmp_path)
