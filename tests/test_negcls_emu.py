"""CPU tier (host SIMT simulator): negative classes in the loss -- the _cls arms of the CE row kernels in every dispatcher form, the
engine step, its checkpoint entry and main --neg_weight / --neg_report (tests/negcls_cases.py).  The geometry with 8 448 columns runs on
the GPU tier only, and so does the engine arm with bf16 logits (R = 64 needs 128 px: minutes per step on the simulator); what that arm
adds below the engine -- dpc_ce_topk_bf16_cls -- is held by the kernel cases here."""
import os
import subprocess

import pytest

import kcases as kc
import loss_cases as lc
import negcls_cases as nc
from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (8, 16, 32, 32)
ARMS = ["f32 logits"]


@pytest.fixture(scope="module")
def k():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return kc.K(L.load_emulator(), "cpu")


@pytest.fixture(scope="module")
def cfg(k):
    return nc.Cfg(device="cpu", simulator=k.lib, widths=WIDTHS)


@pytest.mark.parametrize("geom", nc.GEOMS)
def test_class_map(k, geom):
    nc.case_class_map(k, geom)


@pytest.mark.parametrize("geom", nc.GEOMS)
def test_weighted_loss_and_gradient(k, geom):
    nc.case_weighted(k, geom)


@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("name", list(lc.CE_SHAPES))
@pytest.mark.parametrize("mode", ["f32", "bf16", "null", "bf16-null"])
def test_ones_is_the_old_entry(k, name, mode, bank):
    nc.case_ones_is_the_old_entry(k, "dpc_ce_topk", name, mode, bank)


@pytest.mark.parametrize("bank", [False, True])
@pytest.mark.parametrize("name", list(lc.CE16_SHAPES))
@pytest.mark.parametrize("mode", ["bf16", "null"])
def test_ones16_is_the_old_entry(k, name, mode, bank):
    nc.case_ones_is_the_old_entry(k, "dpc_ce_topk_bf16", name, mode, bank)


@pytest.mark.parametrize("geom", nc.GEOMS)
def test_hot_column_of_weight_zero(k, geom):
    nc.case_hot_zero(k, geom)


@pytest.mark.parametrize("geom", nc.GEOMS)
def test_report(k, geom):
    nc.case_report(k, geom)


@pytest.mark.parametrize("geom,D,K", nc.BANK_SHAPES)
def test_bank(k, geom, D, K):
    nc.case_bank(k, geom, D, K)


def test_refused_calls(k):
    nc.case_refused(k)


@pytest.mark.parametrize("arm", ARMS)
def test_engine_off_is_off(cfg, arm):
    nc.case_off_is_off(cfg, arm)


@pytest.mark.parametrize("arm", ARMS)
def test_engine_report_only(cfg, arm):
    nc.case_report_only(cfg, arm)


@pytest.mark.parametrize("k_slots", [0, 2])
@pytest.mark.parametrize("arm", ARMS)
def test_engine_by_hand(cfg, arm, k_slots):
    nc.case_by_hand(cfg, arm, k_slots)


@pytest.mark.parametrize("arm", ARMS)
def test_engine_temporal_off(cfg, arm):
    nc.case_temporal_off(cfg, arm)


@pytest.mark.parametrize("arm", ARMS)
def test_engine_eval_between_train_steps(cfg, arm):
    nc.case_eval_between(cfg, arm)


def test_engine_combined(cfg):
    nc.case_combined(cfg)


def test_engine_checkpoint(cfg, tmp_path):
    nc.case_checkpoint(cfg, tmp_path)


def test_engine_refusals(cfg):
    nc.case_refusals(cfg)


def test_engine_entry(k, capsys, tmp_path):
    nc.case_entry(k.lib, WIDTHS, capsys, tmp_path)
