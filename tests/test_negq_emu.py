"""CPU tier (host SIMT simulator): the negative queue -- its kernels, the _ext arms of the CE row kernels, the engine step, its
checkpoint, two gloo ranks and main --neg_queue (tests/negq_cases.py).  The largest kernel shape runs on the GPU tier only, and so does
the engine arm with bf16 logits: R = 64 needs 128 px at B = 4, minutes per step on the simulator.  What that arm adds below the engine
-- dpc_ce_topk_bf16_ext and a bf16 target logit for dpc_negq_fwd -- is held by the kernel cases here."""
import os
import subprocess

import pytest

import kcases as kc
import loss_cases as lc
import negq_cases as nq
from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (8, 16, 32, 32)
SHAPES = nq.KERNEL_SHAPES            # (200, 32, 2): padded pitch; (520, 32, 3): several column splits; every K wraps in the push case
EXT_FORMS = [("dpc_ce_topk", "sweep_37"), ("dpc_ce_topk", "nv8_1028"), ("dpc_ce_topk", "nv16_8196")]
EXT16_FORMS = ["vec16x4_2056", "vec16x8_8200"]
ARMS = ["f32 logits"]


@pytest.fixture(scope="module")
def k():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return kc.K(L.load_emulator(), "cpu")


@pytest.fixture(scope="module")
def cfg(k):
    return nq.Cfg(device="cpu", simulator=k.lib, widths=WIDTHS)


@pytest.mark.parametrize("R,D,K", SHAPES)
def test_push(k, R, D, K):
    nq.case_push(k, R, D, K)


@pytest.mark.parametrize("R,D,K", SHAPES)
def test_fwd(k, R, D, K):
    nq.case_fwd(k, R, D, K)


@pytest.mark.parametrize("entry,name", EXT_FORMS)
@pytest.mark.parametrize("mode", ["f32", "bf16", "null", "bf16-null"])
def test_ext_empty_is_the_old_entry(k, entry, name, mode):
    nq.case_ext_empty(k, entry, name, mode)


@pytest.mark.parametrize("name", EXT16_FORMS)
@pytest.mark.parametrize("mode", ["bf16", "null"])
def test_ext16_empty_is_the_old_entry(k, name, mode):
    nq.case_ext_empty(k, "dpc_ce_topk_bf16", name, mode)


@pytest.mark.parametrize("R,D,K", SHAPES)
def test_ext_with_a_bank(k, R, D, K):
    nq.case_ext_bank(k, R, D, K)


@pytest.mark.parametrize("R,D,K", SHAPES)
def test_bwd(k, R, D, K):
    nq.case_bwd(k, R, D, K)


def test_refused_calls(k):
    nq.case_refused(k)


@pytest.mark.parametrize("arm", ARMS)
def test_empty_bank_is_no_bank(cfg, arm):
    nq.case_empty_bank_is_no_bank(cfg, arm)


@pytest.mark.parametrize("arm", ARMS)
def test_by_hand(cfg, arm):
    nq.case_by_hand(cfg, arm)


@pytest.mark.parametrize("arm", ARMS)
def test_eval_between_train_steps(cfg, arm):
    nq.case_eval_between(cfg, arm)


def test_nan_empties_the_bank(cfg):
    nq.case_nan_empties_the_bank(cfg)


def test_accumulation(cfg):
    nq.case_accumulation(cfg)


def test_checkpoint(cfg, tmp_path):
    nq.case_checkpoint(cfg, tmp_path)


def test_refusals(cfg):
    nq.case_refusals(cfg)


def test_two_ranks(k, tmp_path):
    nq.case_two_ranks(WIDTHS, tmp_path)


def test_entry(k, capsys):
    nq.case_entry(k.lib, WIDTHS, capsys)
