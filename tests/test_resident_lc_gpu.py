"""MI355X tier of `python -m dpc_amd.lc_main --frames ... --labels ... --resident`: the cases of tests/resident_lc_cases.py on the
device (dpc_draw_recipe_ex's unfused double arithmetic, its f64 square root and Philox words as gfx950 executes them, the label
gather), load_resident with labels against load_recipe + set_labels through two train steps and one eval step, the captured train
and eval steps with their resident refills across epoch boundaries, and the entry with and without --graph.  The simulator tier is
tests/test_resident_lc_emu.py."""
import pytest
import torch

import resident_cases as rc
import resident_lc_cases as lc
from dpc_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    return L.load_hip()


@pytest.mark.parametrize("mode,shape", lc.LC_CASES, ids=lc.LC_IDS)
def test_draw_kernel_equals_the_host_recipe(lib, mode, shape):
    lc.draw_injected_case(lib, DEV, mode, *shape)


@pytest.mark.parametrize("name", [s[0] for s in rc.DRAW_SHAPES])
def test_new_entry_with_the_additions_off_is_the_old_one(lib, name):
    lc.additions_off_case(lib, DEV, name)


def test_old_entry_ignores_the_flags(lib):
    lc.old_entry_ignores_flags_case(lib, DEV)


def test_draw_kernel_philox(lib):
    lc.philox_case(lib, DEV)


def test_draw_kernel_distribution(lib):
    lc.dist_kernel_case(lib, DEV)


def test_draw_kernel_rejects(lib):
    lc.draw_rejects_case(lib, DEV)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_load_resident_with_labels_equals_load_recipe(lib, dtype, B):
    """B = 2: two train steps and one eval step; B = 3 (one batch per epoch of the four usable videos): operand and target only"""
    lc.engine_case(lib, DEV, dtype, B=B, train=B == 2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_captured_resident_steps_span_epoch_boundaries(dtype):
    lc.graph_case(DEV, dtype)


def test_entry_resident_equals_the_documented_loop(lib, tmp_path, capsys):
    lc.entry_by_hand_case(lib, DEV, str(tmp_path), capsys, "bf16", None, 2, "all")


@pytest.mark.parametrize("train_what", ["all", "head"])
def test_entry_resident_graph_equals_eager(tmp_path, capfd, train_what):
    lc.entry_graph_case(str(tmp_path), capfd, train_what)


def test_test_and_retrieval_resident_equal_the_uploading_runs(tmp_path, capsys):
    lc.protocol_case(str(tmp_path), capsys)


def test_test_resident_under_graph_equals_the_uploading_run(tmp_path, capsys):
    lc.protocol_case(str(tmp_path), capsys, graph=True)
