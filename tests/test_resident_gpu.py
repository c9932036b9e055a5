"""MI355X tier of `python -m dpc_amd.main --frames ... --resident`: the cases of tests/resident_cases.py on the device (the f64 square
root, the unfused double arithmetic and the Philox words of csrc/recipe_draw.hip as gfx950 executes them), a store of more than
2^31 bytes, load_resident against load_recipe through two train steps, the captured step across an epoch boundary, and the entry
with and without --graph.  The simulator tier is tests/test_resident_emu.py."""
import pytest
import torch

import resident_cases as rc
from dpc_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    return L.load_hip()


@pytest.mark.parametrize("name", [s[0] for s in rc.DRAW_SHAPES])
def test_draw_kernel_equals_the_host_recipe(lib, name):
    rc.draw_injected_case(lib, DEV, name)


def test_draw_kernel_philox(lib):
    rc.philox_case(lib, DEV)


def test_draw_kernel_distribution(lib):
    rc.dist_kernel_case(lib, DEV)


def test_draw_kernel_rejects(lib):
    rc.draw_rejects_case(lib, DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("jitter", [True, False])
def test_store_gather_equals_hand_cut_spans(lib, jitter, dtype):
    rc.gather_case(lib, DEV, jitter, dtype)


def test_store_larger_than_2_31_bytes(lib):
    rc.big_store_case(lib, DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_load_resident_equals_load_recipe(lib, dtype):
    rc.engine_case(lib, DEV, dtype, steps=2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_captured_resident_step_spans_an_epoch_boundary(dtype):
    rc.graph_case(DEV, dtype)


def test_entry_resident_graph_equals_eager(tmp_path, capsys):
    rc.entry_case(str(tmp_path), capsys, graph=True)
