"""CPU tier: the on-device synthetic input (dpc_synthetic_input, csrc/synthetic.hip; DPCEngine.fill_synthetic) on the host-side SIMT
simulator, and `main --graph` refusing to run off the HIP device.  The GPU tier is tests/test_entry_graph_gpu.py."""
import os
import subprocess

import pytest
import torch

import synthetic_cases as sc
from dpc_amd import _lib as L
from kcases import K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (8, 16, 32, 32)


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return L.load_emulator()


@pytest.fixture
def k(emu):
    return K(emu, "cpu")


# W % 4 == 0 (every size the build runs: a thread's two cells are one Philox block per row), W % 4 == 2 (rows start half-way into a
# block), and an odd number of cells per row (the last thread of a row has one cell)
SHAPES = [(2, 3, 8, 16), (2, 2, 6, 10), (1, 2, 4, 6)]


@pytest.mark.parametrize("shape", SHAPES)
def test_normals_match_the_definition(k, shape):
    sc.case_normals(k, shape)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_s2d_operand_is_the_pack_of_the_block(k, shape, dtype):
    sc.case_s2d(k, shape, dtype)


def test_counter_and_seed(k):
    sc.case_counter(k, (2, 2, 8, 8))


def test_bad_arguments(k):
    ctr = torch.zeros(1, dtype=torch.int32)
    b = torch.empty(1, 3, 2, 8, 8)
    with pytest.raises(L.DpcError):   # nothing to write
        k.call("dpc_synthetic_input", None, None, L.F32, 1, 2, 8, 8, 1, ctr)
    with pytest.raises(L.DpcError):   # no counter
        k.call("dpc_synthetic_input", b, None, L.F32, 1, 2, 8, 8, 1, None)
    with pytest.raises(L.DpcError):   # odd image: no space-to-depth cells
        k.call("dpc_synthetic_input", b, None, L.F32, 1, 2, 8, 7, 1, ctr)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fill_synthetic_then_train_step_equals_train_step_on_the_block(emu, dtype):
    """fill_synthetic(s, block) + train_step(None) == train_step(block): the operand the generator writes is the one the f32 path packs"""
    from dpc_amd.engine import DPCEngine
    from dpc_amd.model import DPC_RNN
    init = {k_: v.detach() for k_, v in DPC_RNN(64, 4, 5, 1, "resnet18", widths=WIDTHS, seed=0).named_parameters()}
    a, b = (DPCEngine("resnet18", 64, 4, 5, 1, 1, "cpu", dtype, WIDTHS, lib=emu) for _ in range(2))
    a.load_params(init)
    b.load_params(init)
    block = torch.empty(1, 4, 3, 5, 64, 64)
    for _ in range(2):
        a.fill_synthetic(1000, block)
        ra = a.train_step(None).clone()
        rb = b.train_step(block.clone()).clone()
        assert torch.equal(ra, rb)
    assert int(a.dev_input.item()) == 2 and int(b.dev_input.item()) == 0   # one counter step per draw
    assert torch.equal(a.flat_p, b.flat_p) and torch.equal(a.flat_m, b.flat_m)
    assert abs(block.mean().item()) < 0.05 and abs(block.std().item() - 1.0) < 0.05
    # the operand alone: the same draw as with the block, and a following forward(None) sees it
    x = a.x_s2d.clone()
    a.dev_input.sub_(1)
    a.fill_synthetic(1000)
    assert torch.equal(a.x_s2d, x)
    with pytest.raises(ValueError):
        a.fill_synthetic(1000, torch.empty(1, 4, 3, 5, 64, 32))


def test_main_graph_refuses_the_simulator(emu, tmp_path, capsys):
    """--graph off the HIP device: the capture's DpcError, before any step (no log line, no probe file)"""
    from dpc_amd import main as dpc_main
    pr = str(tmp_path / "probe")
    os.makedirs(pr)
    argv = ["--net", "resnet18", "--img_dim", "64", "--batch_size", "1", "--gpu", "0", "--synthetic", "1", "--print_freq", "1",
            "--dtype", "f32", "--num_seq", "4", "--pred_step", "1", "--epochs", "1", "--graph"]
    with pytest.raises(L.DpcError, match="hipGraph capture needs the HIP device"):
        dpc_main.main(argv, _simulator=emu, _widths=WIDTHS, _probe=pr)
    assert "Epoch:" not in capsys.readouterr().out and os.listdir(pr) == []
