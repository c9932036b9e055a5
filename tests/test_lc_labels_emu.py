"""CPU tier: the on-device label draw (dpc_synthetic_labels, csrc/labels.hip), the labels that stay on the device
(LCEngine.set_labels / forward(block, None) / fill_synthetic) on the host-side SIMT simulator, and `lc_main --graph` refusing to run
off the HIP device.  The GPU tier is tests/test_lc_graph_gpu.py."""
import os
import subprocess

import pytest
import torch

import lc_graph_cases as lg
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


@pytest.mark.parametrize("B,num_class", lg.LABEL_CASES)
def test_labels_match_the_definition(k, B, num_class):
    lg.case_definition(k, B, num_class)


def test_counter_and_seed(k):
    lg.case_counter_and_seed(k)


def test_bad_arguments(k):
    lg.case_bad_arguments(k)


def test_definition_is_uniform():
    """the figures the GPU tier's chi-square bound is set beside: the definition itself, in numpy"""
    for (seed, d, nc), want in (((1000, 9, 101), 93.6), ((1001, 1, 51), 44.5)):
        chi = lg.chi_square(lg.labels_np(1 << 20, nc, seed, d), nc)
        assert abs(chi - want) < 0.06 and chi < (nc - 1) + 5 * (2 * (nc - 1)) ** 0.5, chi


def test_labels_as_they_stand(emu):
    lg.case_labels_as_they_stand(emu, "cpu", torch.float32, WIDTHS)


def test_fill_synthetic_draws_the_labels_of_the_batch(emu):
    lg.case_fill_synthetic_labels(emu, "cpu", torch.float32, WIDTHS)


def test_lc_main_graph_refuses_the_simulator(emu, tmp_path, capsys):
    """--graph off the HIP device: the capture's DpcError, before any step (no log line, no probe file); the parser knows the flag"""
    from dpc_amd import lc_main
    assert lc_main.build_parser().parse_args(["--graph"]).graph is True and lc_main.build_parser().parse_args([]).graph is False
    pr = str(tmp_path / "probe")
    os.makedirs(pr)
    argv = ["--net", "resnet18", "--img_dim", "64", "--batch_size", "1", "--gpu", "0", "--synthetic", "1", "--print_freq", "1",
            "--dtype", "f32", "--num_seq", "2", "--seq_len", "2", "--epochs", "1", "--graph"]
    with pytest.raises(L.DpcError, match="hipGraph capture needs the HIP device"):
        lc_main.main(argv, _simulator=emu, _widths=WIDTHS, _probe=pr)
    assert "Epoch:" not in capsys.readouterr().out and os.listdir(pr) == []
