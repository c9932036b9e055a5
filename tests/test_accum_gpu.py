"""GPU tier: gradient accumulation on the MI355X -- dpc_grad_accumulate, the accumulating engine step (resnet18 at the reference's
widths, 64 px, B = 2, num_seq 4, pred_step 1; f32 and bf16), its checkpoint, the LC head groups and the captured micro-batch step,
without an exchange, with counted one- and two-bucket exchanges and with both over RCCL with one rank.  The cases are those of
the CPU tier (tests/accum_cases.py)."""
import os
import subprocess
import sys

import pytest
import torch

import accum_cases as acc
import kcases as kc
from dpc_amd import _lib as L
from dpc_amd.plan import LAYER_WIDTH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def k():
    return kc.K(L.load_hip(), DEV)


@pytest.fixture(scope="module")
def cfg():
    return acc.Cfg(device=DEV, simulator=None, widths=LAYER_WIDTH)


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


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_off_is_the_engine_as_it_was(cfg, dtype):
    acc.case_off_is_the_engine_as_it_was(cfg, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_against_a_by_hand_twin(cfg, dtype):
    acc.case_against_a_by_hand_twin(cfg, dtype)


def test_against_f64_adam(cfg):
    acc.case_against_f64_adam(cfg)


def test_dropped_cycle(cfg):
    acc.case_dropped_cycle(cfg)


def test_lc_head_groups(cfg):
    acc.case_lc_head_groups(cfg, num_class=101)


def test_checkpoint(cfg, tmp_path):
    acc.case_checkpoint(cfg, tmp_path)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [2, 3])
def test_captured_step(cfg, N, dtype):
    acc.case_captured_step(cfg, N, dtype)


@pytest.mark.parametrize("exchange,N,dtype", [("one", 2, torch.bfloat16), ("two", 3, torch.float32)])
def test_captured_step_counted_exchange(cfg, exchange, N, dtype):
    acc.case_captured_step(cfg, N, dtype, exchange=exchange)


_RANK_SCRIPT = r"""
import os, sys, torch
import torch.distributed as dist
sys.path.insert(0, {root!r})
sys.path.insert(0, os.path.join({root!r}, "tests"))
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(rank)
dev = torch.device("cuda", rank)
dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
import accum_cases as acc
from dpc_amd.parallel import make_allreduce
from dpc_amd.plan import LAYER_WIDTH
cfg = acc.Cfg(device=str(dev), simulator=None, widths=LAYER_WIDTH)
for exchange, N, dtype in (("one", 3, torch.bfloat16), ("two", 2, torch.float32)):
    acc.case_captured_step(cfg, N, dtype, exchange=exchange, inner=make_allreduce(dist, world, force=True))
torch.cuda.synchronize()
open(os.path.join({out!r}, "done"), "w").write("ok")
dist.barrier()
dist.destroy_process_group()
"""


def test_captured_step_rccl_single_rank(tmp_path, clean_launcher):
    """the captured micro-batch step with the one-bucket and the two-bucket exchange over RCCL, world_size 1"""
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT.format(root=ROOT, out=str(tmp_path)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    argv = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
            "--master-addr", "127.0.0.1", "--master-port", str(29600 + os.getpid() % 200), str(script)]
    if clean_launcher is not None:
        rc, _, err = clean_launcher.run(argv, env, 600)
    else:   # a single test run by hand without "-m gpu"
        r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=600)
        rc, err = r.returncode, r.stderr
    assert rc == 0 and (tmp_path / "done").exists(), err[-4000:]
