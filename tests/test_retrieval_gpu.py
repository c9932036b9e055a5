"""Nearest-neighbour retrieval on the MI355X: the cases of tests/retrieval_cases.py on libdpc_hip.so -- the kernels of
csrc/retrieval.hip, LCEngine.embed_video at full widths (resnet18, 64 px, B = 2; f32 and one bf16 case) and
`python -m dpc_amd.lc_main --retrieval` as a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import retrieval_cases as rc
from dpc_amd import _lib as L
from test_lc_frames_entry import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("nq,ng,D,K,loo", rc.EXACT_SHAPES)
def test_topk_exact_gpu(nq, ng, D, K, loo):
    rc.topk_exact_case(L.load_hip(), DEV, nq, ng, D, K, loo)


@pytest.mark.parametrize("nq,ng,D,K", rc.ROUNDING_SHAPES)
def test_topk_rounding_gpu(nq, ng, D, K):
    rc.topk_rounding_case(L.load_hip(), DEV, nq, ng, D, K)


def test_recall_kernel_gpu():
    rc.recall_case(L.load_hip(), DEV)


@pytest.mark.parametrize("D", (32, 256))
def test_embed_kernels_gpu(D):
    rc.embed_kernels_case(L.load_hip(), DEV, D)


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_embed_video_running_gpu(dtype):
    rc.embed_video_case(L.load_hip(), DEV, None, dtype, 2, "running")


def test_embed_video_batch_gpu():
    rc.embed_video_case(L.load_hip(), DEV, None, "f32", 2, "batch")


def test_embed_video_graph_gpu():
    """graph=True: the rows of replayed eval-mode steps are the bits of the eager rows"""
    eager = rc.embed_video_case(L.load_hip(), DEV, None, "f32", 2, "running", check=False)
    replayed = rc.embed_video_case(L.load_hip(), DEV, None, "f32", 2, "running", graph=True)
    assert np.array_equal(eager, replayed)


def test_embed_video_errors_gpu():
    rc.embed_video_errors_case(L.load_hip(), DEV, None)


def test_lc_main_retrieval_gpu(tmp_path, clean_launcher):
    """the command line once, as a child process: leave-one-out, bn running"""
    tmp = str(tmp_path)
    fp, lp = rc.entry_files(tmp)
    ckpt = os.path.join(tmp, "epoch3.pth.tar")
    rc.save_checkpoint(L.load_hip(), DEV, None, "f32", 2, ckpt)
    argv = rc.entry_argv(fp, lp, ckpt, 2, "f32")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-c", "import os, runpy, sys; os.chdir(sys.argv[1]); sys.argv = sys.argv[2:]; runpy.run_module(sys.argv[0], run_name='__main__')",
           ROOT, "dpc_amd.lc_main"] + argv
    if clean_launcher is not None:
        code, out, err = clean_launcher.run(cmd, env, 600)
    else:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        code, out, err = r.returncode, r.stdout, r.stderr
    assert code == 0, out[-3000:] + "\n" + err[-3000:]
    rc.check_entry_outputs(ckpt + ".retrieval.npz", out, open(os.path.join(tmp, "retrieval_log.md")).read(), cross=False)
