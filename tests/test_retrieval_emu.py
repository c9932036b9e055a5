"""Nearest-neighbour retrieval on the host simulator: the kernels of csrc/retrieval.hip, dpc_amd/retrieval.py, LCEngine.embed_video at
widths (8, 16, 32, 32) and `lc_main --retrieval` in-process.  The case bodies are in tests/retrieval_cases.py; the MI355X runs the
same ones (tests/test_retrieval_gpu.py)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import retrieval_cases as rc
from dpc_amd import _lib as L
from test_lc_frames_entry import ROOT, WIDTHS


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return L.load_emulator()


@pytest.mark.parametrize("nq,ng,D,K,loo", rc.EXACT_SHAPES)
def test_topk_exact_emu(emu, nq, ng, D, K, loo):
    rc.topk_exact_case(emu, "cpu", nq, ng, D, K, loo)


@pytest.mark.parametrize("nq,ng,D,K", rc.ROUNDING_SHAPES)
def test_topk_rounding_emu(emu, nq, ng, D, K):
    rc.topk_rounding_case(emu, "cpu", nq, ng, D, K)


@pytest.mark.parametrize("seed", (11, 12, 13))
def test_rounding_reference_leaves_few_queries_out(seed):
    """the condition of the list comparison, on the reference alone: at most 5 % of the queries of a case have two of their best
    K + 1 float64 similarities closer than 2e"""
    for nq, ng, D, K in rc.ROUNDING_SHAPES:
        Q, G = rc.rounding_data(nq, ng, D, seed)
        sim64 = Q.astype(np.float64) @ G.astype(np.float64).T
        best = -np.sort(-sim64, axis=1)[:, :K + 1]
        left_out = float(((-np.diff(best, axis=1)) <= 2 * rc.rounding_bound(Q, G)).any(1).mean())
        assert left_out <= rc.MAX_LEFT_OUT, (seed, nq, ng, D, K, left_out)


def test_recall_kernel_emu(emu):
    rc.recall_case(emu, "cpu")


@pytest.mark.parametrize("D", (32, 256))
def test_embed_kernels_emu(emu, D):
    rc.embed_kernels_case(emu, "cpu", D)


def test_wrappers_validate(emu):
    from dpc_amd import retrieval as R
    Q, G = torch.zeros(4, 32), torch.zeros(9, 32)
    with pytest.raises(L.DpcError):                       # CPU tensors without the simulator handle: no fallback
        R.knn_topk(None, Q, G, 2)
    with pytest.raises(L.DpcError):
        R.recall_at_k(None, torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), torch.zeros(9, dtype=torch.int64), [1], 3)
    for bad in (dict(K=65), dict(K=0), dict(n_slabs=65), dict(skip=torch.zeros(4, dtype=torch.int64))):
        with pytest.raises(ValueError):
            R.knn_topk(emu, Q, G, **dict(dict(K=2), **bad))
    with pytest.raises(ValueError):
        R.knn_topk(emu, torch.zeros(4, 48), torch.zeros(9, 48), 2)          # D no multiple of 32
    with pytest.raises(ValueError):
        R.knn_topk(emu, torch.zeros(4, 288), torch.zeros(9, 288), 2)        # D above the engine's limit
    with pytest.raises(ValueError):
        R.knn_topk(emu, torch.zeros(4, 33)[:, 1:], G, 2)                    # rows not 16-byte aligned
    with pytest.raises(ValueError):
        R.recall_at_k(emu, torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), torch.zeros(9, dtype=torch.int64), [2, 1], 3)
    with pytest.raises(ValueError):
        R.recall_at_k(emu, torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), torch.zeros(9, dtype=torch.int64), [3], 3)
    # the C ABI says the same on its own
    ws = torch.zeros(1 << 16, dtype=torch.uint8)
    sim, idx = torch.zeros(4, 2), torch.zeros(4, 2, dtype=torch.int32)
    Q48, G48 = torch.zeros(4, 48), torch.zeros(9, 48)
    fn = emu._fn("dpc_knn_topk")
    p = lambda t: t.data_ptr()    # noqa: E731
    assert fn(p(Q48), 4, 48, p(G48), 9, 48, 48, 2, None, 1, p(sim), p(idx), p(ws), ws.numel(), None) == L.ERR_UNSUPPORTED
    assert fn(p(Q), 4, 32, p(G), 9, 32, 32, 65, None, 1, p(sim), p(idx), p(ws), ws.numel(), None) == L.ERR_UNSUPPORTED
    assert fn(p(Q), 4, 32, p(G), 9, 32, 32, 2, None, 1, p(sim), p(idx), p(ws), 8, None) == L.ERR_ARG     # workspace too small
    assert emu.call("dpc_knn_ws_bytes", 70, 10, 3) == 70 * 3 * 10 * 8


def test_embed_video_running_emu(emu):
    """bn='running' against by-hand eval-mode forwards, and bit-identical rows for engines with B = 2 (2 + 2 + 1 windows) and
    B = 3 (3 + 2)"""
    r2 = rc.embed_video_case(emu, "cpu", WIDTHS, "f32", 2, "running")
    r3 = rc.embed_video_case(emu, "cpu", WIDTHS, "f32", 3, "running", check=False)
    assert np.array_equal(r2, r3)


def test_embed_video_batch_emu(emu):
    rc.embed_video_case(emu, "cpu", WIDTHS, "f32", 2, "batch")


def test_embed_video_errors_emu(emu):
    rc.embed_video_errors_case(emu, "cpu", WIDTHS)


def test_lc_main_retrieval_emu(emu, tmp_path, capsys):
    from dpc_amd import lc_main
    tmp = str(tmp_path)
    fp, lp = rc.entry_files(tmp)
    ckpt = os.path.join(tmp, "epoch3.pth.tar")
    rc.save_checkpoint(emu, "cpu", WIDTHS, "f32", 2, ckpt)
    argv = rc.entry_argv(fp, lp, ckpt, 2, "f32")
    log = os.path.join(tmp, "retrieval_log.md")
    capsys.readouterr()
    lc_main.main(argv, _simulator=emu, _widths=WIDTHS)
    rc.check_entry_outputs(ckpt + ".retrieval.npz", capsys.readouterr().out, open(log).read(), cross=False)
    before = len(open(log).read())
    lc_main.main(argv + ["--gallery_frames", fp, "--gallery_labels", lp], _simulator=emu, _widths=WIDTHS)
    rc.check_entry_outputs(ckpt + ".retrieval.npz", capsys.readouterr().out, open(log).read()[before:], cross=True)
    # random: the printed lines only
    os.remove(ckpt + ".retrieval.npz")
    before = open(log).read()
    i = argv.index("--retrieval")
    lc_main.main(argv[:i] + ["--retrieval", "random", "--retrieval_bn", "batch"] + argv[i + 2:], _simulator=emu, _widths=WIDTHS)
    out = capsys.readouterr().out
    assert "R@1: " in out and "(8 queries, 8 gallery videos, leave-one-out, bn batch)" in out and "(retrieval checkpoint epoch 0)" in out
    assert not os.path.exists(ckpt + ".retrieval.npz") and not os.path.exists("random.retrieval.npz") and open(log).read() == before


def test_lc_main_retrieval_argument_errors(emu, tmp_path):
    from dpc_amd import lc_main
    argv = rc.entry_argv("q.npy", "l.npy", "random", 2, "f32")
    run = lambda a: lc_main.main(a, _simulator=emu, _widths=WIDTHS)    # noqa: E731
    with pytest.raises(ValueError, match="--test"):
        run(argv + ["--test", "random"])
    i = argv.index("--retrieval_k")
    with pytest.raises(ValueError, match="at most 64"):
        run(argv[:i] + ["--retrieval_k", "1,65"] + argv[i + 2:])
    with pytest.raises(ValueError, match="ascending"):
        run(argv[:i] + ["--retrieval_k", "5,1"] + argv[i + 2:])
    with pytest.raises(ValueError, match="--retrieval_bn batch"):
        run(argv + ["--graph", "--retrieval_bn", "batch"])
    with pytest.raises(ValueError, match="one GPU"):
        j = argv.index("--gpu")
        run(argv[:j] + ["--gpu", "0,1"] + argv[j + 2:])
