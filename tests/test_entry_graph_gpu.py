"""GPU tier of `python -m dpc_amd.main --graph`: the on-device synthetic input (dpc_synthetic_input / DPCEngine.fill_synthetic), the
captured train step on the stem's operand, the captured evaluation step, and the entry itself against eager runs, bit for bit.
The CPU tier of the same kernel is tests/test_synthetic_input_emu.py."""
import math
import os
import re

import numpy as np
import pytest
import torch

import synthetic_cases as sc
from dpc_amd import _lib as L
from dpc_amd.engine import DPCEngine
from kcases import K
from oracle import dpc_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAPH_LINE = re.compile(r"Graph replay: (\d+) steps, ([0-9.]+) ms/step, ([0-9.]+) clips/s")


@pytest.fixture(scope="module")
def k():
    return K(L.load_hip(), DEV)


# ---- (1) the kernel on the device
@pytest.mark.parametrize("shape", [(4, 5, 32, 32), (2, 3, 18, 14), (1, 2, 4, 6)])
def test_normals_match_the_definition(k, shape):
    sc.case_normals(k, shape)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(4, 5, 64, 64), (2, 3, 18, 14)])
def test_s2d_operand_is_the_pack_of_the_block(k, shape, dtype):
    sc.case_s2d(k, shape, dtype)


def test_counter_and_seed(k):
    sc.case_counter(k, (4, 5, 32, 32))


def test_statistics(k):
    """18.9 M values: mean, variance and the Kolmogorov-Smirnov distance to N(0,1), each within 5 standard errors"""
    ctr = torch.tensor([9], dtype=torch.int32, device=DEV)
    b, _ = sc.draw(k, (64, 6, 128, 128), 1000, ctr, s2d=False)
    x = b.reshape(-1).double()
    n = x.numel()
    assert n >= 16 * 2 ** 20 and bool(torch.isfinite(x).all())
    mean, var = x.mean().item(), x.var().item()
    assert abs(mean) < 5 / math.sqrt(n), mean
    assert abs(var - 1) < 5 * math.sqrt(2 / n), var
    xs, _ = torch.sort(x)
    cdf = 0.5 * (1 + torch.erf(xs / math.sqrt(2)))
    i = torch.arange(1, n + 1, device=DEV, dtype=torch.float64)
    ks = torch.maximum(i / n - cdf, cdf - (i - 1) / n).max().item()
    assert ks < 5 / math.sqrt(n), ks   # sqrt(n) D has mean 0.87, sd 0.26 under the null
    del x, xs, cdf, i


# ---- (2) / (3) the engine
def _eng(dtype, B=4):
    eng = DPCEngine("resnet18", 64, 8, 5, 3, B, DEV, dtype, seed=233)
    eng.load_params(O.init_params_reference_style("resnet18", seed=0))
    return eng


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_captured_synthetic_step_equals_eager(dtype):
    """2 eager steps + 4 replays of capture_train_step(None, refill=fill_synthetic) == 6 eager (fill + train_step(None)) steps"""
    a, b = _eng(dtype), _eng(dtype)
    for _ in range(6):
        a.fill_synthetic(1000)
        ra = a.train_step(None).clone()
    for _ in range(2):
        b.fill_synthetic(1000)
        b.train_step(None)
    refill = lambda: b.fill_synthetic(1000)  # noqa: E731
    replay = b.capture_train_step(None, warmup=0, refill=refill)
    assert b.capture_train_step(None, warmup=0, refill=refill) is replay   # keyed on the operand
    for _ in range(4):
        rb = replay().clone()
    torch.cuda.synchronize()
    assert a.step_count == b.step_count == 6 and int(b.dev_input.item()) == 6 and int(b.dev_step.item()) == 6
    assert torch.equal(a.flat_p, b.flat_p) and torch.equal(a.flat_m, b.flat_m) and torch.equal(ra, rb)


def _eval(eng):
    eng.fill_synthetic(1000)
    eng.forward(None, train=False, materialise=False)
    return eng.loss_topk(with_grad=False).clone()


def test_captured_eval_step_follows_the_training():
    """capture_eval_step replays interleaved with replayed (and eager) train steps == eager evaluation on a twin engine at every
    point: the replay repacks the weights it evaluates"""
    dtype = torch.bfloat16
    a, b = _eng(dtype), _eng(dtype)
    for e in (a, b):
        for _ in range(2):
            e.fill_synthetic(1000)
            e.train_step(None)
        _eval(e)
    ev = b.capture_eval_step(refill=lambda: b.fill_synthetic(1000))
    tr = b.capture_train_step(None, warmup=0, refill=lambda: b.fill_synthetic(1000))
    assert b.capture_eval_step(refill=ev.refill) is ev
    seen = []
    for plan in ("te", "tte", "ee", "Te", "e"):   # t: replayed train step (T: eager), e: evaluation
        for c in plan:
            if c == "e":
                ra, rb = _eval(a), ev().clone()
                torch.cuda.synchronize()
                assert torch.equal(ra, rb), (plan, ra, rb)
                seen.append(ra[0].item())
                continue
            a.fill_synthetic(1000)
            a.train_step(None)
            if c == "t":
                tr()
            else:
                b.fill_synthetic(1000)
                b.train_step(None)
    torch.cuda.synchronize()
    assert torch.equal(a.flat_p, b.flat_p) and a.step_count == b.step_count == 6
    assert len(set(seen)) == len(seen)   # every evaluation saw new weights and a new batch


# ---- (4) - (6) the entry
def _args(extra):
    return ["--net", "resnet18", "--img_dim", "64", "--gpu", "0", "--dtype", "bf16", "--epochs", "2"] + extra


def test_entry_graph_synthetic_equals_the_documented_eager_loop(tmp_path, capsys):
    from dpc_amd import main as dpc_main
    from dpc_amd.model import DPC_RNN
    pr = str(tmp_path / "probe")
    os.makedirs(pr)
    dpc_main.main(_args(["--batch_size", "2", "--synthetic", "4", "--graph"]), _probe=pr)
    out = capsys.readouterr().out
    got = torch.load(os.path.join(pr, "rank0.pt"))
    assert got["step"] == 8
    lines = GRAPH_LINE.findall(out)
    assert [int(n) for n, _, _ in lines] == [2, 4], out    # epoch 0: steps 0-1 are the eager warm-up
    assert all(float(ms) > 0 and abs(float(c) - 2e3 / float(ms)) < 0.01 * float(c) + 0.1 for _, ms, c in lines)
    assert out.count("Epoch: [0][0/4]") == 1 and out.count("Epoch: [1][0/4]") == 1 and "[1/2] Loss" in out
    # by hand: each train step = fill_synthetic(1000) + train_step(None); each validation step = fill + forward + loss
    eng = DPCEngine("resnet18", 64, 8, 5, 3, 2, DEV, torch.bfloat16, seed=233, reserve_cus=0)
    eng.load_params({k_: v.detach() for k_, v in DPC_RNN(64, 8, 5, 3, "resnet18", seed=0).named_parameters()})
    for _ in range(2):
        for _ in range(4):
            eng.fill_synthetic(1000)
            eng.train_step(None)
        for _ in range(4):
            _eval(eng)
    torch.cuda.synchronize()
    assert torch.equal(got["flat_p"], eng.flat_p.cpu()) and torch.equal(got["flat_m"], eng.flat_m.cpu())


def _clips(tmp_path, golden_dir, n):
    """clips built from tests/golden/aug.npz the way tests/test_data_pipeline.py::_frames_entry_case builds them"""
    g = np.load(os.path.join(golden_dir, "aug.npz"))
    base = g["frames"]
    rng = np.random.default_rng(3)
    clips = np.stack([np.roll(base, k_, axis=0) if k_ % 2 == 0 else base[:, ::-1][:, :, ::-1].copy() for k_ in range(n)])
    clips = (clips.astype(np.int16) + rng.integers(-3, 4, clips.shape)).clip(0, 255).astype(np.uint8)
    path = os.path.join(str(tmp_path), "clips.npy")
    np.save(path, clips)
    return path


def _frames_graph_case(tmp_path, golden_dir, capfd, gpus, B):
    from dpc_amd import main as dpc_main
    world = len(gpus.split(","))
    path = _clips(tmp_path, golden_dir, B * 4)
    argv = _args(["--batch_size", str(B), "--gpu", gpus, "--print_freq", "1", "--num_seq", "4", "--seq_len", "3", "--pred_step", "1",
                  "--ds", "1", "--dataset", "ucf101", "--crop", "56", "--frames", path])
    runs = {}
    for mode in ("eager", "graph"):
        pr = str(tmp_path / mode)
        os.makedirs(pr)
        dpc_main.main(argv + (["--graph"] if mode == "graph" else []), _probe=pr)
        out = capfd.readouterr().out   # (fd level: rank 0 of a two-rank run is a child process)
        runs[mode] = ([torch.load(os.path.join(pr, f"rank{r}.pt")) for r in range(world)],
                      [re.sub(r"T:[0-9.]+", "", ln) for ln in out.splitlines() if "Loss" in ln])
    (pe, le), (pg, lg) = runs["eager"], runs["graph"]
    assert all(r["step"] == 8 for r in pe + pg)   # B * 4 clips: 4 batches of B / world clips per rank and epoch
    for a, b in zip(pe, pg):
        assert torch.equal(a["flat_p"], b["flat_p"]) and torch.equal(a["flat_m"], b["flat_m"])
    assert le == lg and len(le) == 2 * 5   # every train step is logged (print_freq 1) + one validation line per epoch


def test_entry_graph_frames_equals_eager(tmp_path, golden_dir, capfd):
    _frames_graph_case(tmp_path, golden_dir, capfd, "0", 2)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_entry_graph_frames_two_ranks(tmp_path, golden_dir, capfd):
    _frames_graph_case(tmp_path, golden_dir, capfd, "0,1", 4)
