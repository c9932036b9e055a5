"""GPU tier of `python -m dpc_amd.lc_main --graph`: the on-device label draw (dpc_synthetic_labels / LCEngine.fill_synthetic), the
classifier's captured train and evaluation steps (one group, parameter groups, a frozen extractor, the RCCL cut), the entry and the
video-level test protocol on replayed hipGraphs -- each against an eager twin, bit for bit.  The CPU tier is
tests/test_lc_labels_emu.py.  Shapes: the smallest the LC entry tests run (tests/test_lc_frames_entry.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import lc_graph_cases as lg
import test_lc_frames_entry as fe
from dpc_amd import _lib as L
from kcases import K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPH_LINE = re.compile(r"Graph replay: (\d+) steps, ([0-9.]+) ms/step, ([0-9.]+) clips/s")
EXTRACTOR = ("backbone.", "agg.")
SEED = 1000


@pytest.fixture(scope="module")
def k():
    return K(L.load_hip(), DEV)


# ---- (1) the kernel on the device
@pytest.mark.parametrize("B,num_class", lg.LABEL_CASES)
def test_labels_match_the_definition(k, B, num_class):
    lg.case_definition(k, B, num_class)


def test_counter_seed_and_bad_arguments(k):
    lg.case_counter_and_seed(k)
    lg.case_bad_arguments(k)


@pytest.mark.parametrize("seed,d,num_class", [(1000, 9, 101), (1001, 1, 51)])
def test_labels_are_uniform(k, seed, d, num_class):
    lg.case_uniform(k, seed, d, num_class)


def test_labels_as_they_stand_and_fill_synthetic():
    lg.case_labels_as_they_stand(None, DEV, torch.bfloat16, None)
    lg.case_fill_synthetic_labels(None, DEV, torch.bfloat16, None)


# ---- (2) - (4) the engine
def _eng(dtype, B=2):
    return lg.lc_engine(None, DEV, dtype, None, B, fe.SIZE, fe.N, fe.SL, fe.NUM_CLASS)


def _groups(eng, mode, mult=1.0, lr=1e-3):
    """the parameter groups as dpc_amd.lc_main builds them for --train_what ft_backbone / head, scaled by the schedule"""
    extractor = [k_ for k_ in eng.offsets if k_.startswith(EXTRACTOR)]
    if mode == "ft_backbone":
        groups = [(extractor, lr / 10), ([k_ for k_ in eng.offsets if k_ not in extractor], lr)]
    else:
        groups = [([k_ for k_ in eng.offsets if k_.startswith(("final_bn.", "final_fc."))], lr)]
    lrs = [g_lr * mult for _, g_lr in groups]
    eng.set_param_groups([{"params": ks, "lr": g_lr, "weight_decay": 1e-3} for (ks, _), g_lr in zip(groups, lrs)])
    eng.lr = lrs[-1]


def _train(eng):
    eng.fill_synthetic(SEED)
    return eng.train_step(None, None).clone()


def _eval(eng):
    eng.fill_synthetic(SEED)
    eng.forward(None, None, train=False)
    return eng.result.clone()


def _assert_same_state(a, b, ra=None, rb=None):
    torch.cuda.synchronize()
    assert torch.equal(a.flat_p, b.flat_p) and torch.equal(a.flat_m, b.flat_m) and torch.equal(a.flat_v, b.flat_v)
    assert list(a.BUF) == list(b.BUF)
    for name in a.BUF:
        assert torch.equal(a.BUF[name], b.BUF[name]), name
    assert a.step_count == b.step_count == int(b.dev_step.item()) == int(a.dev_step.item())
    assert int(a.dev_input.item()) == int(b.dev_input.item()) and int(a.dev_draw.item()) == int(b.dev_draw.item())
    assert torch.equal(a.target, b.target)
    if ra is not None:
        assert torch.equal(ra, rb) and torch.isfinite(ra).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_captured_train_step_equals_eager(dtype):
    """2 eager steps + 4 replays of capture_train_step(None, refill=fill_synthetic) == 6 eager (fill + train_step(None, None)) steps"""
    a, b = _eng(dtype), _eng(dtype)
    for _ in range(6):
        ra = _train(a)
    for _ in range(2):
        _train(b)
    refill = lambda: b.fill_synthetic(SEED)  # noqa: E731
    replay = b.capture_train_step(None, warmup=0, refill=refill)
    assert b.capture_train_step(None, warmup=0, refill=refill) is replay and len(b._capture_graphs) == 1
    assert len(replay.graphs) == 1 and replay.kernels[0] > 50
    for _ in range(4):
        rb = replay().clone()
    _assert_same_state(a, b, ra, rb)
    assert a.step_count == 6 and int(b.dev_input.item()) == 6
    assert int(b.BUF["backbone.bn1.num_batches_tracked"].item()) == 6 and int(b.BUF["final_bn.num_batches_tracked"].item()) == 6


@pytest.mark.parametrize("mode", ["ft_backbone", "head"])
def test_captured_train_step_with_parameter_groups(mode):
    dtype = torch.bfloat16
    a, b = _eng(dtype), _eng(dtype)
    for e in (a, b):
        _groups(e, mode)
    p0, buf0 = b.flat_p.clone(), {n: t.clone() for n, t in b.BUF.items()}
    assert b.grad_wanted() == ((True, True) if mode == "ft_backbone" else (False, False))
    for _ in range(4):
        ra = _train(a)
    for _ in range(2):
        _train(b)
    refill = lambda: b.fill_synthetic(SEED)  # noqa: E731
    replay = b.capture_train_step(None, warmup=0, refill=refill)
    assert len(replay.graphs) == 1
    for _ in range(2):
        rb = replay().clone()
    _assert_same_state(a, b, ra, rb)
    frozen = torch.zeros(b.numel, dtype=torch.bool, device=DEV)
    for name, (o, n) in b.offsets.items():
        if name.startswith(EXTRACTOR):
            frozen[o:o + n] = True
    bits = lambda t: t.view(torch.int32)   # noqa: E731
    if mode == "head":   # the extractor's parameters are bit-untouched, its BatchNorm layers still ran on batch statistics
        assert torch.equal(bits(b.flat_p)[frozen], bits(p0)[frozen]) and not b.flat_m[frozen].any()
        assert not torch.equal(b.BUF["backbone.bn1.running_mean"], buf0["backbone.bn1.running_mean"])
        assert not torch.equal(b.BUF["backbone.layer4.1.bn2.running_var"], buf0["backbone.layer4.1.bn2.running_var"])
        assert int(b.BUF["backbone.bn1.num_batches_tracked"].item()) == 4
    else:
        assert not torch.equal(bits(b.flat_p)[frozen], bits(p0)[frozen])
    assert not torch.equal(bits(b.flat_p)[~frozen], bits(p0)[~frozen])
    # the schedule changes a group's lr: the table is among the baked values -- the old replay refuses, a new capture follows eager
    for e in (a, b):
        _groups(e, mode, mult=0.1)
    with pytest.raises(RuntimeError, match="capture_train_step"):
        replay()
    replay2 = b.capture_train_step(None, warmup=0, refill=refill)
    assert replay2 is not replay and len(b._capture_graphs) == 2
    for _ in range(2):
        ra, rb = _train(a), replay2().clone()
    _assert_same_state(a, b, ra, rb)
    assert a.step_count == 6
    _groups(b, mode)
    assert b.capture_train_step(None, warmup=0, refill=refill) is replay   # the first capture is still there for its own table


def test_captured_eval_step_follows_the_training():
    """capture_eval_step replays interleaved with replayed (and eager) train steps == eager evaluation on a twin engine at every
    point: the replay repacks the weights and reads the running buffers of now"""
    dtype = torch.bfloat16
    a, b = _eng(dtype), _eng(dtype)
    for e in (a, b):
        for _ in range(2):
            _train(e)
        _eval(e)
    ev = b.capture_eval_step(refill=lambda: b.fill_synthetic(SEED))
    tr = b.capture_train_step(None, warmup=0, refill=lambda: b.fill_synthetic(SEED))
    assert b.capture_eval_step(refill=ev.refill) is ev and len(ev.graphs) == 1
    seen = []
    for plan in ("te", "tte", "ee", "Te", "e"):   # t: replayed train step (T: eager), e: evaluation
        for c in plan:
            if c == "e":
                ra, rb = _eval(a), ev().clone()
                torch.cuda.synchronize()
                assert torch.equal(ra, rb) and torch.equal(a.logits, b.logits), (plan, ra, rb)
                seen.append(ra[0].item())
                continue
            _train(a)
            if c == "t":
                tr()
            else:
                _train(b)
    _assert_same_state(a, b)
    assert a.step_count == 6
    assert len(set(seen)) == len(seen)   # every evaluation saw new weights and a new batch


# ---- (5) RCCL with one rank
_RANK_SCRIPT = r"""
import os, sys, torch
import torch.distributed as dist
sys.path.insert(0, {root!r})
sys.path.insert(0, os.path.join({root!r}, "tests"))
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(rank)
dev = torch.device("cuda", rank)
dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
import lc_graph_cases as lg
from dpc_amd.parallel import make_allreduce

def engine(mode):
    e = lg.lc_engine(None, dev, torch.bfloat16, None, 2, 64, 2, 2, 101, seed=666 + rank)
    if mode == "head":
        e.set_param_groups([{{"params": [k for k in e.offsets if k.startswith(("final_bn.", "final_fc."))], "lr": 1e-3, "weight_decay": 1e-3}}])
    return e

def step(e, a):
    e.fill_synthetic(1000 + rank)
    return e.train_step(None, None, allreduce=a).clone()

# the same 4 train steps launched three ways must leave bit-identical state:
#   A eager + two-bucket exchange | C hipGraphs cut at the exchange points | D one hipGraph, no exchange
out = {{}}
for mode in ("all", "head"):
    for tag in ("A", "C", "D"):
        e = engine(mode)
        a = make_allreduce(dist, world, force=True) if tag != "D" else None
        ng, kernels = 0, []
        if tag == "A":
            for _ in range(4):
                r_ = step(e, a)
        else:
            for _ in range(2):
                step(e, a)
            rp = e.capture_train_step(None, allreduce=a, warmup=0, refill=lambda: e.fill_synthetic(1000 + rank))
            for _ in range(2):
                r_ = rp().clone()
            ng, kernels = len(rp.graphs), list(rp.kernels)
        torch.cuda.synchronize()
        out[mode, tag] = dict(params=e.flat_p.cpu(), m=e.flat_m.cpu(), res=r_.cpu(), ngraphs=ng, kernels=kernels, steps=e.step_count,
                              bn=e.BUF["backbone.bn1.running_mean"].cpu())
torch.save(out, os.path.join({out!r}, f"rank{{rank}}.pt"))
dist.barrier()
dist.destroy_process_group()
"""


def test_rccl_single_rank_exchange_and_graph_cut(tmp_path, clean_launcher):
    """the RCCL path with world_size 1: eager two-bucket exchange == replay cut at the exchange points == one graph without
    exchange, bit for bit; three graphs for the full backward, two for the frozen extractor, none of them empty"""
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT.format(root=ROOT, out=str(tmp_path)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    argv = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
            "--master-addr", "127.0.0.1", "--master-port", str(29400 + os.getpid() % 200), str(script)]
    if clean_launcher is not None:
        rc, _, err = clean_launcher.run(argv, env, 600)
    else:   # a single test run by hand without "-m gpu"
        r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=600)
        rc, err = r.returncode, r.stderr
    assert rc == 0, err[-4000:]
    m = torch.load(tmp_path / "rank0.pt")
    for mode, ngraphs in (("all", 3), ("head", 2)):
        A, C_, D = (m[mode, t] for t in "ACD")
        assert C_["ngraphs"] == ngraphs and len(C_["kernels"]) == ngraphs and all(n > 0 for n in C_["kernels"]), (mode, C_["kernels"])
        assert D["ngraphs"] == 1 and A["steps"] == C_["steps"] == D["steps"] == 4
        for other in (C_, D):
            for key in ("params", "m", "res", "bn"):
                assert torch.equal(A[key], other[key]), (mode, key)
        assert torch.isfinite(A["res"]).all() and A["m"].abs().sum() > 0
    assert m["head", "C"]["kernels"][1] == 2   # graph B of the truncated replay: the step counter and the grouped Adam


# ---- (6) - (8) the entry
def _args(extra):
    return ["--net", "resnet18", "--img_dim", str(fe.SIZE), "--gpu", "0", "--dtype", "bf16", "--num_seq", str(fe.N), "--seq_len", str(fe.SL),
            "--ds", str(fe.DS), "--dataset", "ucf101", "--print_freq", "1"] + extra


def test_entry_graph_synthetic_equals_the_documented_eager_loop(tmp_path, capsys):
    """epochs 60 and 61 of the ucf101 / 64 px schedule (milestones 60 / 80 / 100): the first runs at lr, the second at lr / 10 -- the
    entry captures a second train step; parameters and moments equal the by-hand loop's"""
    from dpc_amd import lc_main
    pr = str(tmp_path / "probe")
    os.makedirs(pr)
    lc_main.main(_args(["--batch_size", "2", "--synthetic", "3", "--start-epoch", "60", "--epochs", "62", "--graph"]), _probe=pr)
    out = capsys.readouterr().out
    got = torch.load(os.path.join(pr, "rank0.pt"))
    assert got["step"] == 6
    lines = GRAPH_LINE.findall(out)
    assert [int(n) for n, _, _ in lines] == [1, 3], out    # epoch 60: steps 0-1 are the eager warm-up
    assert all(float(ms) > 0 and abs(float(c) - 2e3 / float(ms)) < 0.01 * float(c) + 0.1 for _, ms, c in lines)
    assert out.count("lr 0.001\n") == 3 and out.count("lr 0.0001\n") == 3 and "Training from ep 60 to ep 62 finished" in out
    # by hand: each train step = fill_synthetic(1000) + train_step(None, None); each validation step = fill + eval-mode forward
    eng = _eng(torch.bfloat16)
    ms = lc_main.lr_milestones("ucf101", fe.SIZE)
    assert ms == [60, 80, 100]
    for epoch in (60, 61):
        for _ in range(3):
            _train(eng)
        _eval(eng)
        eng.lr = 1e-3 * lc_main.lr_multiplier(epoch, 0.1, ms, 1)
        assert abs(eng.lr - 1e-4) < 1e-12   # one milestone passed from epoch 60 on
    torch.cuda.synchronize()
    assert len(eng._captures) == 0 and eng.step_count == 6
    assert torch.equal(got["flat_p"], eng.flat_p.cpu()) and torch.equal(got["flat_m"], eng.flat_m.cpu())


def _frames_graph_case(tmp_path, capfd, gpus, B, train_what):
    from dpc_amd import lc_main
    world = len(gpus.split(","))
    steps = 2
    clips = fe.variants(fe.base_frames(), B * steps, 3)
    labels = (np.arange(B * steps) * 37 + 5) % fe.NUM_CLASS
    fp, lp = os.path.join(str(tmp_path), "clips.npy"), os.path.join(str(tmp_path), "labels.npy")
    np.save(fp, clips)
    np.save(lp, labels)
    argv = _args(["--batch_size", str(B), "--gpu", gpus, "--epochs", "2", "--crop", str(fe.CROP), "--frames", fp, "--labels", lp,
                  "--train_what", train_what])
    runs = {}
    for mode in ("eager", "graph"):
        pr = str(tmp_path / mode)
        os.makedirs(pr)
        lc_main.main(argv + (["--graph"] if mode == "graph" else []), _probe=pr)
        out = capfd.readouterr().out   # (fd level: rank 0 of a two-rank run is a child process)
        runs[mode] = ([torch.load(os.path.join(pr, f"rank{r}.pt")) for r in range(world)],
                      [ln for ln in out.splitlines() if "Loss" in ln], GRAPH_LINE.findall(out))
    (pe, le, ge), (pg, lg_, gg) = runs["eager"], runs["graph"]
    assert all(r["step"] == 2 * steps for r in pe + pg)
    for a, b in zip(pe, pg):
        assert torch.equal(a["flat_p"], b["flat_p"]) and torch.equal(a["flat_m"], b["flat_m"]) and a["flat_m"].abs().sum() > 0
    assert le == lg_ and len(le) == 2 * (steps + 1)   # every train step is logged (print_freq 1) + one validation line per epoch
    assert ge == [] and [int(n) for n, _, _ in gg] == [steps]   # epoch 0 is the eager warm-up, epoch 1 is replayed


@pytest.mark.parametrize("train_what", ["all", "head"])
def test_entry_graph_frames_equals_eager(tmp_path, capfd, train_what):
    _frames_graph_case(tmp_path, capfd, "0", 2, train_what)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_entry_graph_frames_two_ranks(tmp_path, capfd):
    _frames_graph_case(tmp_path, capfd, "0,1", 4, "all")


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k_], b[k_]) for k_ in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_checkpoints_cross_between_graph_and_eager(tmp_path, capfd):
    """one epoch with --graph and one without write the same checkpoint (model, buffers, grouped optimizer state); the one written
    under --graph resumes without it, the other with it, and both second epochs end in the same bits"""
    from dpc_amd import lc_main
    B, steps = 2, 3
    fp, lp = os.path.join(str(tmp_path), "clips.npy"), os.path.join(str(tmp_path), "labels.npy")
    np.save(fp, fe.variants(fe.base_frames(), B * steps, 3))
    np.save(lp, (np.arange(B * steps) * 37 + 5) % fe.NUM_CLASS)
    base = _args(["--batch_size", str(B), "--crop", str(fe.CROP), "--frames", fp, "--labels", lp, "--train_what", "head"])

    def run(tag, extra):
        pr = str(tmp_path / tag)
        os.makedirs(pr)
        lc_main.main(base + extra, _probe=pr)
        return torch.load(os.path.join(pr, "rank0.pt")), GRAPH_LINE.findall(capfd.readouterr().out)

    sd_e, sd_g = str(tmp_path / "ckpt_eager"), str(tmp_path / "ckpt_graph")
    (e1, _), (g1, lines) = run("e1", ["--epochs", "1", "--save_dir", sd_e]), run("g1", ["--epochs", "1", "--save_dir", sd_g, "--graph"])
    assert [int(n) for n, _, _ in lines] == [1] and e1["step"] == g1["step"] == steps
    ck_e, ck_g = (torch.load(os.path.join(d, "epoch1.pth.tar"), map_location="cpu", weights_only=False) for d in (sd_e, sd_g))
    assert list(ck_e) == list(ck_g) and len(ck_e["optimizer"]["state"]) > 0
    for key in ck_e:
        assert _same(ck_e[key], ck_g[key]), key
    (a, la), (b, lb) = (run("graph_then_eager", ["--epochs", "2", "--resume", os.path.join(sd_g, "epoch1.pth.tar")]),
                        run("eager_then_graph", ["--epochs", "2", "--resume", os.path.join(sd_e, "epoch1.pth.tar"), "--graph"]))
    assert la == [] and [int(n) for n, _, _ in lb] == [1] and a["step"] == b["step"] == 2 * steps
    assert torch.equal(a["flat_p"], b["flat_p"]) and torch.equal(a["flat_m"], b["flat_m"]) and not torch.equal(a["flat_p"], e1["flat_p"])


_TEST_SCRIPT = r"""
import os, sys, json
sys.path.insert(0, {root!r})
os.chdir({root!r})
from dpc_amd import lc_main
argv = json.loads(sys.argv[1])
for mode in ("eager", "graph"):
    pr = os.path.join({out!r}, mode)
    os.makedirs(pr)
    lc_main.main(argv + (["--graph"] if mode == "graph" else []), _probe=pr)
    os.replace(argv[argv.index("--test") + 1] + ".confusion.npy", os.path.join(pr, "confusion.npy"))
"""


def test_test_protocol_on_replayed_graphs(tmp_path, clean_launcher):
    """`--test ckpt --frames ... --graph` against the same line without it on the four videos of tests/test_lc_frames_entry.py (full,
    shorter than the array, too short, full): totals, confusion matrix and skipped count bit for bit, the printed lines equal"""
    import json
    t = fe._train_entry(L.load_hip(), DEV, str(tmp_path), "bf16", None, 2, 2)
    torch.cuda.synchronize()
    videos = fe.variants(fe.long_video(fe.base_frames(), fe.F_TEST), len(fe.LENGTHS), 11)
    fp, lp, np_ = (os.path.join(str(tmp_path), n) for n in ("videos.npy", "vlabels.npy", "vlengths.npy"))
    np.save(fp, videos)
    np.save(lp, np.array([3, 50, 0, 100]))
    np.save(np_, np.array(fe.LENGTHS))
    argv = _args(["--batch_size", "2", "--crop", str(fe.CROP), "--frames", fp, "--labels", lp, "--lengths", np_, "--test", t["ckpt"]])
    script = tmp_path / "run_test.py"
    script.write_text(_TEST_SCRIPT.format(root=ROOT, out=str(tmp_path)))
    cmd = [sys.executable, str(script), json.dumps(argv)]
    env = dict(os.environ)
    if clean_launcher is not None:
        rc, out, err = clean_launcher.run(cmd, env, 600)
    else:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        rc, out, err = r.returncode, r.stdout, r.stderr
    assert rc == 0, out[-3000:] + "\n" + err[-3000:]
    e, g = (torch.load(os.path.join(str(tmp_path), mode, "rank0.pt")) for mode in ("eager", "graph"))
    assert e["totals"] == g["totals"] and e["totals"][3] == 3.0 and e["skipped"] == g["skipped"] == 1
    assert torch.equal(e["confusion"], g["confusion"]) and int(e["confusion"].sum()) == 3
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "eager", "confusion.npy")), np.load(os.path.join(str(tmp_path), "graph", "confusion.npy")))
    lines = [ln for ln in out.splitlines() if ln.startswith("Loss ") or "videos tested" in ln]
    assert len(lines) == 4 and lines[0] == lines[2] and lines[1].split(",")[:2] == lines[3].split(",")[:2], out
