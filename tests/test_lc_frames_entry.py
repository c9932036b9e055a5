"""`python -m dpc_amd.lc_main --frames --labels [--lengths]`: fine-tuning on labelled uint8 frames and the reference's video-level
test (eval/test.py:218-343, eval/dataset_3d_lc.py:72-127) end to end, and LCEngine.test_video underneath it.

Expectations: the same draws replayed by hand through f32 blocks (`recipe_to_input(block=...)`, which tests/golden/lc_data.npz
pins to the reference's own transform classes) and, for the test protocol, eval/test.py:317-334 restated in float64 torch over
the logits of by-hand eval-mode forwards.  CPU tier = host simulator at narrow widths; the same cases on the MI355X under the gpu
mark (the --test command line there as a child process, like tests/test_entries.py::test_main_and_lc_main_gpu)."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
WIDTHS = (8, 16, 32, 32)
N, SL, DS, SIZE, CROP, NUM_CLASS = 2, 2, 3, 64, 56, 101     # 12 of the 14 frames of aug.npz per training clip


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return L.load_emulator()


def base_frames():
    return np.load(os.path.join(GOLDEN, "aug.npz"))["frames"]     # [14, 60, 80, 3] u8


def long_video(frames, F):
    return np.concatenate([frames, frames[:, ::-1, ::-1], np.roll(frames, 7, axis=2)])[:F].copy()


def variants(video, n, seed):
    """n different videos from one: rolled in time or rotated, plus a little noise"""
    rng = np.random.default_rng(seed)
    out = np.stack([np.roll(video, k, axis=0) if k % 2 == 0 else video[:, ::-1][:, :, ::-1].copy() for k in range(n)])
    return (out.astype(np.int16) + rng.integers(-3, 4, out.shape)).clip(0, 255).astype(np.uint8)


def make_engine(lib, dev, dtype, widths, B, num_class=NUM_CLASS):
    """the engine as dpc_amd.lc_main builds it"""
    from dpc_amd.lc import LC, LCEngine
    from dpc_amd.plan import LAYER_WIDTH
    w = widths or LAYER_WIDTH
    cdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    eng = LCEngine("resnet18", SIZE, N, SL, B, dev, cdt, w, lib=lib if lib.kind != "hip" else None, lr=1e-3, wd=1e-3, dropout=0.5,
                   num_class=num_class, seed=666)
    init = LC(SIZE, N, SL, "resnet18", 0.5, num_class, widths=w, seed=0)
    eng.load_params({k: v.detach() for k, v in init.state_dict().items()})
    return eng


def reference_video(logits32, label):
    """eval/test.py:317-334 for one video in float64 over logits [windows, C]: (mean prob, loss, top1, top5, pred, margin)"""
    out = logits32.double()
    p = torch.softmax(out, 1).mean(0)
    top = p.topk(5).indices
    ml = out.mean(0)
    d = (p - p[label]).abs()
    d[label] = float("inf")
    return p, float(torch.logsumexp(ml, 0) - ml[label]), float(top[0] == label), float((top == label).any()), int(ml.argmax()), float(d.min())


# ---- 5. chunk size does not matter ---------------------------------------------------------------------------------------------
def _chunk_case(lib, dev, widths, exact):
    from dpc_amd.data import draw_lc, lc_test_windows
    video = long_video(base_frames(), 36)
    starts = lc_test_windows(36, N, SL, DS, "ucf101")
    assert len(starts) == 5                                     # batch 2: 2 + 2 + 1 (padded); batch 3: 3 + 2 (padded)
    clip = draw_lc(80, 60, CROP, SIZE, N * SL, "test")
    label, res = 4, []
    for B in (2, 3):
        eng = make_engine(lib, dev, "f32", widths, B, num_class=11)
        for _ in range(2):                                      # a second video through the same engine: the state was cleared
            eng.test_video(video, label, starts, clip, ds=DS)
        if dev != "cpu":
            torch.cuda.synchronize()
        res.append((eng.test_prob.cpu().clone(), eng.test_res.cpu().clone(), eng.test_totals.cpu().clone(), eng.test_confusion.cpu().clone()))
    (p2, r2, t2, c2), (p3, r3, t3, c3) = res
    worst = float((p2 - p3).abs().max())
    print(f"chunk size 2 vs 3: max |mean prob difference| {worst:.3g}, loss {float(r2[0]):.6f} vs {float(r3[0]):.6f}")
    assert torch.isfinite(p2).all() and abs(float(p2.sum()) - 1.0) < 1e-4 and float(t2[3]) == 2.0 and int(c2.sum()) == 2
    assert torch.equal(r2[1:], r3[1:]) and torch.equal(c2, c3)  # top-1, top-5, pred
    if exact:
        assert torch.equal(p2, p3) and torch.equal(r2, r3) and torch.equal(t2, t3)
    else:
        assert worst <= 1e-3
    return worst


def test_test_video_chunk_size_does_not_matter_emu(emu):
    _chunk_case(emu, "cpu", WIDTHS, exact=True)


@pytest.mark.gpu
def test_test_video_chunk_size_does_not_matter_gpu():
    """full widths, f32: the plan may pick another kernel for another M, so the project's f32 parity tolerance (1e-3) on the mean
    probabilities; the observed maximum is printed"""
    _chunk_case(L.load_hip(), "cuda:0", None, exact=False)


# ---- 6. entry, training --------------------------------------------------------------------------------------------------------
def _train_entry(lib, dev, tmp, dtype, widths, B, steps):
    """`lc_main --frames --labels` for one epoch of `steps` batches; returns what the by-hand side needs"""
    from dpc_amd import lc_main
    clips = variants(base_frames(), B * steps, 3)
    labels = (np.arange(B * steps) * 37 + 5) % NUM_CLASS
    fp, lp, pr, sd = (os.path.join(tmp, n) for n in ("clips.npy", "labels.npy", "probe", "ckpt"))
    np.save(fp, clips)
    np.save(lp, labels)
    os.makedirs(pr, exist_ok=True)
    argv = ["--net", "resnet18", "--img_dim", str(SIZE), "--batch_size", str(B), "--gpu", "0", "--print_freq", "1", "--dtype", dtype,
            "--num_seq", str(N), "--seq_len", str(SL), "--ds", str(DS), "--epochs", "1", "--dataset", "ucf101", "--crop", str(CROP),
            "--frames", fp, "--labels", lp, "--save_dir", sd]
    lc_main.main(argv, _simulator=lib if lib.kind != "hip" else None, _widths=widths, _probe=pr)
    return dict(frames=fp, labels=lp, probe=torch.load(os.path.join(pr, "rank0.pt")), ckpt=os.path.join(sd, "epoch1.pth.tar"),
                B=B, steps=steps, dtype=dtype, widths=widths, dev=dev, lib=lib)


def _check_train_entry(t):
    """the same draws replayed by hand: torch 0 / random 0 / np.random 0 as the entry seeds them, LabelledFrameSource's batches through
    an f32 block -> eng.train_step(block, y).  Parameters and Adam moments must be bit-identical."""
    from dpc_amd.data import LabelledFrameSource, recipe_to_input
    B, steps, dev = t["B"], t["steps"], t["dev"]
    assert t["probe"]["step"] == steps
    eng = make_engine(t["lib"], dev, t["dtype"], t["widths"], B)
    torch.manual_seed(0)
    random.seed(0)
    np.random.seed(0)
    src = LabelledFrameSource(t["frames"], t["labels"], "ucf101", N, SL, DS, SIZE, B, NUM_CLASS, "train", crop=CROP)
    assert len(src) == steps and src.skipped == 0
    n, seen = 0, []
    for frames, starts, cl, y in src.epoch(torch.device(dev)):
        block = torch.empty(B, N, 3, SL, SIZE, SIZE, device=dev)
        recipe_to_input(eng.lib, frames, starts, cl, N, SL, DS, SIZE, block, None)
        assert torch.isfinite(block).all() and block.std() > 0.3
        eng.train_step(block, y)
        seen += y.tolist()
        n += 1
    assert n == steps and sorted(seen) == sorted(np.load(t["labels"]).tolist())      # every clip once, with ITS label
    if dev != "cpu":
        torch.cuda.synchronize()
    assert torch.equal(t["probe"]["flat_p"], eng.flat_p.cpu()) and torch.equal(t["probe"]["flat_m"], eng.flat_m.cpu())
    assert t["probe"]["flat_m"].abs().sum() > 0
    ck = torch.load(t["ckpt"], map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and ck["iteration"] == steps


@pytest.fixture(scope="module")
def trained_emu(emu, tmp_path_factory):
    return _train_entry(emu, "cpu", str(tmp_path_factory.mktemp("lc_emu")), "f32", WIDTHS, 1, 2)


@pytest.fixture(scope="module")
def trained_gpu(tmp_path_factory):
    return _train_entry(L.load_hip(), "cuda:0", str(tmp_path_factory.mktemp("lc_gpu")), "bf16", None, 2, 2)


def test_lc_main_frames_training_emu(trained_emu):
    _check_train_entry(trained_emu)


@pytest.mark.gpu
def test_lc_main_frames_training_gpu(trained_gpu):
    _check_train_entry(trained_gpu)


# ---- 7. entry, test ------------------------------------------------------------------------------------------------------------
F_TEST, LENGTHS = 30, (30, 24, 12, 30)      # full, vlen < F (3 windows), too short (12 - 2 * 2 * 3 <= 0), full


def _by_hand_test(t, tmp, B):
    """the videos of the test file, the logits of by-hand eval-mode forwards (blocks from REPLICATED frames through recipe_to_input),
    labels picked from them by rank (0, 2, last) and the float64 restatement of eval/test.py:317-334"""
    from dpc_amd import checkpoint as ckpt
    from dpc_amd.data import draw_lc, lc_test_windows, recipe_to_input
    dev = t["dev"]
    videos = variants(long_video(base_frames(), F_TEST), len(LENGTHS), 11)
    eng = make_engine(t["lib"], dev, t["dtype"], t["widths"], B)
    ck = torch.load(t["ckpt"], map_location="cpu", weights_only=False)
    ckpt.load_model_state(eng, ck["state_dict"], strict=True)
    clip = draw_lc(80, 60, CROP, SIZE, N * SL, "test")
    labels, want, ranks = [], [], iter((0, 2, NUM_CLASS - 1))
    for v, vlen in zip(videos, LENGTHS):
        starts = lc_test_windows(vlen, N, SL, DS, "ucf101")
        if not starts:
            labels.append(0)
            continue
        logits = []
        for i in range(0, len(starts), B):
            st = starts[i:i + B]
            nv = len(st)
            st = st + [st[-1]] * (B - nv)
            frames = torch.from_numpy(np.stack([v[:vlen]] * B)).to(dev)
            block = torch.empty(B, N, 3, SL, SIZE, SIZE, device=dev)
            recipe_to_input(eng.lib, frames, st, [clip] * B, N, SL, DS, SIZE, block, None)
            out, _ = eng.forward(block, torch.zeros(B, dtype=torch.int64), train=False)
            logits.append(out.view(B, NUM_CLASS)[:nv].float().cpu().clone())
        logits = torch.cat(logits)
        assert logits.shape[0] == len(starts) and torch.isfinite(logits).all()
        p = torch.softmax(logits.double(), 1).mean(0)
        label = int(p.argsort(descending=True)[next(ranks)])
        labels.append(label)
        want.append(reference_video(logits, label))
    fp, lp, np_ = (os.path.join(tmp, n) for n in ("videos.npy", "vlabels.npy", "vlengths.npy"))
    np.save(fp, videos)
    np.save(lp, np.array(labels))
    np.save(np_, np.array(LENGTHS))
    for k, w in enumerate(want):
        print(f"video {k}: margin {w[5]:.3g} loss {w[1]:.6f} top1 {w[2]} top5 {w[3]} pred {w[4]}")
        assert w[5] >= 1e-5, (k, w[5])                               # the decisions below are not rounding questions
    conf = torch.zeros(NUM_CLASS, NUM_CLASS, dtype=torch.int64)
    for w, lab in zip(want, [l for l, n in zip(labels, LENGTHS) if n - N * SL * DS > 0]):
        conf[w[4], lab] += 1
    assert [w[2] for w in want] == [1.0, 0.0, 0.0] and [w[3] for w in want] == [1.0, 1.0, 0.0]     # ranks 0, 2, last
    return dict(argv=["--net", "resnet18", "--img_dim", str(SIZE), "--batch_size", str(B), "--gpu", "0", "--dtype", t["dtype"], "--num_seq", str(N),
                      "--seq_len", str(SL), "--ds", str(DS), "--dataset", "ucf101", "--crop", str(CROP), "--frames", fp, "--labels", lp,
                      "--lengths", np_, "--test", t["ckpt"]],
                loss=sum(w[1] for w in want), top1=sum(w[2] for w in want), top5=sum(w[3] for w in want), n=len(want), conf=conf)


def _check_test_outputs(t, h, out, log_before):
    m = re.search(r"^Loss ([0-9.]+)\t Acc top1: ([0-9.]+) Acc top5: ([0-9.]+) \t$", out, re.M)
    assert m, out
    n = h["n"]
    assert abs(float(m.group(1)) - h["loss"] / n) <= 5e-5 + 1e-5                    # four printed decimals of a loss held to 1e-5
    assert m.group(2) == "{:.4f}".format(h["top1"] / n) and m.group(3) == "{:.4f}".format(h["top5"] / n)
    assert "(test checkpoint epoch 1)" in out and re.search(r"^3 videos tested, 1 skipped \(too short", out, re.M), out
    conf = np.load(t["ckpt"] + ".confusion.npy")
    assert conf.dtype == np.int64 and conf.shape == (NUM_CLASS, NUM_CLASS) and np.array_equal(conf, h["conf"].numpy())   # [pred][target]
    log = open(os.path.join(os.path.dirname(t["ckpt"]), "test_log.md")).read()[len(log_before):]
    assert re.fullmatch(r"## Epoch 1:\ntime: \d{4}(_\d\d){5}\n" + re.escape(m.group(0)) + r"\n\n", log), log


def _log_so_far(t):
    p = os.path.join(os.path.dirname(t["ckpt"]), "test_log.md")
    return open(p).read() if os.path.exists(p) else ""


def test_lc_main_frames_test_emu(emu, trained_emu, tmp_path, capsys):
    from dpc_amd import lc_main
    t = trained_emu
    h = _by_hand_test(t, str(tmp_path), 2)
    pr = str(tmp_path / "probe")
    os.makedirs(pr)
    before = _log_so_far(t)
    capsys.readouterr()
    lc_main.main(h["argv"], _simulator=emu, _widths=WIDTHS, _probe=pr)
    out = capsys.readouterr().out
    got = torch.load(os.path.join(pr, "rank0.pt"))
    assert got["skipped"] == 1 and got["totals"][1:] == [h["top1"], h["top5"], float(h["n"])]
    print(f"sum of losses: entry {got['totals'][0]:.8f}, by hand (f64) {h['loss']:.8f}")
    assert abs(got["totals"][0] / h["n"] - h["loss"] / h["n"]) <= 1e-5
    assert torch.equal(got["confusion"], h["conf"])
    _check_test_outputs(t, h, out, before)
    # --test random: the printed lines only, nothing written; more than one GPU is refused
    os.remove(t["ckpt"] + ".confusion.npy")
    before = _log_so_far(t)
    lc_main.main(h["argv"][:-1] + ["random"], _simulator=emu, _widths=WIDTHS)
    out = capsys.readouterr().out
    assert re.search(r"^Loss [0-9.]+\t Acc top1: [0-9.]+ Acc top5: [0-9.]+ \t$", out, re.M) and "(test checkpoint epoch 0)" in out
    assert not os.path.exists(t["ckpt"] + ".confusion.npy") and not os.path.exists("random.confusion.npy") and _log_so_far(t) == before
    i = h["argv"].index("--gpu")
    with pytest.raises(ValueError, match="one GPU"):
        lc_main.main(h["argv"][:i] + ["--gpu", "0,1"] + h["argv"][i + 2:], _simulator=emu, _widths=WIDTHS)


@pytest.mark.gpu
def test_lc_main_frames_test_gpu(trained_gpu, tmp_path, clean_launcher):
    t = trained_gpu
    h = _by_hand_test(t, str(tmp_path), 2)
    torch.cuda.synchronize()
    before = _log_so_far(t)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-c", "import os, runpy, sys; os.chdir(sys.argv[1]); sys.argv = sys.argv[2:]; runpy.run_module(sys.argv[0], run_name='__main__')",
           ROOT, "dpc_amd.lc_main"] + h["argv"]
    if clean_launcher is not None:
        rc, out, err = clean_launcher.run(cmd, env, 600)
    else:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        rc, out, err = r.returncode, r.stdout, r.stderr
    assert rc == 0, out[-3000:] + "\n" + err[-3000:]
    _check_test_outputs(t, h, out, before)
