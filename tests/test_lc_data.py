"""The data side of `python -m dpc_amd.lc_main --frames`: the three transform recipes of the downstream classifier
(eval/test.py:121-126,161-176), the test-time windows of eval/dataset_3d_lc.py:72-127 gathered from ONE resident video, the
host-side validation in front of the kernels, and the video-level reduction of eval/test.py:317-334 (csrc/lc_test.hip).

Expectations: tests/golden/lc_data.npz holds what the reference's OWN classes produced (tests/golden/make_lc_data_golden.py) --
bit-exact; the reduction is held to eval/test.py:317-334 restated in float64 torch below.  CPU tier = host simulator; the same
cases run on the MI355X under the gpu mark."""
import os
import random
import subprocess

import numpy as np
import pytest
import torch

from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return L.load_emulator()


def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def long_video(frames, F):
    """the same expression as tests/golden/make_lc_data_golden.py: the frames, their 180-degree rotation, a column roll -- cut to F"""
    return np.concatenate([frames, frames[:, ::-1, ::-1], np.roll(frames, 7, axis=2)])[:F].copy()


# ---- 1. recipes == the reference's Compose ---------------------------------------------------------------------------------------
def _recipes_case(lib, dev):
    from dpc_amd.data import draw_lc, recipe_to_input
    g, a = np.load(os.path.join(GOLDEN, "lc_data.npz")), np.load(os.path.join(GOLDEN, "aug.npz"))
    F, H0, W0, N, SL, ds, size, crop, start = (int(v) for v in a["params"])
    frames = torch.from_numpy(a["frames"]).unsqueeze(0).to(dev)
    for mode in ("train", "val", "test"):
        seeds = [int(s) for s in g[f"seeds::{mode}"]]
        assert len(seeds) == 8
        flags = []
        for s in seeds:
            random.seed(s)
            np.random.seed(s)
            clip = draw_lc(W0, H0, crop, size, N * SL, mode)
            flags.append((int(clip["sized_crop"]), int(clip["flip"] != 0), int(clip["jitter"][0].order[0] != 255)))
            block = torch.empty(1, N, 3, SL, size, size, device=dev)
            s2d = torch.empty(N, SL, size // 2, size // 2, 16, device=dev)
            recipe_to_input(lib, frames, [start], [clip], N, SL, ds, size, block, s2d)
            want, got = torch.from_numpy(g[f"{mode}::{s}"]), block[0].cpu()
            assert torch.equal(got, want), f"{mode} seed {s}: {(got != want).sum().item()} of {want.numel()} values differ, max {(got - want).abs().max().item():.3g}"
            chk = torch.empty_like(s2d)
            lib.call("dpc_pack_input_s2d", block, chk, L.F32, N, SL, size, size, lib.stream())
            _sync(dev)
            assert torch.equal(s2d.cpu(), chk.cpu())
        f = np.array(flags)
        assert np.array_equal(f, g[f"branches::{mode}"])     # the draws took the branches the reference's classes took
        for k in {"train": (1, 2), "val": (0, 1, 2), "test": ()}[mode]:   # (sized crop, flip, jitter): each branch a recipe has, twice on either side
            assert (f[:, k] == 1).sum() >= 2 and (f[:, k] == 0).sum() >= 2, (mode, k, flags)
        if mode == "train":
            assert (f[:, 0] == 1).all()
        if mode == "test":
            assert not f.any()


def test_lc_recipes_match_the_reference_classes_emu(emu):
    _recipes_case(emu, "cpu")


@pytest.mark.gpu
def test_lc_recipes_match_the_reference_classes_gpu():
    _recipes_case(L.load_hip(), "cuda:0")


# ---- 2. windows == the reference's __getitem__ -----------------------------------------------------------------------------------
def _windows_case(lib, dev):
    from dpc_amd.data import draw_lc, lc_test_windows, video_windows_to_input
    g, a = np.load(os.path.join(GOLDEN, "lc_data.npz")), np.load(os.path.join(GOLDEN, "aug.npz"))
    _, H0, W0, _, _, _, size, crop, _ = (int(v) for v in a["params"])
    FL = int(g["item_F"][0])
    video = torch.from_numpy(long_video(a["frames"], FL)).to(dev)     # ONE copy on the device
    for name, dataset, n_win in (("ucf101", "ucf101", 6), ("hmdb51", "hmdb51", 4), ("short", "ucf101", 4)):
        vlen, N, SL, ds = (int(v) for v in g[f"item_params::{name}"])
        want = torch.from_numpy(g[f"item::{name}"])
        starts = lc_test_windows(vlen, N, SL, ds, dataset)
        assert len(starts) == n_win == want.shape[0]
        assert (name == "short") == (vlen < FL)
        clip = draw_lc(W0, H0, crop, size, N * SL, "test")
        for chunk in (2, 3):
            got = []
            for i in range(0, len(starts), chunk):
                st = starts[i:i + chunk]
                block = torch.empty(len(st), N, 3, SL, size, size, device=dev)
                s2d = torch.empty(len(st) * N, SL, size // 2, size // 2, 16, device=dev)
                video_windows_to_input(lib, video, vlen, st, clip, N, SL, ds, size, block, s2d)
                chk = torch.empty_like(s2d)
                lib.call("dpc_pack_input_s2d", block, chk, L.F32, len(st) * N, SL, size, size, lib.stream())
                _sync(dev)
                assert torch.equal(s2d.cpu(), chk.cpu())
                got.append(block.cpu())
            assert torch.equal(torch.cat(got), want), (name, chunk)


def test_lc_test_windows_match_the_reference_getitem_emu(emu):
    _windows_case(emu, "cpu")


@pytest.mark.gpu
def test_lc_test_windows_match_the_reference_getitem_gpu():
    _windows_case(L.load_hip(), "cuda:0")


def test_window_starts_of_the_configurations_the_issue_verified():
    from dpc_amd.data import lc_test_windows
    assert len(lc_test_windows(40, 2, 2, 3, "ucf101")) == 6
    assert len(lc_test_windows(37, 4, 2, 1, "ucf101")) == 8
    assert len(lc_test_windows(37, 4, 2, 1, "hmdb51")) == 5
    assert lc_test_windows(37, 4, 2, 1, "hmdb51") == [0, 6, 12, 18, 24]
    assert lc_test_windows(8, 2, 2, 2, "ucf101") == []          # vlen - N * SL * ds <= 0: dropped by the dataset class


# ---- 3. host validation ------------------------------------------------------------------------------------------------------------
def test_lc_host_validation(emu):
    from dpc_amd.data import LabelledFrameSource, draw_lc, lc_test_windows, video_windows_to_input
    fr = np.zeros((3, 12, 30, 40, 3), np.uint8)
    mk = lambda **k: LabelledFrameSource(**{**dict(frames=fr, labels=np.array([0, 1, 2]), dataset="ucf101", num_seq=2, seq_len=2, ds=2, size=16,  # noqa: E731
                                                   batch=1, num_class=5, crop=28), **k})
    assert len(mk()) == 3 and mk().skipped == 0
    with pytest.raises(ValueError, match="lengths"):
        mk(lengths=np.array([12, 13, 12]))                       # lengths > F
    with pytest.raises(ValueError, match="labels"):
        mk(labels=np.array([0, 5, 2]))                           # label >= num_class
    with pytest.raises(ValueError, match="labels"):
        mk(labels=np.array([0, -1, 2]))
    with pytest.raises(ValueError, match="labels"):
        mk(labels=np.array([0, 1]))                              # label / clip count mismatch
    with pytest.raises(ValueError, match="too small"):
        mk(crop=31)                                              # frames smaller than the crop
    with pytest.raises(ValueError, match="num_seq"):
        lc_test_windows(40, 1, 5, 3, "ucf101")                   # stride 0
    with pytest.raises(ValueError, match="num_seq"):
        lc_test_windows(40, 1, 5, 3, "hmdb51")
    src = mk(lengths=np.array([12, 8, 10]))                      # 8 - 2 * 2 * 2 <= 0: skipped and counted
    assert src.skipped == 1 and len(src) == 2 and [v[0] for v in src.videos()] == [0, 2]
    # a window past vlen, before any launch (the frames exist in the array, the video does not have them)
    video = torch.zeros(12, 30, 40, 3, dtype=torch.uint8)
    clip = draw_lc(40, 30, 28, 16, 4, "test")
    block = torch.empty(1, 2, 3, 2, 16, 16)
    video_windows_to_input(emu, video, 12, [4], clip, 2, 2, 2, 16, block, None)     # last frame 4 + 3 * 2 = 10 < 12
    for vlen, st in ((10, [4]), (12, [6]), (12, [-1]), (13, [0])):
        with pytest.raises(ValueError):
            video_windows_to_input(emu, video, vlen, st, clip, 2, 2, 2, 16, block, None)
    bad = dict(clip, x1=13)                                      # 13 + 28 > 40
    with pytest.raises(ValueError, match="leaves"):
        video_windows_to_input(emu, video, 12, [0], bad, 2, 2, 2, 16, block, None)
    with pytest.raises(L.DpcError):                              # the C entry refuses a label outside [0, num_class) as well
        z = torch.zeros(5)
        emu.call("dpc_lc_test_finish", z, z.clone(), torch.ones(1, dtype=torch.int32), 5, 5, None, torch.zeros(4),
                 torch.zeros(4, dtype=torch.float64), torch.zeros(5, 5, dtype=torch.int64), emu.stream())


# ---- 4. reduction == eval/test.py:317-334 ------------------------------------------------------------------------------------------
def reference_video(logits32, label):
    """eval/test.py:317-334 for one video in float64: logits [windows, C] (the f32 values the kernel gets).  Returns
    (mean prob, loss, top1, top5, pred, margin = min_c |p_c - p_label| over c != label, top-2 logit gap)"""
    out = logits32.double()
    p = torch.softmax(out, 1).mean(0)
    top = p.topk(5).indices
    top1, top5 = float(top[0] == label), float((top == label).any())
    ml = out.mean(0)
    loss = float(torch.logsumexp(ml, 0) - ml[label])
    pred = int(ml.argmax())
    d = (p - p[label]).abs()
    d[label] = float("inf")
    t2 = ml.topk(2).values
    return p, loss, top1, top5, pred, float(d.min()), float(t2[0] - t2[1])


def issue_case(s, num_class):
    g = torch.Generator().manual_seed(s)
    rows = (3, 6, 17)[s % 3]
    logits = (3 * torch.randn(rows, num_class, generator=g, dtype=torch.float64)).float()
    label = int(torch.randint(0, num_class, (1,), generator=g))
    return logits, label


class Reducer:
    """the two entries of csrc/lc_test.hip on raw buffers"""

    def __init__(self, lib, dev, num_class):
        self.lib, self.dev, self.C = lib, dev, num_class
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)   # noqa: E731
        self.psum, self.lsum, self.count = z(num_class), z(num_class), z(1, dt=torch.int32)
        self.prob, self.video, self.totals, self.conf = z(num_class), z(4), z(4, dt=torch.float64), z(num_class, num_class, dt=torch.int64)

    def add(self, logits, n_valid):
        lg = logits.to(self.dev).contiguous()
        self.lib.call("dpc_lc_test_accumulate", lg, lg.shape[0], n_valid, self.C, lg.shape[1], self.psum, self.lsum, self.count, self.lib.stream())
        _sync(self.dev)

    def finish(self, label):
        self.lib.call("dpc_lc_test_finish", self.psum, self.lsum, self.count, self.C, label, self.prob, self.video, self.totals, self.conf,
                      self.lib.stream())
        _sync(self.dev)
        return self.prob.cpu().clone(), self.video.cpu().clone()


CASES = [(101, s) for s in (1, 2, 3, 5, 6)] + [(51, s) for s in (1, 2, 4, 5, 6, 7)]


def _reduction_case(lib, dev, capsys=None):
    worst_p = worst_l = 0.0
    for num_class, s in CASES:
        logits, label = issue_case(s, num_class)
        p, loss, top1, top5, pred, margin, gap = reference_video(logits, label)
        assert margin >= 1e-5 and gap >= 1e-2, (num_class, s, margin, gap)       # the decisions below are not rounding questions
        r = Reducer(lib, dev, num_class)
        r.add(logits, logits.shape[0])
        prob, video = r.finish(label)
        dp, dl = float((prob.double() - p).abs().max()), abs(float(video[0]) - loss)
        worst_p, worst_l = max(worst_p, dp), max(worst_l, dl)
        print(f"C {num_class} seed {s} rows {logits.shape[0]}: |dp| {dp:.3g} |dloss| {dl:.3g} margin {margin:.3g}")
        assert (float(video[1]), float(video[2]), int(video[3])) == (top1, top5, pred), (num_class, s)
        conf = r.conf.cpu()
        assert int(conf[pred, label]) == 1 and int(conf.sum()) == 1                # [pred][target]
        assert dp <= 1e-5 and dl <= 1e-5, (num_class, s, dp, dl)
        assert r.totals.cpu().tolist() == [float(video[0]), top1, top5, 1.0]
        assert not r.psum.cpu().any() and not r.lsum.cpu().any() and int(r.count.cpu()) == 0   # cleared for the next video
        # uneven chunks, padding rows of 1e3 that n_valid keeps out: bit for bit the one-chunk result; and a second run likewise
        rows = logits.shape[0]
        cuts = [0, 1, rows] if rows == 3 else [0, 2, rows - 3, rows]
        r2 = Reducer(lib, dev, num_class)
        for a, b in zip(cuts[:-1], cuts[1:]):
            pad = torch.full((b - a + 2, num_class), 1e3)
            pad[:b - a] = logits[a:b]
            r2.add(pad, b - a)
        prob2, video2 = r2.finish(label)
        assert torch.equal(prob2, prob) and torch.equal(video2, video) and torch.equal(r2.conf.cpu(), conf)
        r3 = Reducer(lib, dev, num_class)
        r3.add(logits, rows)
        prob3, video3 = r3.finish(label)
        assert torch.equal(prob3, prob) and torch.equal(video3, video)
    print(f"reduction: max |mean prob - f64| {worst_p:.3g}, max |loss - f64| {worst_l:.3g}")
    return worst_p, worst_l


def _ties_and_totals_case(lib, dev):
    # an exact tie between the label and another class counts for the label (strictly greater); pred takes the lower index
    C_ = 51
    row = torch.zeros(2, C_)
    row[:, 7] = 2.0
    row[:, 30] = 2.0                                              # same logits in both rows: p_7 == p_30 and l_7 == l_30 exactly
    for label, pred in ((30, 7), (7, 7)):
        r = Reducer(lib, dev, C_)
        r.add(row, 2)
        _, video = r.finish(label)
        assert float(video[1]) == 1.0 and float(video[2]) == 1.0 and int(video[3]) == pred
        assert int(r.conf.cpu()[7, label]) == 1
    # totals and the confusion matrix accumulate over three videos (two of them the same class pair)
    r = Reducer(lib, dev, 101)
    want_tot, want_conf = torch.zeros(4, dtype=torch.float64), torch.zeros(101, 101, dtype=torch.int64)
    for s in (1, 2, 1):
        logits, label = issue_case(s, 101)
        r.add(logits[:2], 2)
        r.add(logits[2:], logits.shape[0] - 2)
        _, video = r.finish(label)
        _, loss, top1, top5, pred, _, _ = reference_video(logits, label)
        want_tot += torch.tensor([float(video[0]), top1, top5, 1.0], dtype=torch.float64)
        want_conf[pred, label] += 1
        assert abs(float(video[0]) - loss) <= 1e-5
    assert torch.equal(r.conf.cpu(), want_conf) and int(want_conf.max()) == 2
    assert torch.equal(r.totals.cpu(), want_tot)


def test_lc_test_reduction_emu(emu):
    _reduction_case(emu, "cpu")
    _ties_and_totals_case(emu, "cpu")


@pytest.mark.gpu
def test_lc_test_reduction_gpu():
    _reduction_case(L.load_hip(), "cuda:0")
    _ties_and_totals_case(L.load_hip(), "cuda:0")
