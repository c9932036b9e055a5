"""CPU tier (host SIMT simulator, width-reduced net (8,16,32,32), 64 px, B = 2, as tests/test_lc.py): torch autograd through
dpc_amd.lc.LC, the reference's training lines (eval/test.py:229-255) over it with dpc_amd.optim.Adam under parameter groups and
frozen parameters, and the two --train_what values of dpc_amd.lc_main that use them."""
import os
import subprocess

import pytest
import torch

import lc_loop_cases as lc
from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (8, 16, 32, 32)


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return L.load_emulator()


@pytest.fixture(scope="module")
def cfg(emu):
    """two blocks per clip for the loop, frozen and entry tests: they compare two runs of the SAME kernels (a torch.optim.Adam
    replica, a resumed run) or check which slices moved, so the length of the ConvGRU chain changes nothing they look at, while the
    simulator's time grows with it; the gradient test above, which is about the chain, runs all eight, and so does the GPU tier"""
    return lc.Cfg(device="cpu", simulator=emu, widths=WIDTHS, num_class=11, N=2)


def test_arbitrary_upstream_gradient(emu):
    """eight blocks per clip, as tests/test_lc.py: the gradient runs back through the whole ConvGRU chain"""
    lc.case_upstream_gradient(lc.Cfg(device="cpu", simulator=emu, widths=WIDTHS, num_class=11, N=8))


def test_autograd_decides_the_truncation(cfg):
    lc.case_autograd_decides_the_truncation(cfg)


def test_reference_loop_with_one_group_per_parameter(cfg):
    lc.case_reference_loop_grouped(cfg)


@pytest.mark.parametrize("how", ["all_parameters", "filter_requires_grad"])
def test_frozen_extractor(cfg, how):
    lc.case_frozen(cfg, how)


def test_set_param_groups_table(cfg):
    lc.case_set_param_groups(cfg)


def _entry(emu, argv, probe):
    from dpc_amd import lc_main
    os.makedirs(probe, exist_ok=True)
    lc_main.main(["--net", "resnet18", "--img_dim", "64", "--batch_size", "2", "--gpu", "0", "--print_freq", "1", "--dtype", "f32",
                  "--num_seq", "2", "--wd", "0"] + argv, _simulator=emu, _widths=WIDTHS, _probe=probe)
    return torch.load(os.path.join(probe, "rank0.pt"))


def _initial(emu):
    """the arena lc_main starts from (LC(seed=0)'s initial values in an LCEngine of the same shape)"""
    from dpc_amd.lc import LC, LCEngine
    eng = LCEngine("resnet18", 64, 2, 5, 2, "cpu", torch.float32, WIDTHS, lib=emu, num_class=101)
    eng.load_params({k: v.detach() for k, v in LC(64, 2, 5, "resnet18", 0.5, 101, widths=WIDTHS, seed=0).state_dict().items()})
    return eng


def _slices(eng):
    ext = torch.zeros(eng.numel, dtype=torch.bool)
    real = torch.zeros(eng.numel, dtype=torch.bool)
    for k, (o, n) in eng.offsets.items():
        real[o:o + n] = True
        if k.startswith(("backbone.", "agg.")):
            ext[o:o + n] = True
    return ext, real & ~ext


def test_lc_main_head(emu, tmp_path, capsys):
    """--train_what head: the extractor's slices of the parameter and moment arenas keep their initial bits, the head moves"""
    eng = _initial(emu)
    ext, head = _slices(eng)
    r = _entry(emu, ["--synthetic", "2", "--epochs", "1", "--train_what", "head"], str(tmp_path / "p"))
    out = capsys.readouterr().out
    assert "=> train only final_bn / final_fc" in out and "lr 0.001" in out
    assert r["step"] == 2
    assert torch.equal(r["flat_p"][ext].view(torch.int32), eng.flat_p[ext].view(torch.int32))
    assert r["flat_m"][ext].abs().max().item() == 0
    assert not torch.equal(r["flat_p"][head], eng.flat_p[head]) and (r["flat_p"][head] != eng.flat_p[head]).float().mean().item() > 0.9


def test_lc_main_ft_backbone_and_resume(emu, tmp_path, capsys):
    """--train_what ft_backbone.  (1) One step from zero moments: Adam's first step is lr * g / (|g| + eps) = +-lr per element, so the
    extractor (lr / 10) moves one tenth as far as the head: ratio of the two mean |dp| within 1 % of 0.1 (weight decay 0).
    That is true of every element with g != 0, and the means are taken over those (the elements that moved).  Elements whose
    gradient is exactly 0 do not move under any lr: at 64 px layer4's maps are 2 x 2, so 2 % of the extractor's elements are 3x3x3
    taps that only ever meet padding (over ALL elements the extractor's mean |dp| is 0.9797e-4, ratio 0.0980), and with
    Dropout(0.5) and two clips a quarter of final_fc's columns see y = 0 in both (ratio 0.1307 over all elements).
    (2) save -> --resume -> the next steps leave the bits of a run that was never interrupted.  The entry's synthetic batch
    generator starts over in every process, so the uninterrupted run is restated here on the engine: the same steps, fed what the
    two processes saw, with no file in between."""
    eng0 = _initial(emu)
    ext, head = _slices(eng0)
    d = str(tmp_path / "run")
    r1 = _entry(emu, ["--synthetic", "1", "--epochs", "1", "--train_what", "ft_backbone", "--save_dir", d], str(tmp_path / "p1"))
    out = capsys.readouterr().out
    assert "backbone.* and agg.* at lr / 10" in out
    dp = (r1["flat_p"] - eng0.flat_p).abs()
    moved = dp > 0
    de, dh = dp[ext & moved].mean().item(), dp[head & moved].mean().item()
    ratio = de / dh
    print(f"ft_backbone: mean |dp| of the moved elements: extractor {de:.4g} ({(ext & moved).sum().item()} of {ext.sum().item()}), "
          f"head {dh:.4g} ({(head & moved).sum().item()} of {head.sum().item()}), ratio {ratio:.5f}")
    assert abs(ratio - 0.1) <= 0.001, ratio
    assert (ext & moved).sum().item() > 0.95 * ext.sum().item() and (head & moved).sum().item() > 0.6 * head.sum().item()
    f1 = os.path.join(d, "epoch1.pth.tar")
    ck = torch.load(f1, map_location="cpu", weights_only=False)
    n_ext = sum(1 for k in eng0.offsets if k.startswith(("backbone.", "agg.")))
    assert [len(g["params"]) for g in ck["optimizer"]["param_groups"]] == [n_ext, len(eng0.offsets) - n_ext]
    assert [g["lr"] for g in ck["optimizer"]["param_groups"]] == pytest.approx([1e-4, 1e-3])
    assert len(ck["optimizer"]["state"]) == len(eng0.offsets) and float(ck["optimizer"]["state"][0]["step"]) == 1.0
    r2 = _entry(emu, ["--synthetic", "1", "--epochs", "2", "--train_what", "ft_backbone", "--resume", f1], str(tmp_path / "p2"))
    assert r2["step"] == 2 and "Epoch: [1][0/1]" in capsys.readouterr().out
    # the uninterrupted run: lc_main's own steps (its batch generator, its groups) on one engine
    shape = (2, 2, 3, 5, 64, 64)
    names_ext = [k for k in eng0.offsets if k.startswith(("backbone.", "agg."))]
    eng0.set_param_groups([{"params": names_ext, "lr": 1e-3 / 10, "weight_decay": 0.0},
                           {"params": [k for k in eng0.offsets if k not in names_ext], "lr": 1e-3, "weight_decay": 0.0}])
    for _ in range(2):   # each process: generator seeded 1000, one train batch (the validation batch after it changes no state)
        gen = torch.Generator("cpu").manual_seed(1000)
        x, y = torch.randn(shape, generator=gen), torch.randint(0, 101, (2,), generator=gen)
        eng0.train_step(x, y)
    assert torch.equal(r2["flat_p"].view(torch.int32), eng0.flat_p.view(torch.int32))
    assert torch.equal(r2["flat_m"].view(torch.int32), eng0.flat_m.view(torch.int32))
