"""The classifier's resident frames (`dpc_amd.lc_main --frames ... --labels ... --resident`) on the host simulator: the anchor of the
host statement to data.draw_lc (no kernel involved), dpc_draw_recipe_ex against that statement, load_resident with labels at widths
(8, 16, 32, 32), the entry in-process and as two gloo ranks, and the refusals of data.FrameStore / ResidentLabelledSource / the
entry.  The case bodies are in tests/resident_lc_cases.py; the MI355X runs the same ones (tests/test_resident_lc_gpu.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import resident_cases as rc
import resident_lc_cases as lc
from dpc_amd import _lib as L
from dpc_amd import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (8, 16, 32, 32)


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return L.load_emulator()


# ---- the host statement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,shape", lc.LC_CASES, ids=lc.LC_IDS)
def test_host_statement_equals_draw_lc(mode, shape):
    lc.anchor_case(mode, *shape)


def test_resident_lc_recipes_are_the_lc_recipes_as_descriptors():
    assert set(D.RESIDENT_LC_RECIPES) == {"train", "val"}
    for name, p, v in (("train", 1.0, (0.5, 0.5, 0.5, 0.25)), ("val", 0.3, (0.2, 0.2, 0.2, 0.1))):
        d = D.recipe_desc(D.RESIDENT_LC_RECIPES[name])
        assert (d.sized_p, d.gray_p, d.jitter_p, d.flip_code) == (p, -1.0, 0.3, 1)
        assert (d.brightness, d.contrast, d.saturation, d.hue) == v
        assert d.flags == L.RECIPE_JITTER_CONSISTENT | L.RECIPE_SCALE_AFTER_SIZED == 3
        assert ctypes.sizeof(d) == 64
    assert D.recipe_desc("k400").flags == 0 and D.recipe_desc("ucf101").flags == 0
    assert D.resident_ks(D.RESIDENT_LC_RECIPES["train"], 320, 240, 128, 224) == 5 and D.resident_ks("k400", 320, 240, 128) == 7
    with pytest.raises(ValueError, match="pass it"):
        D.resident_ks(D.RESIDENT_LC_RECIPES["train"], 320, 240, 128)
    with pytest.raises(ValueError, match="sized_p is None"):
        D.recipe_from_uniforms(dict(D.RECIPES["ucf101"], scale_after_sized=True), np.zeros(D.recipe_slots(6)), 20, 20, 14, 8, 8, 6, 12)


def test_host_recipe_distribution():
    lc.dist_host_case()


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,shape", lc.LC_CASES, ids=lc.LC_IDS)
def test_draw_kernel_equals_the_host_recipe_emu(emu, mode, shape):
    lc.draw_injected_case(emu, "cpu", mode, *shape)


@pytest.mark.parametrize("name", [s[0] for s in rc.DRAW_SHAPES])
def test_new_entry_with_the_additions_off_is_the_old_one_emu(emu, name):
    lc.additions_off_case(emu, "cpu", name)


def test_old_entry_ignores_the_flags_emu(emu):
    lc.old_entry_ignores_flags_case(emu, "cpu")


def test_draw_kernel_philox_emu(emu):
    lc.philox_case(emu, "cpu")


def test_draw_kernel_distribution_emu(emu):
    lc.dist_kernel_case(emu, "cpu")


def test_draw_kernel_rejects_emu(emu):
    lc.draw_rejects_case(emu, "cpu")


def test_abi_version_moved_with_the_new_entry(emu):
    assert L.ABI_VERSION == 2 and emu.call("dpc_abi_version") == 2


# ---- the engine and the entry -------------------------------------------------------------------------------------------------------
def test_load_resident_with_labels_equals_load_recipe_emu(emu):
    """operand bits and `target` only, f32 (see resident_lc_cases.engine_case); the steps themselves run on the MI355X tier and,
    through the entry, in test_entry_resident_equals_the_documented_loop_emu"""
    lc.engine_case(emu, "cpu", torch.float32, WIDTHS, B=2, train=False)


def test_entry_resident_equals_the_documented_loop_emu(emu, tmp_path, capsys):
    lc.entry_by_hand_case(emu, "cpu", str(tmp_path), capsys, "f32", WIDTHS, 2, "head", _simulator=emu, _widths=WIDTHS)


def test_entry_resident_two_gloo_ranks_draw_disjoint_shards(emu, tmp_path, capfd):
    """two simulator ranks over gloo: every rank holds the whole store, each draws its own shard of the epoch's permutation (read off
    sources built and seeded as the entry builds and seeds them), and the exchanged gradients leave the same parameters on both"""
    fp, lp, np_ = lc.entry_files(str(tmp_path))
    argv = lc.entry_argv(fp, lp, np_, 2, "f32", ["--epochs", "1", "--train_what", "head", "--resident"])
    i = argv.index("--gpu")
    pr = lc.run_entry(str(tmp_path), "probe", argv[:i] + ["--gpu", "0,1"] + argv[i + 2:], _simulator=emu, _widths=WIDTHS)
    r0, r1 = (torch.load(os.path.join(pr, f"rank{r}.pt")) for r in range(2))
    assert r0["world"] == r1["world"] == 2 and r0["per_gpu"] == 1 and r0["step"] == r1["step"] == 2
    st = D.FrameStore(fp, None, np_).to_device("cpu")
    shards = []
    for rank in range(2):   # lc_main: torch.manual_seed(0) on every rank, then the train source's begin_epoch
        src = D.ResidentLabelledSource(st, lp, "ucf101", lc.E_N, lc.E_SL, lc.E_DS, lc.E_SIZE, 1, lc.E_CLASSES, "cpu", "train", rank, 2, lc.E_CROP, seed=rank)
        torch.manual_seed(0)
        shards.append(src.begin_epoch())
        assert shards[-1].shape == (2, 1) and len(src) == r0["step"]
    s0, s1 = (sorted(s.reshape(-1).tolist()) for s in shards)
    assert len(s0) == len(s1) == 2 and not set(s0) & set(s1) and sorted(s0 + s1) == [0, 1, 2, 3], (s0, s1)
    assert torch.equal(r0["flat_p"], r1["flat_p"]) and r0["flat_m"].abs().sum() > 0


def test_test_and_retrieval_resident_equal_the_uploading_runs_emu(emu, tmp_path, capsys):
    lc.protocol_case(str(tmp_path), capsys, _simulator=emu, _widths=WIDTHS)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_store_lengths_go_with_the_dense_array():
    dense = np.zeros((3, 15, 6, 8, 3), np.uint8)
    st = D.FrameStore(dense, None, np.array([15, 9, 13]))
    assert st.video_lengths.tolist() == [15, 9, 13] and st.offsets.tolist() == [0, 15, 30, 45] and st.long_enough(12).tolist() == [0, 2]
    assert D.FrameStore(dense).video_lengths.tolist() == [15, 15, 15] and D.FrameStore(dense).long_enough(12).tolist() == [0, 1, 2]
    st.to_device("cpu")
    assert st.lengths_dev.tolist() == [15, 9, 13] and st.lengths_dev.dtype == torch.int64 and D.FrameStore(dense).to_device("cpu").lengths_dev is None
    with pytest.raises(ValueError, match=r"--lengths .* --offsets"):
        D.FrameStore(dense.reshape(45, 6, 8, 3), np.array([0, 15, 30, 45]), np.array([15, 9, 13]))
    with pytest.raises(ValueError, match=r"--lengths .* --offsets"):
        D.FrameStore(dense, np.array([0, 15, 30, 45]), np.array([15, 9, 13]))
    with pytest.raises(ValueError, match="one integer per clip: 3 clips"):
        D.FrameStore(dense, None, np.array([15, 9]))
    with pytest.raises(ValueError, match="one integer per clip"):
        D.FrameStore(dense, None, np.array([15.0, 9.0, 13.0]))
    with pytest.raises(ValueError, match=r"lengths must lie in \[0, 15\]"):
        D.FrameStore(dense, None, np.array([15, 16, 13]))


def test_labelled_source_refusals(emu):
    fr = np.zeros((4, 15, 8, 8, 3), np.uint8)
    st = D.FrameStore(fr, None, np.array([15, 12, 13, 0])).to_device("cpu")      # 12 = the span exactly: dropped
    mk = lambda labels=(1, 2, 3, 4), dataset="ucf101", recipe="train", batch=1, crop=8, store=st, ds=2, num_class=5: \
        D.ResidentLabelledSource(store, np.asarray(labels), dataset, 2, 3, ds, 8, batch, num_class, "cpu", recipe, crop=crop)   # noqa: E731
    src = mk()
    assert src.keep.tolist() == [0, 2] and src.skipped == 2 and len(src) == 2 and src.labels_dev.tolist() == [1, 2, 3, 4] and src.crop == 8
    assert sorted(src.begin_epoch().reshape(-1).tolist()) == [0, 2] and src.scale_tab is None and src.KS == 3
    with pytest.raises(ValueError, match="dataset not supported"):
        mk(dataset="k400")
    with pytest.raises(ValueError, match="recipe must be one of"):
        mk(recipe="k400")
    with pytest.raises(ValueError, match="--labels wants one integer per clip: 4 clips"):
        mk(labels=(1, 2, 3))
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 5\): found 1 .. 5"):
        mk(labels=(1, 2, 3, 5))
    with pytest.raises(ValueError, match=r"the recipes crop 12 x 12 .* too small"):
        mk(crop=12)
    with pytest.raises(ValueError, match="upload the store first"):
        mk(store=D.FrameStore(fr))
    with pytest.raises(ValueError, match="every one of the 4 videos is too short"):
        mk(ds=3)
    with pytest.raises(ValueError, match="do not fill one batch"):
        mk(batch=4)
    # the test protocol: no batches, file order, device slices of the store's head of each slot
    test = mk(recipe="test", batch=4)
    got = list(test.videos())
    assert [g[0] for g in got] == [0, 2] and [g[2] for g in got] == [1, 3] and [tuple(g[1].shape) for g in got] == [(15, 8, 8, 3), (13, 8, 8, 3)]
    assert got[1][1].data_ptr() == st.dev[30:].data_ptr() and got[0][3] == D.lc_test_windows(15, 2, 3, 2, "ucf101")
    # the draw's target must be what the kernel writes into
    with pytest.raises(ValueError, match=r"target: a contiguous int64 \[1\]"):
        src.draw_recipe(emu, target=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"target: a contiguous int64 \[1\]"):
        src.draw_recipe(emu, target=torch.zeros(1, dtype=torch.int32))
    # ... and a source without labels has nothing to write there, whichever entry it would call
    plain = D.ResidentFrameSource(D.FrameStore(fr).to_device("cpu"), "ucf101", 2, 3, 2, 8, 1, "cpu", crop=8)
    assert plain.labels_dev is None and plain.store.lengths_dev is None
    with pytest.raises(ValueError, match="for a source that carries labels"):
        plain.draw_recipe(emu, target=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="the store lives on cpu"):
        D.ResidentFrameSource(st, "ucf101", 2, 3, 2, 8, 1, "cuda:0", crop=8)


def test_entry_says_which_flag_is_missing_or_contradicts(tmp_path):
    from dpc_amd import lc_main
    with pytest.raises(ValueError, match="--resident holds the --frames array in HBM: --frames is missing"):
        lc_main.main(["--resident", "--gpu", "0"])
    with pytest.raises(ValueError, match="--offsets describes a packed frame store.*--resident is missing"):
        lc_main.main(["--frames", "f.npy", "--labels", "l.npy", "--offsets", "o.npy", "--gpu", "0"])
    with pytest.raises(ValueError, match="--offsets describes a packed frame store.*--resident is missing"):
        lc_main.main(["--frames", "f.npy", "--labels", "l.npy", "--val_offsets", "o.npy", "--gpu", "0"])
    with pytest.raises(ValueError, match="pass --lengths or --offsets, not both"):
        lc_main.main(["--frames", "f.npy", "--labels", "l.npy", "--offsets", "o.npy", "--lengths", "n.npy", "--resident", "--gpu", "0"])
    with pytest.raises(ValueError, match="pass --lengths or --offsets, not both"):
        lc_main.main(["--frames", "f.npy", "--labels", "l.npy", "--val_offsets", "o.npy", "--val_lengths", "n.npy", "--resident", "--gpu", "0"])
    with pytest.raises(ValueError, match="--val_offsets describes the packed store of --val_frames: --val_frames is missing"):
        lc_main.main(["--frames", "f.npy", "--labels", "l.npy", "--val_offsets", "o.npy", "--resident", "--gpu", "0"])
    help_text = " ".join(lc_main.build_parser().format_help().split())
    assert "different, equally distributed sample" in help_text and "--val_offsets" in help_text


def test_entry_resident_reads_a_packed_store_emu(emu, tmp_path, capsys):
    """--offsets: the same videos packed back to back give the same --test totals as the dense array with --lengths"""
    tmp = str(tmp_path)
    fp, lp, np_ = lc.entry_files(tmp)
    frames, lengths, _ = lc.lc_store_arrays()
    pp, op = os.path.join(tmp, "packed.npy"), os.path.join(tmp, "offsets.npy")
    np.save(pp, np.concatenate([frames[v, :n] for v, n in enumerate(lengths)]))
    np.save(op, np.concatenate([[0], np.cumsum(lengths)]))
    dense = lc.entry_argv(fp, lp, np_, 2, "f32", ["--test", "random", "--resident"])
    packed = dense[:dense.index("--frames")] + ["--frames", pp, "--labels", lp, "--offsets", op, "--test", "random", "--resident"]
    a = torch.load(os.path.join(lc.run_entry(tmp, "dense", dense, _simulator=emu, _widths=WIDTHS), "rank0.pt"))
    b = torch.load(os.path.join(lc.run_entry(tmp, "packed", packed, _simulator=emu, _widths=WIDTHS), "rank0.pt"))
    assert a["totals"] == b["totals"] and a["totals"][3] == 4.0 and torch.equal(a["confusion"], b["confusion"]) and b["skipped"] == 1
