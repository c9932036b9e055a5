"""Frames resident in HBM (`dpc_amd.main --frames ... --resident`) on the host simulator: csrc/recipe_draw.hip against
data.recipe_from_uniforms, dpc_store_to_input against hand-cut spans, BackboneEngine.load_resident at widths (8, 16, 32, 32), the
entry in-process, and the refusals of data.FrameStore / ResidentFrameSource.  The case bodies are in tests/resident_cases.py; the
MI355X runs the same ones (tests/test_resident_gpu.py)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import resident_cases as rc
from dpc_amd import _lib as L
from dpc_amd import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (8, 16, 32, 32)


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    return L.load_emulator()


@pytest.mark.parametrize("name", [s[0] for s in rc.DRAW_SHAPES])
def test_draw_kernel_equals_the_host_recipe_emu(emu, name):
    rc.draw_injected_case(emu, "cpu", name)


def test_draw_kernel_philox_emu(emu):
    rc.philox_case(emu, "cpu")


def test_host_recipe_distribution():
    rc.dist_host_case()


def test_draw_kernel_distribution_emu(emu):
    rc.dist_kernel_case(emu, "cpu")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("jitter", [True, False])
def test_store_gather_equals_hand_cut_spans_emu(emu, jitter, dtype):
    rc.gather_case(emu, "cpu", jitter, dtype)


def test_draw_kernel_rejects_emu(emu):
    rc.draw_rejects_case(emu, "cpu")


def test_load_resident_equals_load_recipe_emu(emu):
    rc.engine_case(emu, "cpu", torch.float32, WIDTHS, steps=2, train=False)


def test_entry_resident_emu(emu, tmp_path, capsys):
    rc.entry_case(str(tmp_path), capsys, graph=False, sim=emu, widths=WIDTHS)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _frames(n=30):
    return np.zeros((n, 6, 8, 3), np.uint8)


def test_store_refuses_what_does_not_fit(monkeypatch):
    st = D.FrameStore(_frames(), np.array([0, 14, 30]))
    assert st.nbytes == 30 * 6 * 8 * 3 and len(st) == 2
    monkeypatch.setattr(D, "free_device_memory", lambda device: 5000)
    with pytest.raises(ValueError, match=r"needs 4320 bytes .* only 4000 are available \(5000 free, 1000 still"):
        st.to_device("cpu", reserve=1000)
    assert st.dev is None
    st.to_device("cpu", reserve=680)       # exactly what is there
    assert torch.equal(st.dev, torch.from_numpy(st.frames)) and st.offsets_dev.tolist() == [0, 14, 30]


def test_store_upload_goes_through_one_small_staging_buffer(monkeypatch):
    rng = np.random.Generator(np.random.PCG64(1))
    fr = rng.integers(0, 256, (30, 6, 8, 3), dtype=np.uint8)
    made = []
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: made.append(real(*a, **k)) or made[-1])
    st = D.FrameStore(fr, np.array([0, 14, 30])).to_device("cpu", chunk_bytes=1000)   # 4320 bytes: four full chunks and a rest
    assert [t.numel() for t in made] == [4320, 1000]
    assert torch.equal(st.dev, torch.from_numpy(fr))


@pytest.mark.parametrize("offsets,msg", [([0, 20, 14, 30], "never decrease"), ([1, 14, 30], "start at 0"), ([0, 14, 29], "ends at 29 but the store holds 30"),
                                         ([0, 14, 31], "ends at 31"), ([[0, 30]], "integers"), ([0.0, 30.0], "integers")])
def test_store_refuses_bad_offsets(offsets, msg):
    with pytest.raises(ValueError, match=msg):
        D.FrameStore(_frames(), np.array(offsets))


def test_store_says_which_flag_is_missing():
    with pytest.raises(ValueError, match="needs --offsets"):
        D.FrameStore(_frames())
    with pytest.raises(ValueError, match="dense 5-D"):
        D.FrameStore(np.zeros((2, 15, 6, 8, 3), np.uint8), np.array([0, 15, 30]))
    dense = D.FrameStore(np.zeros((2, 15, 6, 8, 3), np.uint8))
    assert dense.offsets.tolist() == [0, 15, 30] and dense.frames.shape == (30, 6, 8, 3)


def test_source_drops_short_videos_and_refuses_when_none_is_left():
    fr = np.zeros((40, 8, 8, 3), np.uint8)
    st = D.FrameStore(fr, np.array([0, 12, 25, 25, 40])).to_device("cpu")     # 12 (span exactly: dropped), 13, 0, 15 frames
    src = D.ResidentFrameSource(st, "ucf101", 2, 3, 2, 8, 1, "cpu", crop=8)
    assert src.keep.tolist() == [1, 3] and src.skipped == 2 and len(src) == 2
    assert sorted(src.begin_epoch().reshape(-1).tolist()) == [1, 3]
    with pytest.raises(ValueError, match="every one of the 4 videos is too short"):
        D.ResidentFrameSource(st, "ucf101", 2, 3, 3, 8, 1, "cpu", crop=8)
    with pytest.raises(ValueError, match="do not fill one batch"):
        D.ResidentFrameSource(st, "ucf101", 2, 3, 2, 8, 4, "cpu", crop=8)
    with pytest.raises(ValueError, match="too small"):
        D.ResidentFrameSource(st, "ucf101", 2, 3, 2, 8, 1, "cpu", crop=12)
    with pytest.raises(ValueError, match="upload the store first"):
        D.ResidentFrameSource(D.FrameStore(fr, np.array([0, 40])), "ucf101", 2, 3, 2, 8, 1, "cpu", crop=8)


def test_entry_says_which_flag_is_missing(tmp_path):
    from dpc_amd import main as dpc_main
    with pytest.raises(SystemExit, match="--frames is missing"):
        dpc_main.main(["--resident", "--gpu", "0"])
    fp, op = str(tmp_path / "f.npy"), str(tmp_path / "o.npy")
    np.save(fp, np.zeros((2, 70, 60, 80, 3), np.uint8))
    np.save(op, np.array([0, 70, 140]))
    with pytest.raises(ValueError, match="--resident is missing"):
        dpc_main.main(["--frames", fp, "--offsets", op, "--gpu", "0", "--dataset", "k400", "--img_dim", "64", "--batch_size", "1"],
                      _simulator=L.load_emulator(), _widths=WIDTHS)


def test_recipe_from_uniforms_is_a_function_of_the_row():
    """a rejected attempt keeps its slots: changing the uniforms of attempts behind the accepted one changes nothing"""
    rng = np.random.Generator(np.random.PCG64(2))
    u = rng.integers(0, 1 << 24, D.recipe_slots(rc.N_FR)).astype(np.float64) * 2.0 ** -24
    a = D.recipe_from_uniforms("k400", u, 40, 40, 30, 16, 16, rc.N_FR, rc.SPAN)
    v = u.copy()
    v[D.SLOT_ATTEMPT + 5:D.SLOT_FRAME] = 0.5
    b = D.recipe_from_uniforms("k400", v, 40, 40, 30, 16, 16, rc.N_FR, rc.SPAN)
    assert rc._fits(40, 30, *u[D.SLOT_ATTEMPT:D.SLOT_ATTEMPT + 3])
    assert all(np.array_equal(a[k], b[k]) for k in ("xb", "xk", "yb", "yk", "gray")) and bytes(a["jitter"]) == bytes(b["jitter"])
    assert set(a) == {"start", "x1", "y1", "flip", "xb", "xk", "yb", "yk", "gray", "jitter"}
    with pytest.raises(ValueError, match="uniforms per clip"):
        D.recipe_from_uniforms("k400", u[:-1], 40, 40, 30, 16, 16, rc.N_FR, rc.SPAN)
    with pytest.raises(ValueError, match="too short"):
        D.recipe_from_uniforms("k400", u, rc.SPAN, 40, 30, 16, 16, rc.N_FR, rc.SPAN)
