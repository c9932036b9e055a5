"""Case bodies of the resident classifier tests (`python -m dpc_amd.lc_main --frames ... --labels ... --resident`), shared by the
simulator tier (tests/test_resident_lc_emu.py) and the MI355X tier (tests/test_resident_lc_gpu.py): dpc_draw_recipe_ex through the
C ABI (the two recipe flags, `lengths`, the label gather), data.FrameStore(lengths=) / ResidentLabelledSource,
BackboneEngine.load_resident with labels, and the entry.

Expectations never come from the code under test.  The host statement (data.recipe_from_uniforms with the two recipe keys) is first
anchored to data.draw_lc -- which tests/golden/lc_data.npz pins to the reference's transform classes -- by serving draw_lc a row
of uniforms in its own call order; the kernel is then held, bit for bit, to that host statement fed with injected uniforms or with
kcases.philox4x32_10_np words; load_resident to load_recipe on hand-cut spans; the entry to the loop it documents.  The
distribution bounds are 4 standard errors of the exact law (Bernoulli(p): sqrt(p (1 - p) / n); uniform: sqrt(1 / (12 n)))."""
import ctypes as C
import math
import os

import numpy as np
import torch

import resident_cases as rc
from dpc_amd import _lib as L
from dpc_amd import data as D
from resident_cases import DS, LENGTHS, N, N_FR, SL, SPAN, TOP

# (W0, H0, crop, size): shrink with a Scale, enlarge (crop > H0: the train recipe only), tall, no Scale (crop == size)
LC_SHAPES = ((40, 30, 16, 8), (20, 14, 16, 8), (14, 20, 16, 8), (40, 30, 16, 16))
LC_CASES = [(mode, s) for s in LC_SHAPES for mode in ("train", "val") if mode == "train" or (s[2] <= s[0] and s[2] <= s[1])]
LC_IDS = ["{}-{}x{}-{}-{}".format(m, *s) for m, s in LC_CASES]
LABELS = np.array([7, 3, 9, 3, 0], np.int64)          # one label per video of LENGTHS; videos 1 and 3 share a class
SLOT_F = 32                                           # the dense store of the `lengths` cases: every video owns 32 frames


def recipe_of(mode):
    return D.RESIDENT_LC_RECIPES[mode]


# ---- (1) the host statement == draw_lc ----------------------------------------------------------------------------------------------
class Scripted:
    """Stands where dpc_amd/data.py has the module `random` and serves u[slot] in draw_lc's call order (eval/test.py:161-176 through
    utils/augmentation.py): the sized crop's p; per attempt area, aspect, swap and on acceptance x1, y1; the flip; the jitter's p;
    the four factors; shuffle.  Which slot a call reads follows from the kind of call alone: after a swap draw a randint means the
    attempt was accepted, a uniform that the next attempt begins, a random() that all ten were rejected."""

    def __init__(self, u):
        self.u, self.phase, self.att, self.sub, self.calls = u, "p", 0, 0, []

    def _slot(self, kind):
        if self.phase == "p":
            self.phase = "attempt"
            return D.SLOT_SIZED_P
        if self.phase == "attempt":
            s = D.SLOT_ATTEMPT + D.ATTEMPT_SLOTS * self.att
            if self.sub < 2 and kind == "uniform":
                self.sub += 1
                return s + self.sub - 1
            if self.sub == 2 and kind == "random":
                self.sub = 3
                return s + 2
            if self.sub in (3, 4) and kind == "randint":
                self.sub += 1
                if self.sub == 5:
                    self.phase = "flip"
                return s + self.sub - 1
            if self.sub == 3 and kind == "uniform":       # rejected: the next attempt's area
                self.att, self.sub = self.att + 1, 1
                return s + D.ATTEMPT_SLOTS
            assert kind == "random" and self.sub in (0, 3), (kind, self.sub)   # the p draw failed / ten attempts rejected: the flip is next
            self.phase = "flip"
        if self.phase == "flip":
            self.phase = "jitter_p"
            return D.SLOT_FLIP
        if self.phase == "jitter_p":
            self.phase, self.sub = "factors", 0
            return D.SLOT_JITTER_P
        assert self.phase == "factors" and kind == "uniform" and self.sub < 4
        self.sub += 1
        return D.SLOT_FRAME + 2 + self.sub - 1

    def _u(self, kind):
        s = self._slot(kind)
        self.calls.append(s)
        return float(self.u[s])

    def random(self):
        return self._u("random")

    def uniform(self, a, b):
        return a + (b - a) * self._u("uniform")

    def randint(self, a, b):
        return a + int(math.floor(self._u("randint") * (b - a + 1)))

    def shuffle(self, x):                                 # Fisher-Yates from the top, as random.shuffle walks
        for i in range(len(x) - 1, 0, -1):
            s = D.SLOT_FRAME + 6 + (3 - i)
            self.calls.append(s)
            q = int(math.floor(float(self.u[s]) * (i + 1)))
            x[i], x[q] = x[q], x[i]


def reject_all(u, W0, H0):
    """ten attempts that cannot fit: the largest area at the aspect that points the long side of the box along the short side of the frame"""
    for a in range(10):
        u[D.SLOT_ATTEMPT + 5 * a: D.SLOT_ATTEMPT + 5 * a + 3] = (TOP, 0.0 if W0 >= H0 else TOP, 0.75)
        assert not rc._fits(W0, H0, *u[D.SLOT_ATTEMPT + 5 * a: D.SLOT_ATTEMPT + 5 * a + 3])


def anchor_case(mode, W0, H0, crop, size, rows=200):
    """data.draw_lc fed the row in its call order == data.recipe_from_uniforms on the same row, field for field"""
    rng = np.random.Generator(np.random.PCG64(7))
    seen = dict(center=0, jitter=0, fallback=0, accepted=0)
    widest = 0
    for t in range(rows):
        u = rng.integers(0, 1 << 24, D.recipe_slots(N_FR)).astype(np.float64) * 2.0 ** -24
        if t % 7 == 0:
            reject_all(u, W0, H0)
        src, real = Scripted(u), D.random
        D.random = src
        try:
            c = D.draw_lc(W0, H0, crop, size, N_FR, mode)
        finally:
            D.random = real
        assert len(set(src.calls)) == len(src.calls), "a slot was read twice"
        h = D.recipe_from_uniforms(recipe_of(mode), u, 20, W0, H0, crop, size, N_FR, SPAN)
        for k in ("x1", "y1", "flip"):
            assert c[k] == h[k], (k, t, c[k], h[k])
        for k in ("xb", "xk", "yb", "yk"):
            assert c[k].dtype == h[k].dtype and np.array_equal(c[k], h[k]), (k, t)
        assert bytes(c["jitter"]) == bytes(h["jitter"]), ("jitter", t)
        assert (np.asarray(c["gray"]) == -1).all() and (h["gray"] == -1).all()
        on = c["jitter"][0].order[0] != 255
        assert on == (D.SLOT_FRAME + 2 in src.calls) and D.SLOT_JITTER_P in src.calls and D.SLOT_FLIP in src.calls
        seen["jitter"] += int(on)
        seen["center"] += int(not c["sized_crop"])
        if c["sized_crop"]:
            fb = D.SLOT_ATTEMPT + 5 * 9 + 2 in src.calls and D.SLOT_ATTEMPT + 5 * 9 + 3 not in src.calls
            assert (fb or t % 7 != 0) and (not fb or (c["x1"] == 0 and c["y1"] == 0))
            seen["fallback" if fb else "accepted"] += 1
        widest = max(widest, c["xk"].shape[1], c["yk"].shape[1])
    assert widest <= D.resident_ks(recipe_of(mode), W0, H0, size, crop)
    print(f"{mode} {W0}x{H0} crop {crop} size {size}: {seen}, widest row {widest} taps")
    assert seen["fallback"] > 0 and seen["accepted"] > 0 and 0 < seen["jitter"] < rows
    assert (seen["center"] > 0) == (mode == "val")
    return seen


# ---- (2) the kernel == the host statement -------------------------------------------------------------------------------------------
def dense_offsets(n=len(LENGTHS)):
    return np.arange(n + 1, dtype=np.int64) * SLOT_F


def draw_ex(lib, dev, recipe, W0, H0, crop, size, vids, offsets, lengths=None, labels=None, seed=0, counter=0, uniforms=None):
    """dpc_draw_recipe_ex for the batch `vids` -> the tables as numpy (and `target`, pre-filled with junk, when labels are given)"""
    B, KS = len(vids), D.resident_ks(recipe, W0, H0, size, crop)
    t = rc.Tables(dev, B, size, KS, N_FR)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    desc = D.recipe_desc(recipe)
    scaled = desc.sized_p < 0 or bool(desc.flags & L.RECIPE_SCALE_AFTER_SIZED)
    tab = dv(D.nearest_tables(crop, size)) if scaled and crop != size else None
    un = None if uniforms is None else dv(np.asarray(uniforms, np.float32))
    ctr = torch.tensor([counter], dtype=torch.int32, device=dev)
    target = torch.full((B,), -0x5A5A5A, dtype=torch.int64, device=dev) if labels is not None else None
    lib.call("dpc_draw_recipe_ex", C.byref(desc), dv(np.asarray(vids, np.int32)), None, dv(offsets), None if lengths is None else dv(lengths),
             None if labels is None else dv(labels), B, W0, H0, crop, size, N, SL, DS, KS, tab, seed, ctr, un, t.aug, t.clip_first, t.gray,
             t.jitter, t.xb, t.xk, t.yb, t.yk, target, lib.stream())
    rc._sync(dev)
    out = t.host()
    if target is not None:
        out["target"] = target.cpu().numpy()
    return out


def expect_ex(recipe, uniforms, W0, H0, crop, size, vids, offsets, lengths=None, labels=None):
    """the same tables from data.recipe_from_uniforms, packed the way data.recipe_to_input packs them; also the per-clip dicts"""
    B, KS = len(vids), D.resident_ks(recipe, W0, H0, size, crop)
    out = dict(aug=np.zeros((B, 4), np.int32), clip_first=np.zeros(B, np.int64), gray=np.zeros((B, N_FR), np.int8),
               jitter=np.zeros(B * N_FR * C.sizeof(D.FrameJitter), np.uint8), xb=np.zeros((B, size, 2), np.int32),
               yb=np.zeros((B, size, 2), np.int32), xk=np.zeros((B, size, KS), np.int32), yk=np.zeros((B, size, KS), np.int32))
    clips = []
    for b, v in enumerate(vids):
        vlen = int(lengths[v]) if lengths is not None else int(offsets[v + 1] - offsets[v])
        c = D.recipe_from_uniforms(recipe, uniforms[b], vlen, W0, H0, crop, size, N_FR, SPAN)
        clips.append(c)
        out["aug"][b] = (c["start"], c["x1"], c["y1"], c["flip"])
        out["clip_first"][b] = offsets[v]
        out["gray"][b] = c["gray"]
        out["jitter"].reshape(B, -1)[b] = np.frombuffer(bytes(c["jitter"]), np.uint8)
        out["xb"][b], out["yb"][b] = c["xb"], c["yb"]
        assert c["xk"].shape[1] <= KS and c["yk"].shape[1] <= KS, "the documented pitch is too small for this row"
        out["xk"][b, :, :c["xk"].shape[1]] = c["xk"]
        out["yk"][b, :, :c["yk"].shape[1]] = c["yk"]
    if labels is not None:
        out["target"] = np.asarray(labels, np.int64)[np.asarray(vids)]
    return out, clips


def check_lc_branches(mode, u, clips, W0, H0, crop, size, taken):
    """the rows did take the branches they were built for (read off the HOST recipes)"""
    r = recipe_of(mode)
    idx = D.nearest_tables(crop, size) if crop != size else np.arange(size)
    assert {c["flip"] for c in clips} == {0, 1}
    assert clips[5]["start"] == LENGTHS[1] - SPAN - 1 == 0 and clips[6]["start"] == LENGTHS[4] - SPAN - 1 and clips[1]["start"] == 0
    assert "jitter skipped" in taken and all(j.order[0] == 255 for j in clips[7]["jitter"]) and clips[0]["jitter"][0].order[0] != 255
    for c in clips:                                       # consistent=True: every frame carries frame 0's draw
        assert all(bytes(j) == bytes(c["jitter"][0]) for j in c["jitter"])
    hue = [c["jitter"][0].hue_shift for c in clips if c["jitter"][0].order[0] != 255]
    assert any(h >= 128 for h in hue) and any(0 < h < 128 for h in hue), "hue shifts of both signs"
    assert sorted(clips[0]["jitter"][0].order) == [0, 1, 2, 3] and list(clips[0]["jitter"][0].order) == [0, 1, 2, 3]   # frame 0: every step keeps its element
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in ("xb", "xk", "yb", "yk")) and (a["x1"], a["y1"]) == (b["x1"], b["y1"])  # noqa: E731
    again = lambda b, **slots: D.recipe_from_uniforms(r, _with(u[b], slots), 20, W0, H0, crop, size, N_FR, SPAN)   # noqa: E731
    a0 = D.SLOT_ATTEMPT
    # row 0: decided by attempt 0 alone; row 1: only because of the swap; row 2: attempt 0 is rejected, attempt 1 decides
    assert same(clips[0], again(0, **{str(a0 + 5): 0.5, str(a0 + 6): 0.5}))
    assert not same(clips[1], again(1, **{str(a0 + 2): 0.75}))
    assert same(clips[2], again(2, **{str(a0 + 3): 0.5, str(a0 + 4): 0.5})) and not same(clips[2], again(2, **{str(a0 + 5): 0.99}))
    # row 3: all ten rejected -- Scale + CenterCrop of the whole frame at `crop`, then the NEAREST rows
    ow, oh = (crop, int(crop * H0 / W0)) if W0 < H0 else (int(crop * W0 / H0), crop)
    fx, fy = D.resample_tables(W0, ow, int(round((ow - crop) / 2.)), crop), D.resample_tables(H0, oh, int(round((oh - crop) / 2.)), crop)
    assert clips[3]["x1"] == 0 and clips[3]["y1"] == 0 and np.array_equal(clips[3]["xb"], fx[0][idx]) and np.array_equal(clips[3]["yk"], fy[1][idx])
    # row 4: randint at the top of its range -- the last row of the `crop` table touches the right edge when the Scale keeps it
    assert again(4, **{str(a0 + 3): 0.0, str(a0 + 4): 0.0})["x1"] == 0
    reach = clips[4]["x1"] + int((clips[4]["xb"][:, 0] + clips[4]["xb"][:, 1]).max())
    assert reach <= W0 and (reach == W0 or idx[-1] != crop - 1)
    if r["sized_p"] < 1:
        assert "CenterCrop" in taken and clips[6]["x1"] == int(round((W0 - crop) / 2.)) and clips[6]["y1"] == int(round((H0 - crop) / 2.))
        assert np.array_equal(clips[6]["xb"][:, 0], idx) and (clips[6]["xb"][:, 1] == 1).all() and (clips[6]["xk"][:, 0] == 1 << D.RS_PREC).all()
    if crop != size:
        assert not np.array_equal(idx, np.arange(size)), "the Scale is not the identity"


def _with(row, slots):
    row = np.array(row, np.float64)
    for s, v in slots.items():
        row[int(s)] = v
    return row


def draw_injected_case(lib, dev, mode, W0, H0, crop, size):
    """injected uniforms, a dense store with `lengths`, the labels gathered by the same launch"""
    recipe = recipe_of(mode)
    u, vids, taken = rc.injected_uniforms(recipe, W0, H0)
    off, lengths = dense_offsets(), np.asarray(LENGTHS, np.int64)
    want, clips = expect_ex(recipe, u, W0, H0, crop, size, vids, off, lengths, LABELS)
    check_lc_branches(mode, u, clips, W0, H0, crop, size, taken)
    got = draw_ex(lib, dev, recipe, W0, H0, crop, size, vids, off, lengths, LABELS, seed=99, counter=3, uniforms=u)
    rc.assert_tables_equal(got, want, f"{mode} {W0}x{H0}")
    # the label gather: duplicates in the batch, every junk word overwritten
    assert len(set(vids)) < len(vids) and np.array_equal(got["target"], LABELS[vids])
    # consistent=True in the kernel's bytes, and the slots of frames >= 1 are unused
    jit = got["jitter"].reshape(len(vids), N_FR, -1)
    assert (jit == jit[:, :1]).all()
    v = u.copy()
    v[:, D.SLOT_FRAME + D.FRAME_SLOTS:] = np.random.Generator(np.random.PCG64(3)).integers(0, 1 << 24, v[:, D.SLOT_FRAME + D.FRAME_SLOTS:].shape) * 2.0 ** -24
    assert not np.array_equal(u, v)
    rc.assert_tables_equal(draw_ex(lib, dev, recipe, W0, H0, crop, size, vids, off, lengths, LABELS, seed=99, counter=3, uniforms=v), got,
                           "slots of frames >= 1")
    # `lengths`: the top start is lengths[v] - span - 1, and no start leaves the video although every slot has slack behind it
    top = u.copy()
    top[:, D.SLOT_START] = TOP
    t = draw_ex(lib, dev, recipe, W0, H0, crop, size, vids, off, lengths, uniforms=top)
    assert np.array_equal(t["aug"][:, 0], lengths[vids] - SPAN - 1) and (lengths < SLOT_F).all() and "target" not in t
    assert np.array_equal(t["clip_first"], off[vids])
    # without `lengths` the same rows start where the SLOT ends
    t = draw_ex(lib, dev, recipe, W0, H0, crop, size, vids, off, uniforms=top)
    assert (t["aug"][:, 0] == SLOT_F - SPAN - 1).all()
    return int(max(want["xb"][..., 1].max(), want["yb"][..., 1].max()))


def additions_off_case(lib, dev, name):
    """flags = 0 and no table: the new entry writes what dpc_draw_recipe writes, on the shapes of tests/resident_cases.py"""
    _, recipe, W0, H0, crop, size = next(s for s in rc.DRAW_SHAPES if s[0] == name)
    u, vids, _ = rc.injected_uniforms(recipe, W0, H0)
    off = rc.offsets_of(LENGTHS)
    assert D.recipe_desc(recipe).flags == 0
    old = rc.draw(lib, dev, recipe, W0, H0, crop, size, vids, off, seed=99, counter=3, uniforms=u)
    new = draw_ex(lib, dev, recipe, W0, H0, crop, size, vids, off, seed=99, counter=3, uniforms=u)
    rc.assert_tables_equal(new, old, name)
    rc.assert_tables_equal(draw_ex(lib, dev, recipe, W0, H0, crop, size, vids, off, seed=5, counter=2),
                           rc.draw(lib, dev, recipe, W0, H0, crop, size, vids, off, seed=5, counter=2), name + " philox")


def old_entry_ignores_flags_case(lib, dev):
    """dpc_draw_recipe keeps its bits whatever the descriptor's last word holds (it was `reserved`)"""
    W0, H0, crop, size = 40, 30, 16, 16
    u, vids, _ = rc.injected_uniforms(rc.LCISH, W0, H0)
    off = rc.offsets_of(LENGTHS)
    plain = rc.draw(lib, dev, rc.LCISH, W0, H0, crop, size, vids, off, uniforms=u)
    flagged = rc.draw(lib, dev, dict(rc.LCISH, jitter_consistent=True), W0, H0, crop, size, vids, off, uniforms=u)
    rc.assert_tables_equal(flagged, plain, "dpc_draw_recipe with a flag set")
    # ... and the new entry does read it
    assert not np.array_equal(draw_ex(lib, dev, dict(rc.LCISH, jitter_consistent=True), W0, H0, crop, size, vids, off, uniforms=u)["jitter"], plain["jitter"])


def philox_case(lib, dev):
    off, lengths, vids = dense_offsets(), np.asarray(LENGTHS, np.int64), [2, 2, 0, 4]
    seed, ctr = (7 << 32) | 12345, 17
    u = np.stack([rc.philox_uniforms(seed, ctr, b) for b in range(len(vids))])
    for mode, (W0, H0, crop, size) in (("train", LC_SHAPES[0]), ("val", LC_SHAPES[3])):
        got = draw_ex(lib, dev, recipe_of(mode), W0, H0, crop, size, vids, off, lengths, LABELS, seed=seed, counter=ctr)
        want, _ = expect_ex(recipe_of(mode), u, W0, H0, crop, size, vids, off, lengths, LABELS)
        rc.assert_tables_equal(got, want, "philox " + mode)
        assert any(not np.array_equal(got[k][0], got[k][1]) for k in ("xb", "xk", "yb", "yk")), "clips 0 and 1 read the same video"
        other = draw_ex(lib, dev, recipe_of(mode), W0, H0, crop, size, vids, off, lengths, LABELS, seed=seed, counter=ctr + 1)
        assert any(not np.array_equal(got[k], other[k]) for k in ("aug", "xb", "xk")), "the next counter"


# ---- (3) the distribution -----------------------------------------------------------------------------------------------------------
P_BOUND = 4 * math.sqrt(0.3 * 0.7 / rc.DIST_CLIPS)        # 0.029: the jitter's p and the val recipe's sized-crop p, both 0.3
DW0, DH0, DCROP, DSIZE = 40, 30, 4, 4                      # every accepted box is wider than 4: a sized crop has rows of more than one tap


def _dist_check(what, on, flip, start):
    print(f"{what}: share {on:.4f} vs 0.3 (bound {P_BOUND:.4f}), flip share {flip:.4f} (bound {rc.FLIP_BOUND:.4f}), "
          f"mean start / range {start:.4f} (bound {rc.START_BOUND:.4f})")
    assert abs(on - 0.3) <= P_BOUND and abs(flip - 0.5) <= rc.FLIP_BOUND and abs(start - 0.5) <= rc.START_BOUND


def dist_host_case():
    """the host statement over numpy uniforms stays inside the bounds for the chosen seed"""
    rng = np.random.Generator(np.random.PCG64(rc.DIST_SEED))
    u = rng.integers(0, 1 << 24, (rc.DIST_CLIPS, D.recipe_slots(N_FR))).astype(np.float64) * 2.0 ** -24
    vids, L_ = rc.dist_vids(), np.asarray(rc.DIST_LENGTHS)
    for mode in ("train", "val"):
        cs = [D.recipe_from_uniforms(recipe_of(mode), u[i], int(L_[vids[i]]), DW0, DH0, DCROP, DSIZE, N_FR, SPAN) for i in range(rc.DIST_CLIPS)]
        on = np.mean([c["jitter"][0].order[0] != 255 for c in cs]) if mode == "train" else np.mean([c["xb"][:, 1].max() > 1 for c in cs])
        _dist_check("host " + mode, float(on), float(np.mean([c["flip"] != 0 for c in cs])),
                    float(np.mean(np.array([c["start"] for c in cs]) / (L_ - SPAN)[vids])))


def dist_kernel_case(lib, dev):
    """4 096 clips per recipe: the jitter-on share (train) and the sized-crop share (val) against 0.3, the flip, the start"""
    vids, L_, off = rc.dist_vids(), np.asarray(rc.DIST_LENGTHS), rc.offsets_of(rc.DIST_LENGTHS)
    for mode in ("train", "val"):
        parts = [draw_ex(lib, dev, recipe_of(mode), DW0, DH0, DCROP, DSIZE, vids[i:i + rc.DIST_B], off, seed=rc.DIST_SEED + (mode == "val"),
                         counter=1 + i // rc.DIST_B) for i in range(0, rc.DIST_CLIPS, rc.DIST_B)]
        t = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        for i in range(0, rc.DIST_CLIPS, 7):
            rc.validate_clip(int(t["aug"][i, 0]), int(t["aug"][i, 1]), int(t["aug"][i, 2]), t["xb"][i], t["yb"][i], int(L_[vids[i]]), DW0, DH0)
        jit = t["jitter"].reshape(rc.DIST_CLIPS, N_FR, C.sizeof(D.FrameJitter))
        on = (jit[:, 0, 16] != 255).mean() if mode == "train" else (t["xb"][:, :, 1].max(1) > 1).mean()   # byte 16: order[0]
        _dist_check("kernel " + mode, float(on), float((t["aug"][:, 3] != 0).mean()), float((t["aug"][:, 0] / (L_ - SPAN)[vids]).mean()))


# ---- (4) what the entry point refuses -----------------------------------------------------------------------------------------------
def draw_rejects_case(lib, dev):
    fn = lib._fn("dpc_draw_recipe_ex")
    t = rc.Tables(dev, 2, 8, 7)
    z = torch.zeros(8, dtype=torch.int64, device=dev)
    tab8, tab16 = (torch.from_numpy(D.nearest_tables(16, s) if s != 16 else np.arange(16, dtype=np.int32)).to(dev) for s in (8, 16))
    p = lambda x: None if x is None else x.data_ptr()   # noqa: E731
    train, val = recipe_of("train"), recipe_of("val")

    def call(recipe, W0=40, H0=30, crop=16, size=8, KS=7, tab=tab8, labels=None, target=None, flags=None):
        d = D.recipe_desc(recipe)
        if flags is not None:
            d.flags = flags
        return fn(C.byref(d), p(z), None, p(z), None, p(labels), 2, W0, H0, crop, size, N, SL, DS, KS, p(tab), 1, p(z), None, p(t.aug),
                  p(t.clip_first), p(t.gray), p(t.jitter), p(t.xb), p(t.xk), p(t.yb), p(t.yk), p(target), None)

    before = t.host()
    assert call(train, flags=4) == L.ERR_ARG and call(train, flags=3 | 8) == L.ERR_ARG and call(train, flags=-1) == L.ERR_ARG   # undefined bits
    assert call(dict(D.RECIPES["ucf101"], scale_after_sized=True), crop=16) == L.ERR_ARG          # the flag needs sized_p >= 0
    assert call(train, KS=6) == L.ERR_ARG and call(train, W0=49) == L.ERR_ARG                     # 2 ceil(40 / 16) + 1 = 7, 2 ceil(49 / 16) + 1 = 9
    assert call(train, tab=None) == L.ERR_ARG                                                     # crop != size: the Scale needs its table
    assert call(train, size=16, tab=tab16) == L.ERR_ARG                                           # crop == size: there is no Scale
    assert call(train, crop=0) == L.ERR_ARG
    assert call(train, labels=z) == L.ERR_ARG and call(train, target=z) == L.ERR_ARG              # labels and target come together
    assert call(train, crop=2048) == L.ERR_UNSUPPORTED and call(train, crop=1025) == L.ERR_UNSUPPORTED   # crop <= 1024, as size
    assert call(val, W0=20, H0=14, KS=5) == L.ERR_UNSUPPORTED and call(val, W0=14, H0=20, KS=5) == L.ERR_UNSUPPORTED   # CenterCrop(16) leaves the frame
    rc.assert_tables_equal(t.host(), before, "a rejected call wrote")
    assert not z.any()
    # the same shapes are fine for the train recipe (p = 1: no CenterCrop), and the size rule follows `crop`, not `size`
    t5 = rc.Tables(dev, 2, 8, 5)
    d = D.recipe_desc(train)
    z[:2] = torch.tensor([0, 40])
    assert fn(C.byref(d), p(z[2:]), None, p(z), None, None, 2, 20, 14, 16, 8, N, SL, DS, 5, p(tab8), 1, p(z[2:]), None, p(t5.aug), p(t5.clip_first),
              p(t5.gray), p(t5.jitter), p(t5.xb), p(t5.xk), p(t5.yb), p(t5.yk), None, None) == 0
    rc._sync(dev)


# ---- (5) the engine -----------------------------------------------------------------------------------------------------------------
E_SIZE, E_W0, E_H0, E_CROP, E_N, E_SL, E_DS, E_F, E_CLASSES = 64, 80, 60, 48, 2, 2, 3, 18, 101
E_LENGTHS = (18, 13, 16, 15, 12)                      # span 12: video 4 is too short and dropped; the others leave 1 .. 6 starts
E_LABELS = (5, 17, 5, 99, 42)
E_SEED = 28                                           # low key word of both sources: the Philox words of the batches below take both
                                                      # jitter branches under `train` and both crop branches under `val` (asserted)


def lc_store_arrays(seed=9, copies=1):
    """copies > 1: the five videos again with other noise (4 usable videos and a short one per copy)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = rng.integers(0, 256, (1, 1, E_H0 // 4, E_W0 // 4, 3), dtype=np.uint8).repeat(4, 2).repeat(4, 3)
    frames = (base.astype(np.int16) + rng.integers(-40, 41, (copies * len(E_LENGTHS), E_F, E_H0, E_W0, 3))).clip(0, 255).astype(np.uint8)
    return frames, np.asarray(E_LENGTHS * copies, np.int64), np.asarray(E_LABELS * copies, np.int64)


def lc_sources(dev, B, store=None, rank=0, world=1):
    frames, lengths, labels = lc_store_arrays()
    st = store or D.FrameStore(frames, None, lengths).to_device(dev)
    mk = lambda recipe, role: D.ResidentLabelledSource(st, labels, "ucf101", E_N, E_SL, E_DS, E_SIZE, B, E_CLASSES, dev, recipe, rank, world,  # noqa: E731
                                                       E_CROP, seed=(role << 32) | E_SEED)
    return mk("train", 0), mk("val", 1)


def lc_engine(lib, dev, dtype, widths, B):
    import lc_graph_cases as lg
    return lg.lc_engine(lib, dev, dtype, widths, B, E_SIZE, E_N, E_SL, E_CLASSES)


def host_batch(src, mine_row, counter):
    """what load_resident draws for one batch, from the documented Philox words: (spans u8 [B, span, H0, W0, 3], clips, labels)"""
    st = src.store
    span = (src.n_fr - 1) * src.ds + 1
    clips, spans = [], []
    for b, v in enumerate(mine_row):
        u = rc.philox_uniforms(src.seed, counter, b, src.n_fr)
        c = D.recipe_from_uniforms(recipe_of(src.recipe), u, int(st.lengths[v]), st.W0, st.H0, src.crop, src.size, src.n_fr, src.n_fr * src.ds)
        assert c["start"] + span <= int(st.lengths[v])
        clips.append(c)
        spans.append(np.asarray(st.frames[st.offsets[v] + c["start"]: st.offsets[v] + c["start"] + span]))
    return np.stack(spans), clips, torch.from_numpy(src.labels[np.asarray(mine_row)])


def counted(eng):
    """record the C entries the engine calls from here on"""
    names, real = [], eng.call
    eng.call = lambda name, *a, **k: names.append(name) or real(name, *a, **k)
    return names


def engine_case(lib, dev, dtype, widths=None, B=2, train=True):
    """load_resident(labelled source) == load_recipe fed hand-cut spans + recipe_from_uniforms(the documented Philox words) +
    set_labels: operand bits and target, and (train=True) the results of two train steps and one eval step and the state after them.
    train=False (the simulator tier, f32 only: a simulated full train step takes the better part of a minute, as in
    resident_cases.engine_case): operand bits and target only -- the train steps, the eval step and bf16 run on the MI355X tier, and
    entry_by_hand_case runs train and eval steps through load_resident on the simulator"""
    a, b = lc_engine(lib, dev, dtype, widths, B), lc_engine(lib, dev, dtype, widths, B)
    tr, va = lc_sources(dev, B)
    assert tr.store is va.store and tr.skipped == 1 and tr.keep.tolist() == [0, 1, 2, 3] and len(tr) == 4 // B
    assert tr.KS == 2 * -(-E_W0 // E_CROP) + 1 and tr.desc.flags == 3 and tr.desc.sized_p == 1.0 and va.desc.sized_p == 0.3 and va.desc.jitter_p == 0.3
    a.target.fill_(-7)
    names = counted(a)
    seen = {"train": [], "val": []}
    for src, steps, is_train in ((tr, 2 if B == 2 else 1, True), (va, 1, False)):
        mine = src.begin_epoch()
        assert len(set(mine.reshape(-1).tolist())) == mine.size and set(mine.reshape(-1).tolist()) <= {0, 1, 2, 3}
        for i in range(steps):
            del names[:]
            a.load_resident(src)
            assert names == ["dpc_counter_advance", "dpc_counter_advance", "dpc_draw_recipe_ex", "dpc_store_to_input"], names
            spans, clips, y = host_batch(src, mine[i], i + 1)
            seen[src.recipe] += [(c["jitter"][0].order[0] != 255, c["xb"][:, 1].max() > 1) for c in clips]
            b.load_recipe(torch.from_numpy(spans).to(dev), [0] * B, clips, ds=src.ds)
            b.set_labels(y)
            rc._sync(dev)
            assert rc.same_bits(a.x_s2d.cpu(), b.x_s2d.cpu()), f"{src.recipe} step {i}: the stem's operand differs"
            assert torch.equal(a.target.cpu(), y) and bool(torch.isfinite(a.x_s2d.float()).all())
            if i == 0 and is_train:
                ptrs = (a._resident_ws, a.target.data_ptr(), a.x_s2d.data_ptr(), src.aug.data_ptr(), src.jitter.data_ptr())
            if train and is_train:
                ra, rb = a.train_step(None, None).clone(), b.train_step(None, None).clone()
            elif train:
                a.forward(None, None, train=False)
                b.forward(None, None, train=False)
                ra, rb = a.result.clone(), b.result.clone()
                assert torch.equal(a.logits, b.logits)
            if train:
                rc._sync(dev)
                assert torch.equal(ra, rb) and bool(torch.isfinite(ra).all()), (src.recipe, i, ra, rb)
        assert int(src.cursor.item()) == steps and int(src.draw.item()) == steps
    assert ptrs[0] is a._resident_ws and ptrs[0] is not None and ptrs[1:] == (a.target.data_ptr(), a.x_s2d.data_ptr(), tr.aug.data_ptr(),
                                                                             tr.jitter.data_ptr()), "allocated once, no address changes"
    assert {j for j, _ in seen["train"]} == {True, False}, "the train batches take both jitter branches"
    assert {s for _, s in seen["val"]} == {True, False} and all(s for _, s in seen["train"]), "the val batch takes the sized crop and the CenterCrop"
    if train:
        assert torch.equal(a.flat_p, b.flat_p) and torch.equal(a.flat_m, b.flat_m) and a.step_count == b.step_count == 2
    # a source with labels needs an engine that can receive them
    del b.target
    try:
        b.load_resident(tr)
    except ValueError as e:
        assert "no `target`" in str(e)
    else:
        raise AssertionError("an engine without `target` accepted a labelled source")


def graph_case(dev, dtype, B=2):
    """a captured train step and a captured eval step, each with its resident refill, replayed interleaved over two epochs (with
    begin_epoch in between: a new permutation uploaded, the cursor zeroed) == an eager twin at every step; ONE capture of each serves both"""
    a, b = lc_engine(None, dev, dtype, None, B), lc_engine(None, dev, dtype, None, B)
    (at, av), (bt, bv) = lc_sources(dev, B), lc_sources(dev, B)
    orders = []

    def begin(src, k):   # ResidentLabelledSource.begin_epoch itself; the same seed in front of both twins gives both the same permutation
        torch.manual_seed(1100 + k)
        return src.begin_epoch().reshape(-1).tolist()

    def eager(eng, src, train):
        eng.load_resident(src)
        if train:
            return eng.train_step(None, None).clone()
        eng.forward(None, None, train=False)
        return eng.result.clone()

    rt, rv = (lambda: b.load_resident(bt)), (lambda: b.load_resident(bv))
    tr = ev = None
    seen = []
    for e in range(3):
        for train, sa, sb in ((True, at, bt), (False, av, bv)):
            orders.append(begin(sa, 2 * e + (not train)))
            assert begin(sb, 2 * e + (not train)) == orders[-1] and sorted(orders[-1]) == [0, 1, 2, 3]
            for _ in range(2):
                ra = eager(a, sa, train)
                if e == 0:                      # epoch 0 eagerly (the warm-up of the entry) ...
                    rb = eager(b, sb, train)
                else:                           # ... epochs 1 and 2 replayed
                    rb = (tr if train else ev)().clone()
                torch.cuda.synchronize()
                assert torch.equal(ra, rb) and torch.equal(a.target, b.target), (e, train, ra, rb)
                seen.append(tuple(ra.tolist()))
        if e == 0:
            tr, ev = b.capture_train_step(None, warmup=0, refill=rt), b.capture_eval_step(rv)
            kernels = (list(tr.kernels), list(ev.kernels))
    assert b.capture_train_step(None, warmup=0, refill=rt) is tr and b.capture_eval_step(rv) is ev
    assert (list(tr.kernels), list(ev.kernels)) == kernels and all(kernels[0]) and all(kernels[1])
    assert len({tuple(o) for o in orders}) > 1, "the epochs did not all see the same order"
    assert int(bt.draw.item()) == 6 and int(bv.draw.item()) == 6 and int(bt.cursor.item()) == 2 and a.step_count == b.step_count == 6
    assert torch.equal(a.flat_p, b.flat_p) and torch.equal(a.flat_m, b.flat_m) and len(set(seen)) == len(seen)
    for k in b.BUF:
        assert torch.equal(a.BUF[k], b.BUF[k]), k


# ---- (6) the entry ------------------------------------------------------------------------------------------------------------------
def entry_files(tmp, copies=1):
    frames, lengths, labels = lc_store_arrays(copies=copies)
    paths = [os.path.join(tmp, n) for n in ("videos.npy", "labels.npy", "lengths.npy")]
    for p, a in zip(paths, (frames, labels, lengths)):
        np.save(p, a)
    return paths


def entry_argv(fp, lp, np_, B, dtype, extra=()):
    return ["--net", "resnet18", "--img_dim", str(E_SIZE), "--batch_size", str(B), "--gpu", "0", "--print_freq", "1", "--dtype", dtype,
            "--num_seq", str(E_N), "--seq_len", str(E_SL), "--ds", str(E_DS), "--dataset", "ucf101", "--crop", str(E_CROP),
            "--frames", fp, "--labels", lp, "--lengths", np_] + list(extra)


def run_entry(tmp, name, argv, **kw):
    from dpc_amd import lc_main
    pr = os.path.join(tmp, name)
    os.makedirs(pr)
    lc_main.main(argv, _probe=pr, **kw)
    return pr


def loss_lines(out):
    return [ln for ln in out.splitlines() if "Loss" in ln]


def entry_by_hand_case(lib, dev, tmp, cap, dtype, widths, B, train_what, epochs=1, **kw):
    """`lc_main --frames --labels --lengths --resident` == the loop it documents on a twin engine: torch.manual_seed(0), per epoch
    begin_epoch + load_resident + train_step for the train source, the same with the eval-mode forward for the val source"""
    fp, lp, np_ = entry_files(tmp)
    cap.readouterr()
    pr = run_entry(tmp, "probe", entry_argv(fp, lp, np_, B, dtype, ["--epochs", str(epochs), "--train_what", train_what, "--resident"]), **kw)
    out = cap.readouterr().out
    got = torch.load(os.path.join(pr, "rank0.pt"))
    steps = 4 // B
    assert "1 training / 1 validation videos skipped" in out and got["step"] == epochs * steps
    lines = loss_lines(out)
    assert len(lines) == epochs * (steps + 1), out
    eng = lc_engine(lib, dev, torch.bfloat16 if dtype == "bf16" else torch.float32, widths, B)
    if train_what == "head":
        eng.set_param_groups([{"params": [k for k in eng.offsets if k.startswith(("final_bn.", "final_fc."))], "lr": 1e-3, "weight_decay": 1e-3}])
    st = D.FrameStore(fp, None, np_).to_device(dev)
    tr, va = (D.ResidentLabelledSource(st, lp, "ucf101", E_N, E_SL, E_DS, E_SIZE, B, E_CLASSES, dev, r, crop=E_CROP, seed=role << 32)
              for role, r in enumerate(("train", "val")))
    torch.manual_seed(0)
    want = []
    for _ in range(epochs):
        tr.begin_epoch()
        for _ in range(steps):
            eng.load_resident(tr)
            want.append(eng.train_step(None, None).clone().cpu().tolist())
        va.begin_epoch()
        vl = va_ = 0.0
        for _ in range(steps):
            eng.load_resident(va)
            eng.forward(None, None, train=False)
            loss, acc = eng.result.cpu().tolist()
            vl, va_ = vl + loss, va_ + acc
        want.append((vl / steps, va_ / steps))
    rc._sync(dev)
    assert torch.equal(got["flat_p"], eng.flat_p.cpu()) and torch.equal(got["flat_m"], eng.flat_m.cpu()) and got["flat_m"].abs().sum() > 0
    for ln, (loss, acc) in zip(lines, want):
        assert "Loss {:.4f}\t Acc: {:.4f}".format(loss, acc) in ln, (ln, loss, acc)
    return got


def entry_graph_case(tmp, capfd, train_what, B=2):
    """--resident vs --resident --graph over epochs 60 and 61 of the ucf101 / 64 px schedule, four train steps each (eight usable
    videos, B = 2).  Epoch 60 runs at lr: two eager warm-up steps, then the first captured train step replays twice.  Epoch 61 runs
    at lr / 10: set_lr dropped the handles, so the entry captures a SECOND train step with the SAME resident refill (the first stays
    parked) and replays it four times.  Parameters, moments and log lines must be bit-identical to the eager run"""
    import re
    fp, lp, np_ = entry_files(tmp, copies=2)
    argv = entry_argv(fp, lp, np_, B, "bf16", ["--start-epoch", "60", "--epochs", "62", "--train_what", train_what, "--resident"])
    runs = {}
    for mode in ("eager", "graph"):
        pr = run_entry(tmp, mode, argv + (["--graph"] if mode == "graph" else []))
        out = capfd.readouterr().out
        runs[mode] = (torch.load(os.path.join(pr, "rank0.pt")), loss_lines(out), re.findall(r"Graph replay: (\d+) steps", out), out)
    (pe, le, ge, oe), (pg, lg_, gg, og) = runs["eager"], runs["graph"]
    steps = 8 // B
    assert steps == 4 and pe["step"] == pg["step"] == 2 * steps and pe["flat_m"].abs().sum() > 0
    assert torch.equal(pe["flat_p"], pg["flat_p"]) and torch.equal(pe["flat_m"], pg["flat_m"])
    assert le == lg_ and len(le) == 2 * (steps + 1), (le, lg_)
    assert ge == [] and [int(n) for n in gg] == [steps - 2, steps], og   # a capture at lr, replayed twice; a second one at lr / 10
    for o in (oe, og):
        assert o.count("lr 0.001\n") == steps and o.count("lr 0.0001\n") == steps and "2 training / 2 validation videos skipped" in o


def protocol_case(tmp, cap, graph=False, **kw):
    """--test and --retrieval (with a gallery) with --resident == the same runs without it: totals, confusion matrix and every
    array of the retrieval record.  The same launches on the same bytes -- the video is a slice of the store instead of an upload"""
    fp, lp, np_ = entry_files(tmp)
    frames, lengths, labels = lc_store_arrays()
    gp, glp, gnp = (os.path.join(tmp, n) for n in ("gallery.npy", "glabels.npy", "glengths.npy"))
    np.save(gp, frames[::-1][:, :, ::-1].copy())
    np.save(glp, labels[::-1].copy())
    np.save(gnp, lengths[::-1].copy())
    extra = ["--graph"] if graph else []
    base = entry_argv(fp, lp, np_, 2, "f32", extra)
    res = {}
    for mode, more in (("plain", []), ("resident", ["--resident"])):
        pr = run_entry(tmp, "test_" + mode, base + ["--test", "random"] + more, **kw)
        out = cap.readouterr().out
        assert "4 videos tested, 1 skipped" in out, out
        t = torch.load(os.path.join(pr, "rank0.pt"))
        pr = run_entry(tmp, "retr_" + mode, base + ["--retrieval", "random", "--retrieval_k", "1,2", "--gallery_frames", gp, "--gallery_labels", glp,
                                                    "--gallery_lengths", gnp] + more, **kw)
        out = cap.readouterr().out
        assert "(4 queries, 4 gallery videos, cross, bn running)" in out and "2 videos skipped" in out, out
        res[mode] = (t, dict(np.load(os.path.join(pr, "retrieval.npz"))), [ln for ln in out.splitlines() if ln.startswith("R@")])
    (tp, rp, lp_), (tr_, rr, lr_) = res["plain"], res["resident"]
    assert tp["totals"] == tr_["totals"] and tp["totals"][3] == 4.0 and torch.equal(tp["confusion"], tr_["confusion"]) and tp["skipped"] == tr_["skipped"] == 1
    assert int(tp["confusion"].sum()) == 4 and math.isfinite(tp["totals"][0])
    assert set(rp) == set(rr) and lp_ == lr_
    for k in rp:
        assert rp[k].dtype == rr[k].dtype and np.array_equal(rp[k], rr[k]), k
    assert np.isfinite(rp["query_emb"]).all() and abs(float(np.linalg.norm(rp["query_emb"][0])) - 1.0) < 1e-5
