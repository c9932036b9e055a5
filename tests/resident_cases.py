"""Case bodies of the resident-frames tests (`python -m dpc_amd.main --frames ... --resident`), shared by the simulator tier
(tests/test_resident_emu.py) and the MI355X tier (tests/test_resident_gpu.py): csrc/recipe_draw.hip and dpc_store_to_input through
the C ABI, data.FrameStore / ResidentFrameSource, BackboneEngine.load_resident.

Expectations never come from the code under test: the draw kernel is held, bit for bit, to data.recipe_from_uniforms (the host
statement of the same decisions, built on the resample_tables that tests/golden/aug.npz pins to PIL) fed with the injected uniforms
or with kcases.philox4x32_10_np words; the gather is held to dpc_frames_to_input_ex on spans cut out of the store by hand; the
distribution bounds are 4 standard errors of the exact law (Bernoulli(1/2): sqrt(0.25 / n); uniform: sqrt(1 / (12 n)))."""
import ctypes as C
import math

import numpy as np
import torch

from dpc_amd import _lib as L
from dpc_amd import data as D
from kcases import philox4x32_10_np

N, SL, DS = 2, 3, 2
N_FR, SPAN = N * SL, N * SL * DS          # 6 frames per clip; a video needs more than 12
TOP = 1.0 - 2.0 ** -24                    # the largest uniform there is
LENGTHS = (20, 13, 31, 15, 14)            # video 1 is the shortest legal one (one start), video 4 the last of the store
NOJIT = dict(sized_p=1.0, flip_code=1, gray_p=0.5, jitter=None)
LCISH = dict(sized_p=0.3, flip_code=1, gray_p=None, jitter=dict(brightness=0.2, contrast=0.2, saturation=0.2, hue=0.1, p=0.3))
# (name, recipe, W0, H0, crop, size): the five shapes of the issue, and the p < 1 branches (CenterCrop, jitter skipped) that the
# two pre-training recipes never take
DRAW_SHAPES = (("shrink", "k400", 40, 30, 16, 16), ("enlarge", "k400", 20, 14, 16, 16), ("tall", "k400", 14, 20, 16, 16),
               ("ucf_scale", "ucf101", 20, 14, 12, 8), ("ucf_plain", "ucf101", 20, 14, 8, 8), ("p_below_1", LCISH, 40, 30, 16, 16))


def _sync(dev):
    if str(dev) != "cpu":
        torch.cuda.synchronize()


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


class Tables:
    """the device tables of one batch, pre-filled with junk so that every byte the kernel owes is seen to be written"""

    def __init__(self, dev, B, size, KS, n_fr=N_FR):
        junk = lambda shape, dt: torch.full(shape, 0x5A, dtype=dt, device=dev)   # noqa: E731
        self.B, self.size, self.KS, self.n_fr = B, size, KS, n_fr
        self.aug, self.clip_first, self.gray = junk((B, 4), torch.int32), junk((B,), torch.int64), junk((B, n_fr), torch.int8)
        self.jitter = junk((B * n_fr * C.sizeof(D.FrameJitter),), torch.uint8)
        self.xb, self.yb = junk((B, size, 2), torch.int32), junk((B, size, 2), torch.int32)
        self.xk, self.yk = junk((B, size, KS), torch.int32), junk((B, size, KS), torch.int32)

    def host(self):
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("aug", "clip_first", "gray", "jitter", "xb", "yb", "xk", "yk")}


def draw(lib, dev, recipe, W0, H0, crop, size, vids, offsets, seed=0, counter=0, uniforms=None, n=N, sl=SL, ds=DS):
    """dpc_draw_recipe for the batch `vids` -> the tables as numpy"""
    B, KS = len(vids), D.resident_ks(recipe, W0, H0, size)
    t = Tables(dev, B, size, KS, n * sl)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    desc = D.recipe_desc(recipe)
    tab = dv(D.nearest_tables(crop, size)) if desc.sized_p < 0 and crop != size else None
    un = None if uniforms is None else dv(np.asarray(uniforms, np.float32))
    ctr = torch.tensor([counter], dtype=torch.int32, device=dev)
    lib.call("dpc_draw_recipe", C.byref(desc), dv(np.asarray(vids, np.int32)), None, dv(offsets), B, W0, H0, crop, size, n, sl, ds, KS, tab,
             seed, ctr, un, t.aug, t.clip_first, t.gray, t.jitter, t.xb, t.xk, t.yb, t.yk, lib.stream())
    _sync(dev)
    return t.host()


def expect(recipe, uniforms, W0, H0, crop, size, vids, offsets, n_fr=N_FR, span=SPAN):
    """the same tables from data.recipe_from_uniforms, packed the way data.recipe_to_input packs them; also the per-clip dicts"""
    B, KS = len(vids), D.resident_ks(recipe, W0, H0, size)
    out = dict(aug=np.zeros((B, 4), np.int32), clip_first=np.zeros(B, np.int64), gray=np.zeros((B, n_fr), np.int8),
               jitter=np.zeros(B * n_fr * C.sizeof(D.FrameJitter), np.uint8), xb=np.zeros((B, size, 2), np.int32),
               yb=np.zeros((B, size, 2), np.int32), xk=np.zeros((B, size, KS), np.int32), yk=np.zeros((B, size, KS), np.int32))
    clips = []
    for b, v in enumerate(vids):
        vlen = int(offsets[v + 1] - offsets[v])
        c = D.recipe_from_uniforms(recipe, uniforms[b], vlen, W0, H0, crop, size, n_fr, span)
        clips.append(c)
        out["aug"][b] = (c["start"], c["x1"], c["y1"], c["flip"])
        out["clip_first"][b] = offsets[v]
        out["gray"][b] = c["gray"]
        out["jitter"].reshape(B, -1)[b] = np.frombuffer(bytes(c["jitter"]), np.uint8)
        out["xb"][b], out["yb"][b] = c["xb"], c["yb"]
        assert c["xk"].shape[1] <= KS and c["yk"].shape[1] <= KS, "the documented pitch is too small for this row"
        out["xk"][b, :, :c["xk"].shape[1]] = c["xk"]
        out["yk"][b, :, :c["yk"].shape[1]] = c["yk"]
    return out, clips


def assert_tables_equal(got, want, what=""):
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        if not np.array_equal(got[k], want[k]):
            bad = np.argwhere(got[k] != want[k])[0]
            raise AssertionError(f"{what}: {k} differs first at {tuple(bad)}: kernel {got[k][tuple(bad)]}, host {want[k][tuple(bad)]}")


# ---- (1) injected uniforms --------------------------------------------------------------------------------------------------------
def _fits(W0, H0, ua, us, uw):
    """does a crop attempt with these three uniforms fit the frame?  (the test's own statement of augmentation.py:160-170, used to
    CONSTRUCT rows and to check that every branch of the issue's list is present -- never to judge the kernel)"""
    area = (0.5 + 0.5 * ua) * (W0 * H0)
    asp = 0.75 + (4. / 3 - 0.75) * us
    w, h = int(round(math.sqrt(area * asp))), int(round(math.sqrt(area / asp)))
    if uw < 0.5:
        w, h = h, w
    return w <= W0 and h <= H0


def _attempt_rows(W0, H0):
    """uniform triples (area, aspect, swap): one accepted without the swap, one accepted only because of the swap, one rejected"""
    grid = [k / 16 for k in range(16)] + [TOP]
    plain = next((a, s, 0.75) for a in grid for s in grid if _fits(W0, H0, a, s, 0.75))
    swapped = next((a, s, 0.25) for a in grid for s in grid if _fits(W0, H0, a, s, 0.25) and not _fits(W0, H0, a, s, 0.75))
    rejected = next((a, s, w) for a in reversed(grid) for s in grid for w in (0.75, 0.25) if not _fits(W0, H0, a, s, w))
    return plain, swapped, rejected


def injected_uniforms(recipe, W0, H0):
    """8 clips: random 24-bit uniforms, then the rows of the issue's list written over them.  Returns (uniforms f32 [8, slots],
    vids, the set of branch names the rows were built to take)"""
    B, slots = 8, D.recipe_slots(N_FR)
    rng = np.random.Generator(np.random.PCG64(7))
    u = (rng.integers(0, 1 << 24, (B, slots)).astype(np.float64) * 2.0 ** -24)
    vids = [0, 1, 2, 3, 4, 1, 4, 2]
    taken = set()
    u[:, D.SLOT_FLIP] = [0.25, 0.75] * 4
    taken |= {"flip on", "flip off"}
    u[5, D.SLOT_START] = u[6, D.SLOT_START] = TOP      # the last legal frame of the shortest video (1) and of the last video (4)
    u[1, D.SLOT_START] = 0.0
    taken |= {"start on the last legal frame"}
    r = D.RECIPES[recipe] if isinstance(recipe, str) else recipe
    if r["sized_p"] is not None:
        plain, swapped, rejected = _attempt_rows(W0, H0)
        att = lambda b, a, tri: u.__setitem__((b, slice(D.SLOT_ATTEMPT + 5 * a, D.SLOT_ATTEMPT + 5 * a + 3)), tri)   # noqa: E731
        u[:, D.SLOT_SIZED_P] = 0.1 if r["sized_p"] < 1 else u[:, D.SLOT_SIZED_P]
        att(0, 0, plain); taken.add("first attempt accepted")
        att(1, 0, swapped); taken.add("swap taken")
        att(2, 0, rejected); att(2, 1, plain); taken.add("rejected then accepted")
        for a in range(10):
            att(3, a, rejected)
        taken.add("all ten rejected")
        att(4, 0, plain)
        u[4, D.SLOT_ATTEMPT + 3] = u[4, D.SLOT_ATTEMPT + 4] = TOP; taken.add("randint at the top")
        if r["sized_p"] < 1:
            u[6, D.SLOT_SIZED_P] = 0.9; taken.add("CenterCrop")
    else:
        u[4, D.SLOT_CROP_X] = u[4, D.SLOT_CROP_Y] = TOP; taken.add("randint at the top")
        u[2, D.SLOT_CROP_X] = u[2, D.SLOT_CROP_Y] = 0.0
    for b in range(B):
        for f in range(N_FR):
            s = D.SLOT_FRAME + D.FRAME_SLOTS * f
            k = (b + f) % 4
            u[b, s] = 0.75 if k == 3 else 0.25                     # no gray / gray ...
            u[b, s + 1] = (k % 3) / 3 + 0.125                      # ... of channel 0, 1, 2
            u[b, s + 5] = 0.125 if (b + f) % 2 else 0.875          # hue factor below / above 0
            if f == 0:
                u[b, s + 6:s + 9] = TOP                            # every Fisher-Yates step keeps its element
            if f == 1:
                u[b, s + 6:s + 9] = 0.0
    taken |= {"each gray channel and no gray", "negative hue"}
    if r.get("jitter") and r["jitter"].get("p", 1.0) < 1:
        u[:, D.SLOT_JITTER_P] = 0.1
        u[7, D.SLOT_JITTER_P] = 0.9; taken.add("jitter skipped")
    return u.astype(np.float32), vids, taken


def check_branches(recipe, clips, W0, H0, crop, size, taken):
    """the rows did take the branches they were built for (read off the HOST recipes)"""
    r = D.RECIPES[recipe] if isinstance(recipe, str) else recipe
    assert {c["flip"] for c in clips} == {0, r["flip_code"]}
    off = offsets_of(LENGTHS)
    assert clips[5]["start"] == LENGTHS[1] - SPAN - 1 == 0 and clips[6]["start"] == LENGTHS[4] - SPAN - 1 and clips[1]["start"] == 0
    assert int(off[-1]) == sum(LENGTHS)
    if r.get("gray_p") is not None:
        assert {int(g) for c in clips for g in c["gray"]} == {-1, 0, 1, 2}
    hue = [j.hue_shift for c in clips for j in c["jitter"] if j.order[0] != 255]
    assert any(h >= 128 for h in hue) and any(0 < h < 128 for h in hue), "hue shifts of both signs (a negative factor wraps to >= 128)"
    if "jitter skipped" in taken:
        assert all(j.order[0] == 255 for j in clips[7]["jitter"]) and clips[0]["jitter"][0].order[0] != 255
    if r["sized_p"] is not None:
        wide = clips[3]["xb"][:, 1].max() if W0 >= H0 else clips[3]["yb"][:, 1].max()
        assert clips[3]["x1"] == 0 and clips[3]["y1"] == 0 and wide >= 2, "row 3 is the Scale + CenterCrop fallback"
        assert clips[4]["x1"] + int((clips[4]["xb"][:, 0] + clips[4]["xb"][:, 1]).max()) == W0, "x1 at the top of its range touches the right edge"
        if "CenterCrop" in taken:
            assert clips[6]["xk"].shape[1] == 1 and clips[6]["x1"] == int(round((W0 - size) / 2.))
    else:
        assert clips[4]["x1"] == W0 - crop and clips[4]["y1"] == H0 - crop, "randint at the top of its range"
        assert clips[2]["x1"] == 0 and clips[2]["y1"] == 0


def draw_injected_case(lib, dev, name):
    _, recipe, W0, H0, crop, size = next(s for s in DRAW_SHAPES if s[0] == name)
    u, vids, taken = injected_uniforms(recipe, W0, H0)
    off = offsets_of(LENGTHS)
    want, clips = expect(recipe, u, W0, H0, crop, size, vids, off)
    check_branches(recipe, clips, W0, H0, crop, size, taken)
    got = draw(lib, dev, recipe, W0, H0, crop, size, vids, off, seed=99, counter=3, uniforms=u)
    assert_tables_equal(got, want, name)
    taps = int(max(want["xb"][..., 1].max(), want["yb"][..., 1].max()))
    print(f"{name}: {sorted(taken)}; widest row {taps} taps, pitch {want['xk'].shape[2]}")
    return taps


# ---- (2) the Philox path ----------------------------------------------------------------------------------------------------------
def philox_uniforms(seed, counter, clip, n_fr=N_FR):
    """the documented draw: word slot & 3 of block (slot >> 2, counter, stream 4, clip) under the seed's two halves, (w >> 8) 2^-24"""
    n = D.recipe_slots(n_fr)
    ctr = np.zeros(((n + 3) // 4, 4), np.uint32)
    ctr[:, 0] = np.arange(ctr.shape[0], dtype=np.uint32)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = counter, 4, clip
    w = philox4x32_10_np(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(-1)[:n]
    return (w >> 8).astype(np.float64) * 2.0 ** -24


def philox_case(lib, dev):
    recipe, W0, H0, crop, size = "k400", 40, 30, 16, 16
    off, vids = offsets_of(LENGTHS), [2, 2, 0, 4]
    seed, ctr = (7 << 32) | 12345, 17
    got = draw(lib, dev, recipe, W0, H0, crop, size, vids, off, seed=seed, counter=ctr)
    u = np.stack([philox_uniforms(seed, ctr, b) for b in range(len(vids))])
    want, _ = expect(recipe, u, W0, H0, crop, size, vids, off)
    assert_tables_equal(got, want, "philox")
    again = draw(lib, dev, recipe, W0, H0, crop, size, vids, off, seed=seed, counter=ctr)
    assert_tables_equal(again, got, "the same (seed, counter)")
    differs = lambda a, b: any(not np.array_equal(a[k], b[k]) for k in ("xb", "xk", "yb", "yk"))   # noqa: E731
    assert differs(got, draw(lib, dev, recipe, W0, H0, crop, size, vids, off, seed=seed, counter=ctr + 1)), "the next counter"
    assert differs(got, draw(lib, dev, recipe, W0, H0, crop, size, vids, off, seed=seed + 1, counter=ctr)), "seed + 1"
    assert any(not np.array_equal(got[k][0], got[k][1]) for k in ("xb", "xk", "yb", "yk")), "clips 0 and 1 read the same video"
    # ucf101: the key's high half and the NEAREST table
    got = draw(lib, dev, "ucf101", 20, 14, 12, 8, vids, off, seed=seed, counter=ctr)
    want, _ = expect("ucf101", u, 20, 14, 12, 8, vids, off)
    assert_tables_equal(got, want, "philox ucf101")


# ---- (3) the distribution ---------------------------------------------------------------------------------------------------------
DIST_CLIPS, DIST_B, DIST_SEED = 4096, 1024, 20240
DIST_LENGTHS = (1012, 2500, 4012, 1512)      # ranges of 1000 .. 4000 starts: the floor moves the mean of start / range by < 0.0005
FLIP_BOUND = 4 * math.sqrt(0.25 / DIST_CLIPS)        # 0.031
START_BOUND = 4 * math.sqrt(1 / (12 * DIST_CLIPS))   # 0.018


def dist_stats(aug, gray0, ranges):
    return (float((aug[:, 3] != 0).mean()), float((aug[:, 0] / ranges).mean()), float((gray0 >= 0).mean()))


def check_dist(stats, what):
    flip, start, gray = stats
    print(f"{what}: flip share {flip:.4f}, mean start / range {start:.4f}, gray share {gray:.4f} (bounds {FLIP_BOUND:.3f}, {START_BOUND:.3f})")
    assert abs(flip - 0.5) <= FLIP_BOUND and abs(gray - 0.5) <= FLIP_BOUND and abs(start - 0.5) <= START_BOUND


def validate_clip(start, x1, y1, xb, yb, vlen, W0, H0):
    """what data.recipe_to_input checks on the host before it trusts a draw"""
    assert 0 <= start and start + (N_FR - 1) * DS < vlen, (start, vlen)
    assert x1 >= 0 and y1 >= 0 and x1 + int((xb[:, 0] + xb[:, 1]).max()) <= W0 and y1 + int((yb[:, 0] + yb[:, 1]).max()) <= H0, (x1, y1, xb, yb)
    assert (xb[:, 1] >= 1).all() and (yb[:, 1] >= 1).all() and (xb[:, 0] >= 0).all() and (yb[:, 0] >= 0).all()


def dist_vids():
    return np.arange(DIST_CLIPS) % len(DIST_LENGTHS)


def dist_host_case():
    """the host statement over numpy uniforms of the same count stays inside the bounds for the chosen seed"""
    rng = np.random.Generator(np.random.PCG64(DIST_SEED))
    u = rng.integers(0, 1 << 24, (DIST_CLIPS, D.recipe_slots(N_FR))).astype(np.float64) * 2.0 ** -24
    vids, L_ = dist_vids(), np.asarray(DIST_LENGTHS)
    aug, gray0 = np.zeros((DIST_CLIPS, 4), np.int64), np.zeros(DIST_CLIPS, np.int64)
    for i in range(DIST_CLIPS):
        c = D.recipe_from_uniforms("k400", u[i], int(L_[vids[i]]), 40, 30, 4, 4, N_FR, SPAN)
        validate_clip(c["start"], c["x1"], c["y1"], c["xb"], c["yb"], int(L_[vids[i]]), 40, 30)
        aug[i], gray0[i] = (c["start"], c["x1"], c["y1"], c["flip"]), c["gray"][0]
    check_dist(dist_stats(aug, gray0, (L_ - SPAN)[vids]), "host")


def dist_kernel_case(lib, dev):
    vids, L_, off = dist_vids(), np.asarray(DIST_LENGTHS), offsets_of(DIST_LENGTHS)
    parts = [draw(lib, dev, "k400", 40, 30, 4, 4, vids[i:i + DIST_B], off, seed=DIST_SEED, counter=1 + i // DIST_B)
             for i in range(0, DIST_CLIPS, DIST_B)]
    t = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    for i in range(DIST_CLIPS):
        validate_clip(int(t["aug"][i, 0]), int(t["aug"][i, 1]), int(t["aug"][i, 2]), t["xb"][i], t["yb"][i], int(L_[vids[i]]), 40, 30)
    assert np.array_equal(t["clip_first"], off[vids])
    check_dist(dist_stats(t["aug"].astype(np.int64), t["gray"][:, 0].astype(np.int64), (L_ - SPAN)[vids]), "kernel")


# ---- (4) the gather ---------------------------------------------------------------------------------------------------------------
STORE_LENGTHS = (9, 23, 12, 17, 14)       # 5 videos of 9 .. 23 frames
GW0, GH0, GSIZE = 40, 30, 16
GN, GSL, GDS = 2, 2, 2                    # 4 frames per clip, 2 apart: a video needs more than 8
G_FR, GSPAN = GN * GSL, GN * GSL * GDS


def ragged_store(seed=5):
    rng = np.random.Generator(np.random.PCG64(seed))
    off = offsets_of(STORE_LENGTHS)
    return rng.integers(0, 256, (int(off[-1]), GH0, GW0, 3), dtype=np.uint8), off


def pack_tables(dev, clips, firsts, size):
    """host recipes -> the device tables of dpc_store_to_input, packed like data.recipe_to_input packs them"""
    B = len(clips)
    ksx, ksy = max(c["xk"].shape[1] for c in clips), max(c["yk"].shape[1] for c in clips)
    aug = np.array([(c["start"], c["x1"], c["y1"], c["flip"]) for c in clips], np.int32)
    xb, yb = np.stack([c["xb"] for c in clips]).astype(np.int32), np.stack([c["yb"] for c in clips]).astype(np.int32)
    xk, yk = np.zeros((B, size, ksx), np.int32), np.zeros((B, size, ksy), np.int32)
    for b, c in enumerate(clips):
        xk[b, :, :c["xk"].shape[1]], yk[b, :, :c["yk"].shape[1]] = c["xk"], c["yk"]
    gray = np.stack([c["gray"] for c in clips]).astype(np.int8)
    any_jit = any(j.order[0] != 255 for c in clips for j in c["jitter"])
    jit = np.concatenate([np.frombuffer(bytes(c["jitter"]), np.uint8) for c in clips])
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(aug=aug, xb=xb, yb=yb, xk=xk, yk=yk, gray=gray, jitter=jit.copy(),
                                                          clip_first=np.asarray(firsts, np.int64)).items()}
    t["rs"] = L.Resample(t["xb"].data_ptr(), t["xk"].data_ptr(), t["yb"].data_ptr(), t["yk"].data_ptr(), ksx, ksy)
    if not any_jit:
        t["jitter"] = None
    return t


def gather_from_store(lib, dev, store_dev, clips, firsts, size, dtype, n=GN, sl=GSL, ds=GDS):
    B, n_fr = len(clips), n * sl
    t = pack_tables(dev, clips, firsts, size)
    block = torch.full((B, n, 3, sl, size, size), float("nan"), device=dev)
    s2d = torch.full((B * n, sl, size // 2, size // 2, 16), float("nan"), device=dev).to(dtype)
    u8 = torch.empty(B * n_fr * size * size * 3, dtype=torch.uint8, device=dev)
    ls = torch.empty(B * n_fr, dtype=torch.int64, device=dev)
    D.store_to_input(lib, store_dev, t["aug"], t["clip_first"], t["gray"], t["rs"], t["jitter"], n, sl, ds, size, block, s2d, u8, ls)
    _sync(dev)
    return block.cpu(), s2d.cpu()


def gather_by_hand(lib, dev, frames, off, vids, clips, size, dtype, n=GN, sl=GSL, ds=GDS):
    """dpc_frames_to_input_ex on the clips' spans, cut out of the host array by hand"""
    B, span = len(clips), (n * sl - 1) * ds + 1
    dense = np.stack([frames[off[v] + c["start"]: off[v] + c["start"] + span] for v, c in zip(vids, clips)])
    block = torch.full((B, n, 3, sl, size, size), float("nan"), device=dev)
    s2d = torch.full((B * n, sl, size // 2, size // 2, 16), float("nan"), device=dev).to(dtype)
    D.recipe_to_input(lib, torch.from_numpy(dense).to(dev), [0] * B, clips, n, sl, ds, size, block, s2d)
    _sync(dev)
    return block.cpu(), s2d.cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def gather_clips(recipe, vids, off, starts=(TOP, 0.5, TOP), seed=31):
    """host recipes of one batch; `starts` = the uniform of each clip's start (TOP: the last legal one of its video)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    u = rng.integers(0, 1 << 24, (len(vids), D.recipe_slots(G_FR))).astype(np.float64) * 2.0 ** -24
    u[:, D.SLOT_START] = starts
    return [D.recipe_from_uniforms(recipe, u[b], int(off[v + 1] - off[v]), GW0, GH0, GSIZE, GSIZE, G_FR, GSPAN) for b, v in enumerate(vids)]


def gather_case(lib, dev, jitter, dtype):
    frames, off = ragged_store()
    vids = [0, 3, 4]             # the first and the last video among them
    clips = gather_clips("k400" if jitter else NOJIT, vids, off)
    assert clips[0]["start"] == STORE_LENGTHS[0] - GSPAN - 1 == 0 and clips[2]["start"] == STORE_LENGTHS[4] - GSPAN - 1
    store_dev = torch.from_numpy(frames).to(dev)
    got = gather_from_store(lib, dev, store_dev, clips, [int(off[v]) for v in vids], GSIZE, dtype)
    want = gather_by_hand(lib, dev, frames, off, vids, clips, GSIZE, dtype)
    assert bool(torch.isfinite(want[0]).all()) and bool(torch.isfinite(want[1].float()).all())
    assert same_bits(got[0], want[0]), "block differs"
    assert same_bits(got[1], want[1]), "space-to-depth operand differs"
    assert not same_bits(want[0][0], want[0][1])


# ---- (5) the engine ---------------------------------------------------------------------------------------------------------------
E_SIZE, E_W0, E_H0, E_B = 64, 80, 60, 2


def engine_store(n_videos=4, seed=9, n_fr=N_FR, ds=5):
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = [n_fr * ds + 2 + 3 * i for i in range(n_videos)]
    off = offsets_of(lengths)
    base = rng.integers(0, 256, (1, E_H0 // 4, E_W0 // 4, 3), dtype=np.uint8).repeat(4, 1).repeat(4, 2)
    frames = (base.astype(np.int16) + rng.integers(-40, 41, (int(off[-1]), E_H0, E_W0, 3))).clip(0, 255).astype(np.uint8)
    return frames, off


def host_recipes(src, mine_row, counter):
    """what load_resident draws for one batch, from the documented Philox words: (spans u8 [B, span, H0, W0, 3], clips)"""
    st = src.store
    clips, spans = [], []
    span = (src.n_fr - 1) * src.ds + 1
    for b, v in enumerate(mine_row):
        vlen = int(st.offsets[v + 1] - st.offsets[v])
        c = D.recipe_from_uniforms(src.dataset, philox_uniforms(src.seed, counter, b, src.n_fr), vlen, st.W0, st.H0, src.crop, src.size,
                                   src.n_fr, src.n_fr * src.ds)
        clips.append(c)
        spans.append(np.asarray(st.frames[st.offsets[v] + c["start"]: st.offsets[v] + c["start"] + span]))
    return np.stack(spans), clips


E_N, E_SL, E_PRED = 4, 3, 1               # 12 frames per clip at the k400 stride of 5: a video needs more than 60


def make_engine(lib, dev, dtype, widths=None):
    from dpc_amd.engine import DPCEngine
    from oracle import dpc_oracle as O
    kw = dict(lib=lib) if str(dev) == "cpu" else dict(reserve_cus=0)
    args = ("resnet18", E_SIZE, E_N, E_SL, E_PRED, E_B, dev, dtype) + ((widths,) if widths else ())
    eng = DPCEngine(*args, seed=233, **kw)
    eng.load_params(O.make_params_pcg("resnet18", widths) if widths else O.make_params_pcg("resnet18"))
    return eng


def make_source(dev, n_videos=4, seed=(1 << 32) | 3):
    frames, off = engine_store(n_videos, n_fr=E_N * E_SL)
    st = D.FrameStore(frames, off).to_device(dev)
    return D.ResidentFrameSource(st, "k400", E_N, E_SL, 1, E_SIZE, E_B, dev, seed=seed)


def engine_case(lib, dev, dtype, widths=None, steps=2, train=True):
    """load_resident == load_recipe fed with hand-cut spans and recipe_from_uniforms(the documented Philox words): the operand, and
    the parameters after `steps` train steps, bit for bit (train=False: the operand only -- a simulated train step takes most of a
    minute, and the MI355X tier runs this case whole)"""
    a, b = make_engine(lib, dev, dtype, widths), make_engine(lib, dev, dtype, widths)
    src = make_source(dev)
    assert len(src) == 2 and src.KS == 2 * -(-E_W0 // E_SIZE) + 1
    mine = src.begin_epoch()
    assert sorted(mine.reshape(-1).tolist()) == [0, 1, 2, 3]
    for i in range(steps):
        a.load_resident(src)
        spans, clips = host_recipes(src, mine[i], i + 1)
        b.load_recipe(torch.from_numpy(spans).to(dev), [0] * E_B, clips, ds=src.ds)
        _sync(dev)
        assert same_bits(a.x_s2d.cpu(), b.x_s2d.cpu()), f"step {i}: the stem's operand differs"
        assert bool(torch.isfinite(a.x_s2d.float()).all())
        if train:
            ra, rb = a.train_step(None).clone(), b.train_step(None).clone()
            _sync(dev)
            assert torch.equal(ra, rb)
        if i == 0:
            ws = a._resident_ws
    assert int(src.cursor.item()) == steps and int(src.draw.item()) == steps
    assert a._resident_ws is ws and ws is not None, "the jitter workspaces are allocated once"
    if train:
        assert torch.equal(a.flat_p, b.flat_p) and torch.equal(a.flat_m, b.flat_m) and a.step_count == steps


def graph_case(dev, dtype):
    """three replayed steps that span an epoch boundary (2 steps per epoch: the permutation is uploaded again, the cursor zeroed)
    == an eager twin; ONE capture serves both epochs"""
    a, b = make_engine(None, dev, dtype), make_engine(None, dev, dtype)
    sa, sb = make_source(dev), make_source(dev)
    g = torch.Generator().manual_seed(11)
    perms = [torch.randperm(4, generator=g) for _ in range(3)]

    def begin(src, e):   # the same permutation for both engines, whatever torch's global generator holds
        mine = perms[e].numpy().astype(np.int32)
        src.perm.copy_(torch.from_numpy(src.keep[mine].astype(np.int32)))
        src.cursor.zero_()

    for e in range(3):   # eager: 6 steps over 3 epochs
        begin(sa, e)
        for _ in range(2):
            a.load_resident(sa)
            ra = a.train_step(None).clone()
    begin(sb, 0)
    for _ in range(2):   # epoch 0 eagerly (the warm-up of the entry) ...
        b.load_resident(sb)
        b.train_step(None)
    refill = lambda: b.load_resident(sb)   # noqa: E731
    replay = b.capture_train_step(None, warmup=0, refill=refill)
    kernels = list(replay.kernels)
    begin(sb, 1)
    for _ in range(2):   # ... epoch 1 replayed ...
        replay()
    begin(sb, 2)         # ... and across the boundary: new permutation, cursor reset, the same graph
    for _ in range(2):
        rb = replay().clone()
    torch.cuda.synchronize()
    assert b.capture_train_step(None, warmup=0, refill=refill) is replay and list(replay.kernels) == kernels and all(kernels)
    assert int(sb.draw.item()) == 6 and int(sb.cursor.item()) == 2 and a.step_count == b.step_count == 6
    assert torch.equal(a.flat_p, b.flat_p) and torch.equal(a.flat_m, b.flat_m) and torch.equal(ra, rb)


def big_store_case(lib, dev):
    """a store of more than 2^31 bytes, only its last video written: a clip of that video == the same video gathered from a
    small store.  A 32-bit frame address fails this."""
    frames, off = ragged_store()
    last = frames[off[-2]:]
    total = (1 << 31) // (GH0 * GW0 * 3) + 1000
    big = torch.empty((total, GH0, GW0, 3), dtype=torch.uint8, device=dev)
    assert big.numel() > (1 << 31) + last.size
    first = total - last.shape[0]
    big[first:] = torch.from_numpy(last).to(dev)
    clips = gather_clips("k400", [4, 4, 4], off, starts=(0.0, 0.5, TOP))
    assert [c["start"] for c in clips] == [0, 3, 5]
    got = gather_from_store(lib, dev, big, clips, [first] * 3, GSIZE, torch.bfloat16)
    del big
    want = gather_from_store(lib, dev, torch.from_numpy(last).to(dev), clips, [0] * 3, GSIZE, torch.bfloat16)
    assert bool(torch.isfinite(want[0]).all()) and same_bits(got[0], want[0]) and same_bits(got[1], want[1])


def draw_rejects_case(lib, dev):
    """the entry checks what it can: a pitch below the documented worst case, a crop box larger than the frame, too many clips"""
    fn = lib._fn("dpc_draw_recipe")
    t = Tables(dev, 2, 16, 7)
    z = torch.zeros(8, dtype=torch.int64, device=dev)
    p = lambda x: x.data_ptr()   # noqa: E731

    def call(recipe, B=2, W0=40, H0=30, crop=16, size=16, KS=7, tab=None):
        d = D.recipe_desc(recipe)
        return fn(C.byref(d), p(z), None, p(z), B, W0, H0, crop, size, N, SL, DS, KS, tab, 1, p(z), None, p(t.aug), p(t.clip_first), p(t.gray),
                  p(t.jitter), p(t.xb), p(t.xk), p(t.yb), p(t.yk), None)

    before = t.host()
    assert call("k400", KS=6) == L.ERR_ARG and call("k400", W0=49) == L.ERR_ARG           # 2 ceil(40 / 16) + 1 = 7, 2 ceil(49 / 16) + 1 = 9
    assert call("ucf101", crop=31) == L.ERR_ARG and call("ucf101", crop=12) == L.ERR_ARG  # box leaves the frame; Scale without its table
    assert call("k400", B=1025) == L.ERR_UNSUPPORTED and call(LCISH, size=32, KS=7) == L.ERR_UNSUPPORTED   # CenterCrop(32) of 40 x 30
    assert call(dict(NOJIT, flip_code=3)) == L.ERR_ARG
    assert_tables_equal(t.host(), before, "a rejected call wrote")


# ---- (6) the entry ----------------------------------------------------------------------------------------------------------------
def entry_files(tmp, n_videos=4):
    """a tiny ragged store on disk: n_videos usable videos and one that is too short (dropped, and said so)"""
    import os
    frames, off = engine_store(n_videos, n_fr=E_N * E_SL)
    short = frames[:7]
    fp, op = os.path.join(tmp, "store.npy"), os.path.join(tmp, "offsets.npy")
    np.save(fp, np.concatenate([frames[:off[1]], short, frames[off[1]:]]))
    np.save(op, np.concatenate([off[:2], off[1:] + 7]))
    return fp, op


def entry_run(tmp, name, fp, op, dtype, epochs, B, extra, **kw):
    import os
    from dpc_amd import main as dpc_main
    d, pr = os.path.join(tmp, name), os.path.join(tmp, name + "_probe")
    os.makedirs(pr)
    dpc_main.main(["--net", "resnet18", "--img_dim", str(E_SIZE), "--gpu", "0", "--dtype", dtype, "--epochs", str(epochs), "--batch_size", str(B),
                   "--print_freq", "1", "--num_seq", str(E_N), "--seq_len", str(E_SL), "--pred_step", str(E_PRED), "--dataset", "k400",
                   "--frames", fp, "--offsets", op, "--resident", "--save_dir", d] + list(extra), _probe=pr, **kw)
    ck = torch.load(os.path.join(d, f"epoch{epochs}.pth.tar"), map_location="cpu", weights_only=False)
    return ck, torch.load(os.path.join(pr, "rank0.pt"))


def loss_lines(out):
    import re
    return [re.sub(r"T:[0-9.]+", "", ln) for ln in out.splitlines() if "Loss" in ln]


def entry_case(tmp, cap, graph, sim=None, widths=None):
    """`python -m dpc_amd.main --frames store.npy --offsets offsets.npy --resident` (in-process).  graph: the same with --graph must
    print the same lines and save the same state_dict.  Simulator tier: one epoch, eager."""
    kw = dict(_simulator=sim, _widths=widths) if sim is not None else {}
    epochs, B, steps, dtype = (1, 1, 1, "f32") if sim is not None else (2, E_B, 2, "bf16")    # steps per epoch
    fp, op = entry_files(tmp, n_videos=B * steps)
    cap.readouterr()
    ck, probe = entry_run(tmp, "eager", fp, op, dtype, epochs, B, [], **kw)
    out = cap.readouterr().out
    lines = loss_lines(out)
    assert "1 training / 1 validation videos skipped" in out
    assert len(lines) == epochs * (steps + 1) and probe["step"] == steps * epochs and ck["iteration"] == steps * epochs, out
    assert all(math.isfinite(float(x)) for ln in lines for x in ln.split("Loss")[1].split()[:1])
    if not graph:
        return
    ck_g, probe_g = entry_run(tmp, "graph", fp, op, dtype, epochs, B, ["--graph"], **kw)
    out_g = cap.readouterr().out
    assert "Graph replay: 2 steps" in out_g
    assert loss_lines(out_g) == lines
    assert torch.equal(probe["flat_p"], probe_g["flat_p"]) and torch.equal(probe["flat_m"], probe_g["flat_m"])
    assert set(ck["state_dict"]) == set(ck_g["state_dict"]) and all(torch.equal(v, ck_g["state_dict"][k]) for k, v in ck["state_dict"].items())
