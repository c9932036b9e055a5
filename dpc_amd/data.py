"""GPU-side input pipeline: the per-clip random draws of the reference's loader stay on the host
(a handful of integers), the per-pixel work -- frame gather, crop, flip, channel splitting, ToTensor, Normalize, the
[N, C, SL, H, W] layout -- is one HIP kernel (csrc/input_pipeline.hip) that can write the stem's operand directly.

Restates dpc/dataset_3d.py:85-111 (idx_sampler, __getitem__) and the transforms of utils/augmentation.py: RandomCrop :99-143,
RandomSizedCrop :144-196 (crop box + PIL's BILINEAR resize as fixed-point resampling tables, `resample_tables`),
RandomHorizontalFlip :198-222, RandomGray :224-251, ColorJitter :253-351 (per-frame factors and shuffled order; the PIL /
torchvision arithmetic lives in the kernel), Scale :20-43 (NEAREST tables from PIL itself, `nearest_tables`), ToTensor /
Normalize :368-379.  `draw_k400` / `draw_ucf101` make the random choices of the two training recipes of dpc/main.py:114-132
with the SAME calls of `random` / `np.random` in the same order as the reference's classes, so a seeded run reproduces the
reference's clip bit for bit (tests/golden/aug.npz holds clips produced by the reference's own classes)."""
from __future__ import annotations

import ctypes as C
import math
import random
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L

MEAN = (0.485, 0.456, 0.406)  # utils/augmentation.py:374
STD = (0.229, 0.224, 0.225)


class ClipAug(C.Structure):
    """struct dpc_clip_aug (include/dpc_hip.h)"""
    _fields_ = [(n, C.c_int32) for n in ("start", "x1", "y1", "flip")]


def draw_clip_params(rng: np.random.Generator, B: int, vlen: int, num_seq: int, seq_len: int, ds: int, H0: int, W0: int, size: int,
                     flip_p: float = 0.5, gray_p: float = 0.5, flip_code: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """the loader's random choices for B clips: start frame (idx_sampler, dataset_3d.py:85-92), crop corner
    (RandomCrop consistent=True), flip (RandomHorizontalFlip consistent=True), per-frame gray channel
    (RandomGray consistent=False, p; -1 = keep colour).  Returns (aug int32 [B,4], gray int8 [B, num_seq*seq_len])."""
    span = vlen - num_seq * seq_len * ds
    if span <= 0:
        raise ValueError("video too short (dataset_3d.py:87 drops it)")
    aug = np.zeros((B, 4), np.int32)
    aug[:, 0] = rng.integers(0, span, B)
    aug[:, 1] = rng.integers(0, W0 - size + 1, B)   # `size` here = the side of the crop box (224 in the ucf101 recipe)
    aug[:, 2] = rng.integers(0, H0 - size + 1, B)
    aug[:, 3] = (rng.random(B) < flip_p) * flip_code
    gray = np.where(rng.random((B, num_seq * seq_len)) < gray_p, rng.integers(0, 3, (B, num_seq * seq_len)), -1).astype(np.int8)
    return aug, gray


_NEAREST_TABLES = {}


def nearest_tables(crop: int, size: int):
    """Scale(size=(size, size)) with its default NEAREST interpolation (utils/augmentation.py:20-43; the ucf101 recipe crops
    224 and scales to img_dim, dpc/main.py:116-118): output index -> index inside the crop, obtained from PIL itself by resizing
    a coordinate ramp, so whatever rounding PIL's resampler applies is reproduced exactly."""
    key = (crop, size)
    if key not in _NEAREST_TABLES:
        from PIL import Image
        ramp = Image.fromarray(np.tile(np.arange(crop, dtype=np.int32), (2, 1)), mode="I")
        xt = np.array(ramp.resize((size, 2), Image.NEAREST))[0].astype(np.int32)
        _NEAREST_TABLES[key] = xt
    return _NEAREST_TABLES[key]


def frames_to_input(lib: L.Lib, frames: torch.Tensor, aug: torch.Tensor, gray: Optional[torch.Tensor], num_seq: int, seq_len: int,
                    ds: int, size: int, block: Optional[torch.Tensor] = None, s2d: Optional[torch.Tensor] = None, crop: Optional[int] = None):
    """frames u8 [B,F,H0,W0,3]; aug int32 [B,4] (start, x1, y1, flip: 0 / 1 after crop (k400) / 2 before crop (ucf101));
    gray int8 [B, N*SL] or None -- all on the kernels' device.  crop: side of the crop box when it differs from `size`
    (Scale, NEAREST).  Fills block f32 [B,N,3,SL,size,size] and / or s2d [B*N,SL,size/2,size/2,16] (compute dtype)."""
    B, F, H0, W0, ch = frames.shape
    if ch != 3 or frames.dtype != torch.uint8 or aug.dtype != torch.int32 or tuple(aug.shape) != (B, 4):
        raise ValueError("frames must be uint8 [B,F,H0,W0,3], aug int32 [B,4]")
    # the kernel trusts the draws: check them here (a short clip or a bad box would read outside the frames buffer)
    a = aug.detach().cpu()
    box = crop or size
    if int(a[:, 0].min()) < 0 or int(a[:, 0].max()) + (num_seq * seq_len - 1) * ds >= F:
        raise ValueError(f"sampled frames leave the video: start up to {int(a[:, 0].max())}, {num_seq * seq_len} frames every {ds}, {F} available")
    if int(a[:, 1].min()) < 0 or int(a[:, 2].min()) < 0 or int(a[:, 1].max()) + box > W0 or int(a[:, 2].max()) + box > H0:
        raise ValueError(f"crop box of {box} pixels leaves the {W0} x {H0} frame")
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    tab = None
    if crop is not None and crop != size:
        tab = torch.from_numpy(nearest_tables(crop, size)).to(frames.device)
    lib.call("dpc_frames_to_input", frames.contiguous(), B, F, H0, W0, aug.contiguous(), gray.contiguous() if gray is not None else None,
             num_seq, seq_len, ds, size, size, tab, tab, crop or size, crop or size, mean, std, block, s2d,
             L.dtype_code(s2d.dtype) if s2d is not None else L.F32, lib.stream())
    return block, s2d


# ------------------------------------------------------------------------------------------------------------------
# the full training recipes of dpc/main.py:114-132 (ColorJitter and the BILINEAR resize of RandomSizedCrop included)
# ------------------------------------------------------------------------------------------------------------------
RS_PREC = 32 - 8 - 2  # PIL ImagingResample PRECISION_BITS (8 bits per channel)


class FrameJitter(C.Structure):
    """struct dpc_frame_jitter (include/dpc_hip.h)"""
    _fields_ = [("factor", C.c_float * 3), ("hue_shift", C.c_int32), ("order", C.c_uint8 * 4)]


def resample_tables(in_size: int, out_size: int, first: int = 0, count: Optional[int] = None, support: float = 1.0):
    """PIL's ImagingResample coefficient tables for resizing a line of `in_size` samples to `out_size` with the BILINEAR (triangle)
    filter, restated from libImaging/Resample.c (precompute_coeffs + normalize_coeffs_8bpc): double-precision weights,
    normalised, rounded to 22-bit fixed point.  Rows [first, first + count) of the table.  Returns (bounds int32 [count, 2] =
    (first source index, taps), coefficients int32 [count, ksize])."""
    count = out_size - first if count is None else count
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    sup = support * fscale
    ksize = int(math.ceil(sup)) * 2 + 1
    bounds = np.zeros((count, 2), np.int32)
    coef = np.zeros((count, ksize), np.int32)
    ss = 1.0 / fscale
    for i in range(count):
        xx = first + i
        center = (xx + 0.5) * scale
        xmin = max(int(center - sup + 0.5), 0)
        xmax = min(int(center + sup + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)]
        ww = sum(w)  # same left-to-right accumulation as the C loop
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[i] = (xmin, xmax)
        for x, v in enumerate(w):
            coef[i, x] = int(-0.5 + v * (1 << RS_PREC)) if v < 0 else int(0.5 + v * (1 << RS_PREC))
    return bounds, coef


def _tables_from_index(idx: np.ndarray):
    """a pure index map (NEAREST) in resampling-table form: one tap of weight 1.0 (clip8((1 << 21) + v << 22) == v)"""
    b = np.stack([idx.astype(np.int32), np.ones_like(idx, dtype=np.int32)], 1)
    return b, np.full((len(idx), 1), 1 << RS_PREC, np.int32)


def _jitter_get_params(j: FrameJitter, jitter: dict):
    """ColorJitter.get_params (utils/augmentation.py:298-326) into one dpc_frame_jitter: four uniform draws, then random.shuffle of the list"""
    ops: List[int] = []
    for op, name in enumerate(("brightness", "contrast", "saturation", "hue")):
        v = jitter.get(name, 0)
        if not v:
            continue
        lo, hi = (-v, v) if name == "hue" else (max(0.0, 1.0 - v), 1.0 + v)   # _check_input
        f = random.uniform(lo, hi)
        if name == "hue":
            j.hue_shift = int(f * 255) & 0xFF   # np.uint8(hue_factor * 255): C truncation, uint8 wrap
        else:
            j.factor[op] = f
        ops.append(op)
    random.shuffle(ops)
    for k, op in enumerate(ops):
        j.order[k] = op


def _draw_gray_and_jitter(n_frames: int, gray_p: float, jitter: Optional[dict], consistent: bool = False):
    """RandomGray(consistent=False, p) then ColorJitter(..., p) over the frames of one clip, call for call (utils/augmentation.py:229-243
    and :310-351).  consistent=False: one get_params draw per frame (the pre-training recipes); consistent=True: ONE draw copied to
    every frame (:330-333, the fine-tuning recipes of eval/test.py:161-176).  gray_p = None: the recipe has no RandomGray."""
    gray = np.full(n_frames, -1, np.int8)
    if gray_p is not None:
        for i in range(n_frames):                   # RandomGray: one Bernoulli per frame, then np.random.choice(3)
            if random.random() < gray_p:
                gray[i] = np.random.choice(3)
    jit = (FrameJitter * n_frames)()
    for i in range(n_frames):
        jit[i].order[:] = [255, 255, 255, 255]
    if jitter is not None and random.random() < jitter.get("p", 1.0):
        for i in range(1 if consistent else n_frames):
            _jitter_get_params(jit[i], jitter)
        if consistent:
            for i in range(1, n_frames):
                jit[i] = jit[0]
    return gray, jit


def _draw_sized_crop(W0: int, H0: int, size: int, p: float):
    """RandomSizedCrop(size, BILINEAR, consistent=True, p).__call__ (utils/augmentation.py:151-195) on W0 x H0 frames: the crop box and the
    BILINEAR resize to size x size as resampling tables.  Returns (x1, y1, (xb, xk), (yb, yk), taken); taken = False is the CenterCrop(size)
    branch of a failed `p` draw (:193-195), an index map."""
    if random.random() < p:                                     # RandomSizedCrop.threshold = p
        for _ in range(10):
            area = W0 * H0
            target_area = random.uniform(0.5, 1) * area
            aspect = random.uniform(3. / 4, 4. / 3)
            w = int(round(math.sqrt(target_area * aspect)))
            h = int(round(math.sqrt(target_area / aspect)))
            if random.random() < 0.5:
                w, h = h, w
            if w <= W0 and h <= H0:
                x1 = random.randint(0, W0 - w)
                y1 = random.randint(0, H0 - h)
                return x1, y1, resample_tables(w, size), resample_tables(h, size), True
        # fallback (augmentation.py:190-193): Scale(size) then CenterCrop(size), both on the whole frame
        if W0 < H0:
            ow, oh = size, int(size * H0 / W0)
        else:
            oh, ow = size, int(size * W0 / H0)
        cx, cy = int(round((ow - size) / 2.)), int(round((oh - size) / 2.))
        return 0, 0, resample_tables(W0, ow, cx, size), resample_tables(H0, oh, cy, size), True
    if W0 < size or H0 < size:
        raise ValueError(f"CenterCrop({size}) of {W0} x {H0} frames leaves the frame (PIL would pad with black; not reproduced)")
    ident = np.arange(size, dtype=np.int32)
    return int(round((W0 - size) / 2.)), int(round((H0 - size) / 2.)), _tables_from_index(ident), _tables_from_index(ident), False


def draw_k400(W0: int, H0: int, size: int, n_frames: int, gray_p: float = 0.5,
              jitter: Optional[dict] = dict(brightness=0.5, contrast=0.5, saturation=0.5, hue=0.25, p=1.0)):
    """the k400 training recipe (dpc/main.py:124-132) for ONE clip of n_frames frames of W0 x H0 pixels:
    RandomSizedCrop(size, consistent=True, p=1.0) -> RandomHorizontalFlip(consistent=True) -> RandomGray(p=0.5) -> ColorJitter.
    Consumes `random` / `np.random` exactly as the reference's classes do.  Returns dict(x1, y1, flip, xb, xk, yb, yk, gray, jitter)."""
    x1, y1, xt, yt, _ = _draw_sized_crop(W0, H0, size, 1.0)
    flip = 1 if random.random() < 0.5 else 0                    # RandomHorizontalFlip(consistent=True): after the crop + resize
    gray, jit = _draw_gray_and_jitter(n_frames, gray_p, jitter)
    return dict(x1=x1, y1=y1, flip=flip, xb=xt[0], xk=xt[1], yb=yt[0], yk=yt[1], gray=gray, jitter=jit)


def draw_ucf101(W0: int, H0: int, crop: int, size: int, n_frames: int, gray_p: float = 0.5,
                jitter: Optional[dict] = dict(brightness=0.5, contrast=0.5, saturation=0.5, hue=0.25, p=1.0)):
    """the ucf101 training recipe (dpc/main.py:114-123): RandomHorizontalFlip -> RandomCrop(crop) -> Scale((size, size)) [NEAREST]
    -> RandomGray(p=0.5) -> ColorJitter, same contract as draw_k400 (flip code 2: the frame is flipped BEFORE the crop)"""
    flip = 2 if random.random() < 0.5 else 0
    x1 = y1 = 0
    if not (W0 == crop and H0 == crop):                         # RandomCrop draws only when there is something to crop
        x1 = random.randint(0, W0 - crop)
        y1 = random.randint(0, H0 - crop)
    idx = nearest_tables(crop, size) if crop != size else np.arange(size, dtype=np.int32)
    xb, xk = _tables_from_index(idx)
    gray, jit = _draw_gray_and_jitter(n_frames, gray_p, jitter)
    return dict(x1=x1, y1=y1, flip=flip, xb=xb, xk=xk, yb=xb.copy(), yk=xk.copy(), gray=gray, jitter=jit)


LC_RECIPES = {   # eval/test.py:161-176 (train, val) and :121-126 (test): RandomSizedCrop's p, flip, ColorJitter(consistent=True)
    "train": dict(p=1.0, flip=True, jitter=dict(brightness=0.5, contrast=0.5, saturation=0.5, hue=0.25, p=0.3)),
    "val": dict(p=0.3, flip=True, jitter=dict(brightness=0.2, contrast=0.2, saturation=0.2, hue=0.1, p=0.3)),
    "test": dict(p=0.0, flip=False, jitter=None),
}


def draw_lc(W0: int, H0: int, crop: int = 224, size: int = 128, n_frames: int = 40, mode: str = "train"):
    """the three recipes of the downstream classifier (eval/test.py:121-126,161-176) for ONE clip: RandomSizedCrop(size=crop, BILINEAR,
    consistent=True, p) -> Scale((size, size)) [NEAREST] -> RandomHorizontalFlip(consistent=True) -> ColorJitter(consistent=True, p=0.3);
    the test recipe has neither flip nor jitter and p = 0.0 (always the CenterCrop).  Same `random` calls in the same order as the
    reference's classes; same contract as draw_k400.  The NEAREST Scale after the BILINEAR resize picks rows of the BILINEAR table:
    PIL's resize is separable and per output sample, so a sub-sampled output is an exact subset."""
    if mode not in LC_RECIPES:
        raise ValueError(f"mode must be one of {sorted(LC_RECIPES)}")
    r = LC_RECIPES[mode]
    x1, y1, xt, yt, taken = _draw_sized_crop(W0, H0, crop, r["p"])
    idx = nearest_tables(crop, size) if crop != size else np.arange(size, dtype=np.int32)
    flip = (1 if random.random() < 0.5 else 0) if r["flip"] else 0   # after crop + scale
    gray, jit = _draw_gray_and_jitter(n_frames, None, r["jitter"], consistent=True)
    return dict(x1=x1, y1=y1, flip=flip, xb=xt[0][idx], xk=xt[1][idx], yb=yt[0][idx], yk=yt[1][idx], gray=gray, jitter=jit, sized_crop=taken)


def lc_test_windows(vlen: int, num_seq: int, seq_len: int, ds: int, dataset: str = "ucf101") -> List[int]:
    """first frames of the test-time windows of one video (eval/dataset_3d_lc.py:72-78,109-127): every frame at stride ds, cut into
    seq_len blocks, a num_seq-block window slid by num_seq // 2 blocks (ucf101, :124) or 3 * num_seq // 4 (hmdb51, :254).  A video with
    vlen - num_seq * seq_len * ds <= 0 has no window: the dataset class drops it (:61-67)."""
    if dataset not in ("ucf101", "hmdb51"):
        raise ValueError("dataset not supported")
    stride = num_seq // 2 if dataset == "ucf101" else 3 * num_seq // 4
    if num_seq < 2 or stride < 1:
        raise ValueError(f"num_seq {num_seq}: the window stride of the test protocol is {stride} blocks (range() with step 0 in the reference)")
    if vlen - num_seq * seq_len * ds <= 0:
        return []
    nblk = len(range(0, vlen, ds)) // seq_len
    return [w * seq_len * ds for w in range(0, nblk + 1 - num_seq, stride)]


def video_windows_to_input(lib: L.Lib, video: torch.Tensor, vlen: int, starts, clip: dict, num_seq: int, seq_len: int, ds: int, size: int,
                           block: Optional[torch.Tensor] = None, s2d: Optional[torch.Tensor] = None):
    """ONE video u8 [F,H0,W0,3] on the kernels' device, of which the first vlen frames are real; starts[b] = first frame of window b
    (lc_test_windows); clip = one draw_lc(..., mode='test') result, shared by the windows (the transform sees the whole video once,
    dataset_3d_lc.py:96).  Fills block f32 [B,N,3,SL,size,size] and / or the stem's operand through dpc_video_windows_to_input:
    no frame is replicated."""
    if video.dim() != 4 or video.shape[3] != 3 or video.dtype != torch.uint8:
        raise ValueError("video must be uint8 [F,H0,W0,3]")
    F, H0, W0, _ = video.shape
    B, n_fr = len(starts), num_seq * seq_len
    if not 0 < vlen <= F:
        raise ValueError(f"a video of {F} frames cannot have length {vlen}")
    for b, st in enumerate(starts):   # the kernel trusts these
        if st < 0 or st + (n_fr - 1) * ds >= vlen:
            raise ValueError(f"window {b}: frames {st} .. {st + (n_fr - 1) * ds} do not fit a video of {vlen} frames")
    c = clip
    if c["x1"] < 0 or c["y1"] < 0 or c["x1"] + int((c["xb"][:, 0] + c["xb"][:, 1]).max()) > W0 or \
            c["y1"] + int((c["yb"][:, 0] + c["yb"][:, 1]).max()) > H0:
        raise ValueError(f"the crop box / resampling window leaves the {W0} x {H0} frame")
    if any(j.order[0] != 255 for j in c["jitter"]) or (np.asarray(c["gray"]) >= 0).any():
        raise ValueError("the windowed gather has no gray / jitter stage (the test recipe draws none)")
    dev = video.device
    aug = np.array([(st, c["x1"], c["y1"], c["flip"]) for st in starts], np.int32)
    rep = lambda a: torch.from_numpy(np.repeat(a[None].astype(np.int32), B, 0)).to(dev)   # noqa: E731  (the kernel indexes its tables by clip)
    t = dict(aug=torch.from_numpy(aug).to(dev), xb=rep(c["xb"]), xk=rep(c["xk"]), yb=rep(c["yb"]), yk=rep(c["yk"]))
    rs = L.Resample(t["xb"].data_ptr(), t["xk"].data_ptr(), t["yb"].data_ptr(), t["yk"].data_ptr(), c["xk"].shape[1], c["yk"].shape[1])
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    lib.call("dpc_video_windows_to_input", video.contiguous(), B, F, H0, W0, t["aug"], num_seq, seq_len, ds, size, size, C.byref(rs),
             mean, std, block, s2d, L.dtype_code(s2d.dtype) if s2d is not None else L.F32, lib.stream())
    return block, s2d


def recipe_to_input(lib: L.Lib, frames: torch.Tensor, starts, clips: "List[dict]", num_seq: int, seq_len: int, ds: int, size: int,
                    block: Optional[torch.Tensor] = None, s2d: Optional[torch.Tensor] = None):
    """frames u8 [B,F,H0,W0,3] on the kernels' device + one draw_k400 / draw_ucf101 result per clip -> block f32 [B,N,3,SL,size,size]
    and / or the stem's space-to-depth operand, through dpc_frames_to_input_ex.  starts[b] = first sampled frame of clip b."""
    B, F, H0, W0, ch = frames.shape
    n_fr = num_seq * seq_len
    if ch != 3 or frames.dtype != torch.uint8 or len(clips) != B:
        raise ValueError("frames must be uint8 [B,F,H0,W0,3] with one recipe draw per clip")
    dev = frames.device
    ksx = max(c["xk"].shape[1] for c in clips)
    ksy = max(c["yk"].shape[1] for c in clips)
    aug = np.zeros((B, 4), np.int32)
    xb, yb = np.zeros((B, size, 2), np.int32), np.zeros((B, size, 2), np.int32)
    xk, yk = np.zeros((B, size, ksx), np.int32), np.zeros((B, size, ksy), np.int32)
    gray = np.zeros((B, n_fr), np.int8)
    jit = (FrameJitter * (B * n_fr))()
    any_jitter = False
    for b, c in enumerate(clips):
        # host-side validation: the kernel trusts these: sampled frames inside the video, source windows inside the frame
        if starts[b] < 0 or starts[b] + (n_fr - 1) * ds >= F:
            raise ValueError(f"clip {b}: frames {starts[b]} .. {starts[b] + (n_fr - 1) * ds} do not fit a video of {F} frames")
        if c["x1"] < 0 or c["y1"] < 0 or c["x1"] + int((c["xb"][:, 0] + c["xb"][:, 1]).max()) > W0 or \
                c["y1"] + int((c["yb"][:, 0] + c["yb"][:, 1]).max()) > H0:
            raise ValueError(f"clip {b}: the crop box / resampling window leaves the {W0} x {H0} frame")
        aug[b] = (starts[b], c["x1"], c["y1"], c["flip"])
        xb[b], yb[b] = c["xb"], c["yb"]
        xk[b, :, :c["xk"].shape[1]] = c["xk"]
        yk[b, :, :c["yk"].shape[1]] = c["yk"]
        gray[b] = c["gray"]
        for i in range(n_fr):
            jit[b * n_fr + i] = c["jitter"][i]
            any_jitter |= c["jitter"][i].order[0] != 255
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(aug=aug, xb=xb, xk=xk, yb=yb, yk=yk, gray=gray).items()}
    rs = L.Resample(t["xb"].data_ptr(), t["xk"].data_ptr(), t["yb"].data_ptr(), t["yk"].data_ptr(), ksx, ksy)
    jt = u8 = ls = None
    if any_jitter:
        jt = torch.frombuffer(bytearray(bytes(jit)), dtype=torch.uint8).clone().to(dev)
        u8 = torch.empty(B * n_fr * size * size * 3, dtype=torch.uint8, device=dev)
        ls = torch.empty(B * n_fr, dtype=torch.int64, device=dev)
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    lib.call("dpc_frames_to_input_ex", frames.contiguous(), B, F, H0, W0, t["aug"], t["gray"], num_seq, seq_len, ds, size, size, C.byref(rs),
             jt, u8, ls, mean, std, block, s2d, L.dtype_code(s2d.dtype) if s2d is not None else L.F32, lib.stream())
    return block, s2d


# ------------------------------------------------------------------------------------------------------------------
# frames resident in HBM (`--resident`): packed store, the recipes as descriptors, their draws from given uniforms
# ------------------------------------------------------------------------------------------------------------------
_JITTER = dict(brightness=0.5, contrast=0.5, saturation=0.5, hue=0.25, p=1.0)
RECIPES = {   # dpc/main.py:114-132 as the fields of dpc_recipe_desc (include/dpc_hip.h); sized_p None = RandomCrop(crop) + NEAREST Scale
    "k400": dict(sized_p=1.0, flip_code=1, gray_p=0.5, jitter=_JITTER),
    "ucf101": dict(sized_p=None, flip_code=2, gray_p=0.5, jitter=_JITTER),
}
# The fine-tuning recipes (LC_RECIPES 'train' / 'val', eval/test.py:161-176) as descriptors: what they need beyond the pre-training
# ones are the two flags of dpc_draw_recipe_ex -- ColorJitter(consistent=True) (one draw, frame 0's slots, copied to every frame)
# and the NEAREST Scale((size, size)) behind the BILINEAR RandomSizedCrop(crop).  The test recipe draws nothing and needs no kernel.
RESIDENT_LC_RECIPES = {
    name: dict(sized_p=r["p"], flip_code=1, gray_p=None, jitter=r["jitter"], jitter_consistent=True, scale_after_sized=True)
    for name, r in LC_RECIPES.items() if name != "test"
}
SLOT_START, SLOT_FLIP, SLOT_SIZED_P, SLOT_CROP_X, SLOT_CROP_Y, SLOT_JITTER_P, SLOT_ATTEMPT, SLOT_FRAME = 0, 1, 2, 3, 4, 5, 8, 58
ATTEMPT_SLOTS, FRAME_SLOTS = 5, 9   # include/dpc_hip.h (dpc_draw_recipe) documents the layout
recipe_slots = L.recipe_slots


def recipe_desc(recipe) -> "L.RecipeDesc":
    r = RECIPES[recipe] if isinstance(recipe, str) else recipe
    j = r.get("jitter") or {}
    neg = lambda v: -1.0 if v is None else float(v)   # noqa: E731
    return L.RecipeDesc(neg(r.get("sized_p")), neg(r.get("gray_p")), float(j.get("p", 1.0)) if r.get("jitter") else -1.0,
                        float(j.get("brightness", 0)), float(j.get("contrast", 0)), float(j.get("saturation", 0)), float(j.get("hue", 0)),
                        int(r.get("flip_code", 0)), (L.RECIPE_JITTER_CONSISTENT if r.get("jitter_consistent") else 0) |
                        (L.RECIPE_SCALE_AFTER_SIZED if r.get("scale_after_sized") else 0))


def resident_ks(recipe, W0: int, H0: int, size: int, crop: Optional[int] = None) -> int:
    """pitch of the coefficient tables dpc_draw_recipe writes: the widest window any crop box of a W0 x H0 frame can need,
    2 ceil(max(W0, H0) / size) + 1 (resample_tables: ksize = 2 ceil(in / out) + 1 with in <= max(W0, H0)); an index map has one tap.
    A recipe with ``scale_after_sized`` resizes to `crop`, not to `size`: the same rule with `crop`"""
    r = RECIPES[recipe] if isinstance(recipe, str) else recipe
    if r.get("scale_after_sized"):
        if crop is None:
            raise ValueError("a recipe with scale_after_sized resizes to `crop`: pass it")
        size = crop
    return 1 if r.get("sized_p") is None else 2 * -(-max(W0, H0) // size) + 1


def recipe_from_uniforms(recipe, u, vlen: int, W0: int, H0: int, crop: int, size: int, n_frames: int, span: int):
    """The draws of one clip made from a given row of uniforms: u[slot] in [0, 1), ``recipe_slots(n_frames)`` of them in the slot
    layout of dpc_draw_recipe (include/dpc_hip.h), the decisions of ``draw_k400`` / ``draw_ucf101`` and of ``idx_sampler``
    (span = num_seq * seq_len * ds; the start is uniform on [0, vlen - span)).  randint(0, n) = floor(u (n + 1)), uniform(a, b) =
    a + (b - a) u, a rejected crop attempt keeps its slots: a pure function of the row, whichever branch is taken.  Returns the dict
    ``draw_k400`` returns plus ``start``.  csrc/recipe_draw.hip makes the same decisions with the same double arithmetic on the
    device (bit for bit, tests/resident_cases.py); fed to ``recipe_to_input`` it gives a --frames run the recipes of a --resident run.
    The two recipe keys of the classifier's recipes (RESIDENT_LC_RECIPES; tests/resident_lc_cases.py anchors them to ``draw_lc``):
    ``scale_after_sized``: RandomSizedCrop works at `crop` and the NEAREST Scale((size, size)) behind it picks rows
    ``nearest_tables(crop, size)`` of its tables; ``jitter_consistent``: one get_params draw, frame 0's slots, copied to every frame."""
    r = RECIPES[recipe] if isinstance(recipe, str) else recipe
    scale_after, consistent = bool(r.get("scale_after_sized")), bool(r.get("jitter_consistent"))
    if scale_after and r.get("sized_p") is None:
        raise ValueError("scale_after_sized is the Scale behind RandomSizedCrop: the recipe has none (sized_p is None)")
    pick, out_size = None, size
    if scale_after:                                             # everything up to the Scale happens at `crop`
        pick, size = (nearest_tables(crop, size) if crop != size else None), crop
    u = [float(v) for v in u]
    if len(u) != recipe_slots(n_frames):
        raise ValueError(f"{recipe_slots(n_frames)} uniforms per clip of {n_frames} frames, got {len(u)}")
    if vlen - span <= 0:
        raise ValueError("video too short (dataset_3d.py:87 drops it)")
    randint = lambda s, n: int(math.floor(u[s] * (n + 1)))   # noqa: E731
    uniform = lambda s, a, b: a + (b - a) * u[s]             # noqa: E731  (random.uniform)
    start = int(math.floor(u[SLOT_START] * (vlen - span)))
    code = int(r.get("flip_code", 0))
    flip = code if code and u[SLOT_FLIP] < 0.5 else 0
    ident = np.arange(size, dtype=np.int32)
    x1 = y1 = 0
    if r.get("sized_p") is None:                                # RandomCrop(crop) -> Scale((size, size)) [NEAREST]
        if crop > W0 or crop > H0:
            raise ValueError(f"RandomCrop({crop}) of {W0} x {H0} frames leaves the frame")
        if not (W0 == crop and H0 == crop):
            x1, y1 = randint(SLOT_CROP_X, W0 - crop), randint(SLOT_CROP_Y, H0 - crop)
        xt = _tables_from_index(nearest_tables(crop, size) if crop != size else ident)
        yt = (xt[0].copy(), xt[1].copy())
    elif u[SLOT_SIZED_P] < r["sized_p"]:                        # RandomSizedCrop (_draw_sized_crop with the uniforms of the slots)
        xt = None
        for a in range(10):
            s = SLOT_ATTEMPT + ATTEMPT_SLOTS * a
            target_area = uniform(s, 0.5, 1) * (W0 * H0)
            aspect = uniform(s + 1, 3. / 4, 4. / 3)
            w = int(round(math.sqrt(target_area * aspect)))
            h = int(round(math.sqrt(target_area / aspect)))
            if u[s + 2] < 0.5:
                w, h = h, w
            if w <= W0 and h <= H0:
                x1, y1 = randint(s + 3, W0 - w), randint(s + 4, H0 - h)
                xt, yt = resample_tables(w, size), resample_tables(h, size)
                break
        if xt is None:
            if W0 < H0:
                ow, oh = size, int(size * H0 / W0)
            else:
                oh, ow = size, int(size * W0 / H0)
            cx, cy = int(round((ow - size) / 2.)), int(round((oh - size) / 2.))
            xt, yt = resample_tables(W0, ow, cx, size), resample_tables(H0, oh, cy, size)
    else:                                                       # the failed `p` draw: CenterCrop(size)
        if W0 < size or H0 < size:
            raise ValueError(f"CenterCrop({size}) of {W0} x {H0} frames leaves the frame (PIL would pad with black; not reproduced)")
        x1, y1 = int(round((W0 - size) / 2.)), int(round((H0 - size) / 2.))
        xt, yt = _tables_from_index(ident), _tables_from_index(ident)
    if pick is not None:                                        # NEAREST Scale: a sub-sampled output is an exact subset of the rows
        xt, yt = (xt[0][pick], xt[1][pick]), (yt[0][pick], yt[1][pick])
    size = out_size
    gray = np.full(n_frames, -1, np.int8)
    jit = (FrameJitter * n_frames)()
    jitter, gray_p = r.get("jitter"), r.get("gray_p")
    jit_on = jitter is not None and u[SLOT_JITTER_P] < jitter.get("p", 1.0)
    for f in range(n_frames):
        s = SLOT_FRAME + FRAME_SLOTS * f
        if gray_p is not None and u[s] < gray_p:
            gray[f] = int(math.floor(u[s + 1] * 3))
        if consistent:
            s = SLOT_FRAME                                      # ColorJitter(consistent=True): every frame repeats frame 0's draw
        j = jit[f]
        j.order[:] = [255, 255, 255, 255]
        if not jit_on:
            continue
        ops: List[int] = []
        for op, name in enumerate(("brightness", "contrast", "saturation", "hue")):   # _jitter_get_params
            v = jitter.get(name, 0)
            if not v:
                continue
            lo, hi = (-v, v) if name == "hue" else (max(0.0, 1.0 - v), 1.0 + v)
            fac = uniform(s + 2 + op, lo, hi)
            if name == "hue":
                j.hue_shift = int(fac * 255) & 0xFF
            else:
                j.factor[op] = fac
            ops.append(op)
        for i in range(len(ops) - 1, 0, -1):                    # Fisher-Yates from the top, as random.shuffle walks
            q = int(math.floor(u[s + 6 + (3 - i)] * (i + 1)))
            ops[i], ops[q] = ops[q], ops[i]
        for k, op in enumerate(ops):
            j.order[k] = op
    return dict(start=start, x1=x1, y1=y1, flip=flip, xb=xt[0], xk=xt[1], yb=yt[0], yk=yt[1], gray=gray, jitter=jit)


def free_device_memory(device) -> int:
    """bytes of device memory still free (the one place FrameStore.to_device asks; tests replace it)"""
    device = torch.device(device)
    return int(torch.cuda.mem_get_info(device)[0]) if device.type == "cuda" else 1 << 62


def _load(a, mmap=False):
    if isinstance(a, (str, bytes)) or hasattr(a, "__fspath__"):
        return np.load(a, mmap_mode="r") if mmap else np.load(a)
    return a


class FrameStore:
    """Decoded videos of ANY length packed back to back: frames uint8 [total_frames, H0, W0, 3] and offsets int64 [videos + 1]
    (non-decreasing, offsets[0] == 0, offsets[-1] == total_frames), video v = frames[offsets[v]:offsets[v + 1]].  Built from such a
    packed array with its offsets (``--frames packed.npy --offsets offsets.npy``) or from the dense [clips, F, H0, W0, 3] array of
    ``FrameSource`` (every video F frames, offsets = arange(clips + 1) * F).  With the dense array ``lengths`` integer [clips] gives
    the real frame count of each video (<= F, the ``--lengths`` of dpc_amd.lc_main): a video then fills only the head of its slot.
    ``to_device`` uploads it ONCE; after that a training step reads its frames from HBM (dpc_store_to_input) and nothing crosses
    the host per step."""

    def __init__(self, frames, offsets=None, lengths=None):
        fr = _load(frames, mmap=True)
        if getattr(fr, "dtype", None) != np.uint8 or fr.ndim not in (4, 5) or fr.shape[-1] != 3:
            raise ValueError("--frames wants a uint8 array [clips, F, H0, W0, 3], or with --offsets a packed [total_frames, H0, W0, 3]")
        if lengths is not None and (offsets is not None or fr.ndim != 5):
            raise ValueError("--lengths goes with the dense 5-D --frames array [clips, F, H0, W0, 3]; with --offsets a packed store says "
                             "how long each video is: pass --lengths or --offsets, not both")
        self.lengths = None
        if lengths is not None:
            ln = np.asarray(_load(lengths))
            if ln.ndim != 1 or ln.shape[0] != fr.shape[0] or not np.issubdtype(ln.dtype, np.integer):
                raise ValueError(f"--lengths wants one integer per clip: {fr.shape[0]} clips, array of shape {ln.shape} and type {ln.dtype}")
            if ln.size and (int(ln.min()) < 0 or int(ln.max()) > fr.shape[1]):
                raise ValueError(f"lengths must lie in [0, {fr.shape[1]}] (the frames the array holds): found {int(ln.min())} .. {int(ln.max())}")
            self.lengths = ln.astype(np.int64)
        if fr.ndim == 5:
            if offsets is not None:
                raise ValueError("--offsets goes with a packed 4-D array [total_frames, H0, W0, 3]; this --frames array is the dense 5-D one")
            offsets = np.arange(fr.shape[0] + 1, dtype=np.int64) * fr.shape[1]
            fr = fr.reshape((-1,) + tuple(fr.shape[2:]))
        elif offsets is None:
            raise ValueError("a packed 4-D --frames array [total_frames, H0, W0, 3] needs --offsets (int64 [videos + 1]): the flag is missing")
        off = np.asarray(_load(offsets))
        if off.ndim != 1 or off.shape[0] < 2 or not np.issubdtype(off.dtype, np.integer):
            raise ValueError(f"--offsets wants integers [videos + 1], got shape {off.shape} and type {off.dtype}")
        off = off.astype(np.int64)
        if int(off[0]) != 0 or (np.diff(off) < 0).any():
            raise ValueError("--offsets must start at 0 and never decrease")
        if int(off[-1]) != fr.shape[0]:
            raise ValueError(f"--offsets ends at {int(off[-1])} but the store holds {fr.shape[0]} frames")
        self.frames, self.offsets = fr, off
        self.H0, self.W0 = int(fr.shape[1]), int(fr.shape[2])
        self.dev: Optional[torch.Tensor] = None
        self.offsets_dev: Optional[torch.Tensor] = None
        self.lengths_dev: Optional[torch.Tensor] = None

    def __len__(self):
        return self.offsets.shape[0] - 1

    @property
    def video_lengths(self) -> np.ndarray:
        """frames of each video: ``lengths`` when given, else what the offsets leave"""
        return self.lengths if self.lengths is not None else np.diff(self.offsets)

    @property
    def total_frames(self) -> int:
        return int(self.frames.shape[0])

    @property
    def nbytes(self) -> int:
        return self.total_frames * self.H0 * self.W0 * 3

    def long_enough(self, span: int) -> np.ndarray:
        """videos with vlen - span > 0, span = num_seq * seq_len * ds (dpc/dataset_3d.py:80-82 drops the others)"""
        return np.nonzero(self.video_lengths - span > 0)[0]

    def to_device(self, device, reserve: int = 0, chunk_bytes: int = 64 << 20):
        """one upload, in chunks through ONE pinned staging buffer (no second host copy of the store).  `reserve` = bytes the engine
        still has to allocate beside it.  Every rank calls this: each GPU holds a whole copy of the store."""
        device = torch.device(device)
        if self.dev is not None:
            if self.dev.device != device:
                raise ValueError(f"the store already lives on {self.dev.device}")
            return self
        free = free_device_memory(device)
        if self.nbytes + reserve > free:
            raise ValueError(f"the frame store needs {self.nbytes} bytes of device memory but only {free - reserve} are available "
                             f"({free} free, {reserve} still to be allocated by the engine): --resident holds every frame in HBM")
        dev = torch.empty((self.total_frames, self.H0, self.W0, 3), dtype=torch.uint8, device=device)
        flat, src, n = dev.view(-1), self.frames.reshape(-1), self.nbytes
        stage = torch.empty(max(1, min(chunk_bytes, n)), dtype=torch.uint8, pin_memory=device.type == "cuda")
        host = stage.numpy()
        for o in range(0, n, stage.numel()):
            m = min(stage.numel(), n - o)
            host[:m] = src[o:o + m]
            flat[o:o + m].copy_(stage[:m])   # blocking: the staging buffer is free again when it returns
        self.dev, self.offsets_dev = dev, torch.from_numpy(self.offsets).to(device)
        self.lengths_dev = torch.from_numpy(self.lengths).to(device) if self.lengths is not None else None
        return self


class ResidentFrameSource:
    """``FrameSource`` for a store that lives in HBM (``python -m dpc_amd.main --frames ... --resident``).  The epoch order stays
    on the host (``torch.randperm``, as RandomSampler); ONCE per epoch this rank's slice of it, int32 [steps * B] video indices,
    is copied into a device buffer of fixed size and a device cursor is zeroed.  Per step ``BackboneEngine.load_resident``
    advances the cursor and the draw counter, draws the recipe on the device (dpc_draw_recipe: Philox stream 4 keyed by `seed`
    and the draw counter -- NOT the draws of Python's ``random``: a different, equally distributed sample than ``FrameSource``
    makes) and gathers (dpc_store_to_input): no host synchronisation, no copy, no allocation, no address that changes, so one
    captured step serves every epoch.  Every rank holds the WHOLE store (any rank may draw any video): one copy per GPU.
    The draw counter is not part of a checkpoint (the engine keeps none of its counters there): a resumed run sets it from the
    steps already taken (``set_draw``), which is what it would have been."""

    def __init__(self, store: FrameStore, dataset: str, num_seq: int, seq_len: int, ds: int, size: int, batch: int, device, rank: int = 0,
                 world: int = 1, crop: int = 224, seed: int = 0):
        if dataset not in RECIPES:
            raise ValueError("dataset not supported")   # dpc/main.py:301
        # dpc/main.py:294, :299: k400 samples every 5th frame; dpc/main.py:117: only the ucf101 recipe crops before it scales
        self._fields(store, dataset, num_seq, seq_len, 5 if dataset == "k400" else ds, size, batch, device, rank, world,
                     crop if dataset == "ucf101" else size, seed)
        if dataset == "ucf101" and (store.H0 < crop or store.W0 < crop):
            raise ValueError(f"the ucf101 recipe crops {crop} x {crop} (dpc/main.py:117): frames of {store.W0} x {store.H0} are too small")
        self._tables(dataset)

    def _fields(self, store, dataset, num_seq, seq_len, ds, size, batch, device, rank, world, crop, seed):
        """what every resident source is made of (the one place its fields are set); `device` must be where the store lives"""
        if store.dev is None:
            raise ValueError("upload the store first (FrameStore.to_device)")
        if torch.device(device).type != store.dev.device.type:
            raise ValueError(f"the store lives on {store.dev.device}, the source was asked for {device}")
        self.store, self.dataset, self.N, self.SL, self.size, self.batch, self.rank, self.world = store, dataset, num_seq, seq_len, size, batch, rank, world
        self.ds, self.n_fr, self.crop, self.seed = ds, num_seq * seq_len, crop, int(seed) & 0xFFFFFFFFFFFFFFFF
        self.device = store.dev.device
        self.labels_dev: Optional[torch.Tensor] = None

    def _tables(self, recipe):
        """drop the videos too short for one clip, then this source's device tables: the epoch's video indices, the two counters and
        what dpc_draw_recipe writes for one batch"""
        store, num_seq, seq_len, batch, world, size = self.store, self.N, self.SL, self.batch, self.world, self.size
        H0, W0 = store.H0, store.W0
        self.keep = store.long_enough(self.n_fr * self.ds)
        self.skipped = len(store) - len(self.keep)
        if len(self.keep) == 0:
            raise ValueError(f"every one of the {len(store)} videos is too short for {num_seq} x {seq_len} frames at stride {self.ds} "
                             "(dpc/dataset_3d.py:80-82 drops such videos)")
        if len(self) == 0:
            raise ValueError(f"{len(self.keep)} videos do not fill one batch of {batch} x {world}")
        dev = self.device
        B, n_fr = batch, self.n_fr
        self.desc = recipe_desc(recipe)
        self.KS = resident_ks(recipe, W0, H0, size, self.crop)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
        self.perm, self.cursor, self.draw = z(len(self) * B, torch.int32), z(1, torch.int32), z(1, torch.int32)
        self.aug, self.clip_first, self.gray = z((B, 4), torch.int32), z(B, torch.int64), z((B, n_fr), torch.int8)
        self.jitter = z(B * n_fr * C.sizeof(FrameJitter), torch.uint8)
        self.xb, self.yb = z((B, size, 2), torch.int32), z((B, size, 2), torch.int32)
        self.xk, self.yk = z((B, size, self.KS), torch.int32), z((B, size, self.KS), torch.int32)
        self.scale_tab = torch.from_numpy(nearest_tables(self.crop, size)).to(dev) if self.crop != size else None
        self.rs = L.Resample(self.xb.data_ptr(), self.xk.data_ptr(), self.yb.data_ptr(), self.yk.data_ptr(), self.KS, self.KS)
        self.has_jitter = self.desc.jitter_p >= 0

    def __len__(self):   # batches per epoch, drop_last
        return len(self.keep) // (self.batch * self.world)

    def set_draw(self, steps: int):
        """a resumed run: the draw counter after `steps` steps of this source"""
        self.draw.fill_(int(steps))

    def begin_epoch(self) -> np.ndarray:
        """a new permutation: this rank's video indices int32 [steps, B] go to the device buffer, the cursor to 0"""
        order = self.keep[torch.randperm(len(self.keep)).numpy()]     # RandomSampler: torch's generator, seeded by torch.manual_seed(0)
        gb, B = self.batch * self.world, self.batch
        mine = np.stack([order[i * gb + self.rank * B: i * gb + (self.rank + 1) * B] for i in range(len(self))]).astype(np.int32)
        self.perm.copy_(torch.from_numpy(mine.reshape(-1)))
        self.cursor.zero_()
        return mine

    def draw_recipe(self, lib: L.Lib, uniforms: Optional[torch.Tensor] = None, video_idx: Optional[torch.Tensor] = None, call=None,
                    target: Optional[torch.Tensor] = None):
        """dpc_draw_recipe into this source's tables for the batch the cursor points at (video_idx given: that batch, cursor unused).
        A store with ``lengths`` or a source with labels goes through dpc_draw_recipe_ex: the same launch reads each video's length
        from the device table and writes ``target[b] = labels[video of clip b]`` (int64 [B]; None: the labels are not gathered)"""
        st = self.store
        head = (C.byref(self.desc), self.perm if video_idx is None else video_idx, self.cursor if video_idx is None else None, st.offsets_dev)
        tail = (self.batch, st.W0, st.H0, self.crop, self.size, self.N, self.SL, self.ds, self.KS, self.scale_tab, self.seed, self.draw,
                uniforms, self.aug, self.clip_first, self.gray, self.jitter, self.xb, self.xk, self.yb, self.yk)
        if target is not None and (self.labels_dev is None or target.dtype != torch.int64 or tuple(target.shape) != (self.batch,)
                                   or target.device != self.device or not target.is_contiguous()):
            raise ValueError(f"target: a contiguous int64 [{self.batch}] on {self.device}, for a source that carries labels")
        if st.lengths_dev is None and self.labels_dev is None:
            name, args = "dpc_draw_recipe", head + tail
        else:
            name, args = "dpc_draw_recipe_ex", head + (st.lengths_dev, self.labels_dev if target is not None else None) + tail + (target,)
        if call is not None:
            return call(name, *args)
        return lib.call(name, *args, lib.stream())


class ResidentLabelledSource(ResidentFrameSource):
    """``LabelledFrameSource`` for a store that lives in HBM (``python -m dpc_amd.lc_main --frames ... --labels ... --resident``):
    the fine-tuning recipes of eval/test.py:161-176 as RESIDENT_LC_RECIPES, drawn on the device like the pre-training ones
    (``ResidentFrameSource``; the same Philox stream and slots, so again NOT the draws of Python's ``random``: a different, equally
    distributed sample than ``LabelledFrameSource`` makes), and the labels, uploaded once, gathered by the draw's own launch into
    the engine's ``target``.  recipe 'test' draws nothing: ``videos()`` walks the store in file order for the video-level protocols
    and hands out DEVICE slices of it, so no video is uploaded again."""

    def __init__(self, store: FrameStore, labels, dataset: str, num_seq: int, seq_len: int, ds: int, size: int, batch: int, num_class: int,
                 device, recipe: str = "train", rank: int = 0, world: int = 1, crop: int = 224, seed: int = 0):
        if dataset not in ("ucf101", "hmdb51"):
            raise ValueError("dataset not supported")   # eval/test.py:378
        if recipe not in LC_RECIPES:
            raise ValueError(f"recipe must be one of {sorted(LC_RECIPES)}")
        self._fields(store, dataset, num_seq, seq_len, ds, size, batch, device, rank, world, crop, seed)
        labels = np.asarray(_load(labels))
        if labels.ndim != 1 or labels.shape[0] != len(store) or not np.issubdtype(labels.dtype, np.integer):
            raise ValueError(f"--labels wants one integer per clip: {len(store)} clips, array of shape {labels.shape} and type {labels.dtype}")
        if labels.size and (int(labels.min()) < 0 or int(labels.max()) >= num_class):
            raise ValueError(f"labels must lie in [0, {num_class}): found {int(labels.min())} .. {int(labels.max())}")
        if store.H0 < crop or store.W0 < crop:
            raise ValueError(f"the recipes crop {crop} x {crop} (eval/test.py:122,162,170): frames of {store.W0} x {store.H0} are too small")
        self.recipe, self.num_class, self.labels = recipe, num_class, labels.astype(np.int64)
        self.labels_dev = torch.from_numpy(self.labels).to(self.device)
        if recipe == "test":   # no batches, no draws: the file order of videos()
            self.keep = store.long_enough(self.n_fr * ds)
            self.skipped = len(store) - len(self.keep)
        else:
            self._tables(RESIDENT_LC_RECIPES[recipe])

    def videos(self):
        """``LabelledFrameSource.videos`` without the upload: (index, frames u8 [vlen, H0, W0, 3] -- a slice of the store ON THE DEVICE
        --, label, window starts, the test recipe's draw) for every video long enough"""
        st = self.store
        lengths = st.video_lengths
        for ci in self.keep.tolist():
            first, vlen = int(st.offsets[ci]), int(lengths[ci])
            starts = lc_test_windows(vlen, self.N, self.SL, self.ds, self.dataset)
            yield ci, st.dev[first:first + vlen], int(self.labels[ci]), starts, draw_lc(st.W0, st.H0, self.crop, self.size, self.n_fr, "test")


def store_to_input(lib: L.Lib, store: torch.Tensor, aug: torch.Tensor, clip_first: torch.Tensor, gray: Optional[torch.Tensor], rs,
                   jitter: Optional[torch.Tensor], num_seq: int, seq_len: int, ds: int, size: int, block: Optional[torch.Tensor] = None,
                   s2d: Optional[torch.Tensor] = None, u8_ws: Optional[torch.Tensor] = None, lsum_ws: Optional[torch.Tensor] = None, call=None):
    """dpc_store_to_input: store u8 [total_frames,H0,W0,3] and the device tables of one batch (aug int32 [B,4], clip_first int64 [B],
    gray int8 [B,N*SL] or None, rs = L.Resample over [B] tables or None, jitter = dpc_frame_jitter bytes or None with its two
    workspaces) -> block and / or the stem's operand.  The tables are trusted: dpc_draw_recipe wrote them."""
    if store.dim() != 4 or store.shape[3] != 3 or store.dtype != torch.uint8 or not store.is_contiguous():
        raise ValueError("store must be contiguous uint8 [total_frames,H0,W0,3]")
    B = aug.shape[0]
    if aug.dtype != torch.int32 or tuple(aug.shape) != (B, 4) or clip_first.dtype != torch.int64 or tuple(clip_first.shape) != (B,):
        raise ValueError("aug int32 [B,4], clip_first int64 [B]")
    n_fr = num_seq * seq_len
    if jitter is not None and (u8_ws is None or lsum_ws is None or u8_ws.numel() < B * n_fr * size * size * 3 or lsum_ws.numel() < B * n_fr):
        raise ValueError("jitter needs u8_ws (B*N*SL*size*size*3 bytes) and lsum_ws (B*N*SL int64)")
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    args = (store, B, store.shape[0], store.shape[1], store.shape[2], aug, gray, num_seq, seq_len, ds, size, size,
            C.byref(rs) if rs is not None else None, jitter, u8_ws if jitter is not None else None, lsum_ws if jitter is not None else None,
            mean, std, block, s2d, L.dtype_code(s2d.dtype) if s2d is not None else L.F32, clip_first)
    if call is not None:
        call("dpc_store_to_input", *args)
    else:
        lib.call("dpc_store_to_input", *args, lib.stream())
    return block, s2d


class FrameSource:
    """Decoded clips as ONE uint8 array [clips, F, H0, W0, 3] (``np.load(path, mmap_mode='r')`` or an array) -- the data source of
    ``python -m dpc_amd.main --frames``.  It stands where the reference has ``dataset[index]`` under
    ``DataLoader(RandomSampler(dataset), batch_size, drop_last=True)`` (dpc/dataset_3d.py:88-111, dpc/main.py:304-313): per
    epoch a random permutation of the clips cut into batches (the last partial one dropped); per clip the start frame of
    ``idx_sampler`` (``np.random.choice(range(vlen - num_seq * seq_len * ds), 1)``, dataset_3d.py:88-92) and then the draws of the
    training transform (``draw_k400`` / ``draw_ucf101``: the ``Compose`` of dpc/main.py:114-132, same ``random`` / ``np.random``
    calls in the same order).  What it hands out is NOT a float tensor: the uint8 frames the clip needs (its span of
    (num_seq * seq_len - 1) * ds + 1 frames) and the draws; ``DPCEngine.load_recipe`` runs crop / resize / flip / grey / jitter /
    ToTensor / Normalize / layout on the GPU and fills the stem's operand.  Readers of video files are out of scope (SURVEY section 2
    row 8); anything that can produce this array (a decoder, a frame cache) plugs in here."""

    def __init__(self, frames, dataset: str, num_seq: int, seq_len: int, ds: int, size: int, batch: int, rank: int = 0, world: int = 1,
                 crop: int = 224):
        self.frames = np.load(frames, mmap_mode="r") if isinstance(frames, (str, bytes)) or hasattr(frames, "__fspath__") else frames
        fr = self.frames
        if fr.ndim != 5 or fr.shape[4] != 3 or fr.dtype != np.uint8:
            raise ValueError("--frames wants a uint8 array [clips, F, H0, W0, 3]")
        if dataset not in ("k400", "ucf101"):
            raise ValueError("dataset not supported")   # dpc/main.py:301
        self.dataset, self.N, self.SL, self.size, self.batch, self.rank, self.world, self.crop = dataset, num_seq, seq_len, size, batch, rank, world, crop
        self.ds = 5 if dataset == "k400" else ds           # dpc/main.py:294 (k400: downsample=5), :299 (ucf101: args.ds)
        self.n_fr = num_seq * seq_len
        self.span = (self.n_fr - 1) * self.ds + 1
        if fr.shape[1] - self.n_fr * self.ds <= 0:
            raise ValueError(f"clips of {fr.shape[1]} frames are too short for {num_seq} x {seq_len} frames at stride {self.ds} "
                             "(dpc/dataset_3d.py:80-82 drops such videos)")
        if dataset == "ucf101" and (fr.shape[2] < crop or fr.shape[3] < crop):
            raise ValueError(f"the ucf101 recipe crops {crop} x {crop} (dpc/main.py:117): frames of {fr.shape[3]} x {fr.shape[2]} are too small")

    def __len__(self):   # batches per epoch, drop_last
        return self.frames.shape[0] // (self.batch * self.world)

    def epoch(self, device):
        """yields (frames u8 [B, span, H0, W0, 3] on `device`, starts (all 0: the span is cut out on the host), clips) per batch of THIS rank"""
        fr = self.frames
        F, H0, W0 = fr.shape[1:4]
        order = torch.randperm(fr.shape[0]).tolist()     # RandomSampler: torch's generator, seeded by torch.manual_seed(0) (dpc/main.py:50)
        gb = self.batch * self.world
        for i in range(len(self)):
            mine = order[i * gb + self.rank * self.batch: i * gb + (self.rank + 1) * self.batch]
            clips, host = [], np.empty((self.batch, self.span, H0, W0, 3), np.uint8)
            for j, ci in enumerate(mine):
                start = int(np.random.choice(range(F - self.n_fr * self.ds), 1)[0])         # idx_sampler
                host[j] = fr[ci, start:start + self.span]
                clips.append(draw_k400(W0, H0, self.size, self.n_fr) if self.dataset == "k400"
                             else draw_ucf101(W0, H0, self.crop, self.size, self.n_fr))
            yield torch.from_numpy(host).to(device, non_blocking=False), [0] * self.batch, clips


class LabelledFrameSource:
    """Labelled videos for ``python -m dpc_amd.lc_main --frames``: frames uint8 [clips, F, H0, W0, 3], labels integer [clips] (0-based
    class ids), optional lengths integer [clips] (the real frame count of each video, <= F; default F).  It stands where the
    reference has ``UCF101_3d`` / ``HMDB51_3d`` (eval/dataset_3d_lc.py) under its DataLoaders (eval/test.py:345-380): for
    'train' / 'val' a random permutation cut into batches (drop_last), per clip the start frame of ``idx_sampler``
    (``np.random.choice(range(vlen - num_seq * seq_len * ds))``, :79) and then the draws of ``draw_lc``; for the test protocol
    ``videos()`` walks the file in order.  Videos too short for one clip are dropped, as the dataset classes do (:61-67)."""

    def __init__(self, frames, labels, dataset: str, num_seq: int, seq_len: int, ds: int, size: int, batch: int, num_class: int,
                 recipe: str = "train", lengths=None, rank: int = 0, world: int = 1, crop: int = 224):
        self.frames = np.load(frames, mmap_mode="r") if isinstance(frames, (str, bytes)) or hasattr(frames, "__fspath__") else frames
        fr = self.frames
        if fr.ndim != 5 or fr.shape[4] != 3 or fr.dtype != np.uint8:
            raise ValueError("--frames wants a uint8 array [clips, F, H0, W0, 3]")
        if dataset not in ("ucf101", "hmdb51"):
            raise ValueError("dataset not supported")   # eval/test.py:378
        if recipe not in LC_RECIPES:
            raise ValueError(f"recipe must be one of {sorted(LC_RECIPES)}")
        load = lambda a: np.load(a) if isinstance(a, (str, bytes)) or hasattr(a, "__fspath__") else np.asarray(a)  # noqa: E731
        labels = load(labels)
        lengths = np.full(fr.shape[0], fr.shape[1], np.int64) if lengths is None else load(lengths)
        for name, a in (("labels", labels), ("lengths", lengths)):
            if a.ndim != 1 or a.shape[0] != fr.shape[0] or not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"--{name} wants one integer per clip: {fr.shape[0]} clips, array of shape {a.shape} and type {a.dtype}")
        if labels.size and (int(labels.min()) < 0 or int(labels.max()) >= num_class):
            raise ValueError(f"labels must lie in [0, {num_class}): found {int(labels.min())} .. {int(labels.max())}")
        if lengths.size and (int(lengths.min()) < 0 or int(lengths.max()) > fr.shape[1]):
            raise ValueError(f"lengths must lie in [0, {fr.shape[1]}] (the frames the array holds): found {int(lengths.min())} .. {int(lengths.max())}")
        if fr.shape[2] < crop or fr.shape[3] < crop:
            raise ValueError(f"the recipes crop {crop} x {crop} (eval/test.py:122,162,170): frames of {fr.shape[3]} x {fr.shape[2]} are too small")
        self.labels, self.lengths = labels.astype(np.int64), lengths.astype(np.int64)
        self.dataset, self.N, self.SL, self.ds, self.size, self.batch = dataset, num_seq, seq_len, ds, size, batch
        self.rank, self.world, self.crop, self.recipe, self.num_class = rank, world, crop, recipe, num_class
        self.n_fr = num_seq * seq_len
        self.span = (self.n_fr - 1) * ds + 1
        self.keep = [i for i in range(fr.shape[0]) if int(self.lengths[i]) - self.n_fr * ds > 0]
        self.skipped = fr.shape[0] - len(self.keep)

    def __len__(self):   # batches per epoch, drop_last
        return len(self.keep) // (self.batch * self.world)

    def epoch(self, device):
        """yields (frames u8 [B, span, H0, W0, 3] on `device`, starts (all 0: the span is cut out on the host), clips, labels int64 [B])
        per batch of THIS rank"""
        fr = self.frames
        H0, W0 = fr.shape[2:4]
        order = [self.keep[i] for i in torch.randperm(len(self.keep)).tolist()]     # RandomSampler
        gb = self.batch * self.world
        for i in range(len(self)):
            mine = order[i * gb + self.rank * self.batch: i * gb + (self.rank + 1) * self.batch]
            clips, host = [], np.empty((self.batch, self.span, H0, W0, 3), np.uint8)
            for j, ci in enumerate(mine):
                start = int(np.random.choice(range(int(self.lengths[ci]) - self.n_fr * self.ds), 1)[0])         # idx_sampler
                host[j] = fr[ci, start:start + self.span]
                clips.append(draw_lc(W0, H0, self.crop, self.size, self.n_fr, self.recipe))
            yield torch.from_numpy(host).to(device, non_blocking=False), [0] * self.batch, clips, torch.from_numpy(self.labels[mine])

    def videos(self):
        """the test protocol, in file order: (index, frames u8 [vlen, H0, W0, 3] host array, label, window starts, the test recipe's
        draw) for every video long enough (``skipped`` counts the others)"""
        fr = self.frames
        H0, W0 = fr.shape[2:4]
        for ci in self.keep:
            vlen = int(self.lengths[ci])
            starts = lc_test_windows(vlen, self.N, self.SL, self.ds, self.dataset)
            yield ci, fr[ci, :vlen], int(self.labels[ci]), starts, draw_lc(W0, H0, self.crop, self.size, self.n_fr, "test")
