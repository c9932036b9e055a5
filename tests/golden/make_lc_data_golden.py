"""Generate tests/golden/lc_data.npz by running THE REFERENCE'S OWN classes: the three transform pipelines of the downstream
classifier (eval/test.py:121-126 test, :161-168 train, :169-176 val; utils/augmentation.py) and the test-mode `__getitem__` of
its dataset classes (eval/dataset_3d_lc.py:85-138 UCF101_3d, :214-268 HMDB51_3d).

Runs only in the build container (needs /root/reference and PIL); reuses the torchvision stand-in of make_aug_golden.py by
importing it.  The frames are the 14 frames already stored in aug.npz (not stored again), the geometry is aug.npz's (crop 44
for the reference's 224, img_dim 24, N 2, SL 2, ds 3, start 1).

What is stored:
  * `<recipe>::<seed>` f32 [N, 3, SL, H, W] for recipe in train / val / test: the Compose output under random.seed(s);
    np.random.seed(s).  `seeds::<recipe>` lists the seeds, `branches::<recipe>` int8 [seeds, 3] what the reference's classes did
    (sized crop taken, flipped, jitter drawn), observed from thin wrappers around their methods.  The seeds are picked from 1..16 so
    that every branch a recipe has appears at least twice on either side (asserted below).  The test recipe draws nothing that
    changes its output (p = 0.0, no flip, no jitter): its eight clips are equal, which is the point.
  * `item::<name>` f32 [windows, N, 3, SL, H, W]: `dataset[0]` in mode 'test' on a longer video derived from aug.npz's frames by
    `long_video` below (the test holds the same expression), `item_params::<name>` = (vlen, N, SL, ds).  The dataset objects are
    made with object.__new__ (their __init__ reads csv files), `video_info` is a two-line shim, `pil_loader` serves frames from
    the array, `cv2` (imported, never used) is an empty module.

usage:  python tests/golden/make_lc_data_golden.py
"""
import itertools
import os
import random
import sys
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_aug_golden as G  # noqa: E402  (installs the torchvision stand-in, imports the reference's augmentation as G.A)

A, tvt, REF = G.A, G.tvt, G.REF
MAX_BYTES = 439379   # aug.npz, the largest fixture committed so far


def long_video(frames, F):
    """a longer video from aug.npz's 14 frames: the frames, their 180-degree rotation, a column roll -- cut to F"""
    return np.concatenate([frames, frames[:, ::-1, ::-1], np.roll(frames, 7, axis=2)])[:F].copy()


def recipe(mode, crop, size):
    if mode == "train":      # eval/test.py:161-168
        return tvt.Compose([A.RandomSizedCrop(consistent=True, size=crop, p=1.0), A.Scale(size=(size, size)), A.RandomHorizontalFlip(consistent=True),
                            A.ColorJitter(brightness=0.5, contrast=0.5, saturation=0.5, hue=0.25, p=0.3, consistent=True), A.ToTensor(), A.Normalize()])
    if mode == "val":        # eval/test.py:169-176
        return tvt.Compose([A.RandomSizedCrop(consistent=True, size=crop, p=0.3), A.Scale(size=(size, size)), A.RandomHorizontalFlip(consistent=True),
                            A.ColorJitter(brightness=0.2, contrast=0.2, saturation=0.2, hue=0.1, p=0.3, consistent=True), A.ToTensor(), A.Normalize()])
    return tvt.Compose([A.RandomSizedCrop(consistent=True, size=crop, p=0.0), A.Scale(size=(size, size)), A.ToTensor(), A.Normalize()])   # :121-126


# ---- what the reference's classes did, observed from outside -------------------------------------------------------------------
SEEN = {}


def _watch():
    cc, fl, gp = A.CenterCrop.__call__, A.RandomHorizontalFlip.__call__, A.ColorJitter.get_params

    def center(self, imgmap):
        SEEN["center"] = True
        return cc(self, imgmap)

    def flip(self, imgmap):
        out = fl(self, imgmap)
        SEEN["flip"] = out is not imgmap
        return out

    def params(*a):
        SEEN["jitter"] = True
        return gp(*a)

    A.CenterCrop.__call__, A.RandomHorizontalFlip.__call__, A.ColorJitter.get_params = center, flip, staticmethod(params)


def run_recipe(mode, frames, idx, N, SL, crop, size, seed):
    random.seed(seed)
    np.random.seed(seed)
    SEEN.clear()
    out = G.run_reference(recipe(mode, crop, size), frames, idx, N, SL).numpy()
    return out, (0 if SEEN.get("center") else 1, int(SEEN.get("flip", False)), int(SEEN.get("jitter", False)))


def covered(flags, mode):
    f = np.array(flags)
    need = {"train": (1, 2), "val": (0, 1, 2), "test": ()}[mode]   # train always takes the sized crop; test has no branch
    return all((f[:, k] == 1).sum() >= 2 and (f[:, k] == 0).sum() >= 2 for k in need)


# ---- the dataset classes in test mode -------------------------------------------------------------------------------------------
class _Info:
    """video_info.iloc[index] -> (vpath, vlen)"""

    def __init__(self, row):
        self.iloc = [row]


def dataset_item(cls_name, video, vlen, N, SL, ds, crop, size):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, f"{REF}/eval")
    import dataset_3d_lc as D
    D.pil_loader = lambda path: Image.fromarray(video[int(os.path.basename(path)[6:11]) - 1])   # 'image_%05d.jpg' % (i + 1)
    ds_obj = object.__new__(getattr(D, cls_name))
    ds_obj.mode, ds_obj.transform, ds_obj.seq_len, ds_obj.num_seq, ds_obj.downsample = "test", recipe("test", crop, size), SL, N, ds
    ds_obj.video_info = _Info(("root/Archery/v_Archery_g01_c01/", vlen))
    ds_obj.action_dict_encode = {"Archery": 2}
    t_seq, label = ds_obj[0]
    assert int(label) == 2
    return t_seq.numpy()


def main():
    g = np.load(os.path.join(HERE, "aug.npz"))
    frames = g["frames"]
    F, H0, W0, N, SL, ds, size, crop, start = (int(v) for v in g["params"])
    idx = (np.arange(N)[:, None] * ds * SL + start + np.arange(SL)[None, :] * ds).reshape(-1)
    _watch()
    out = {}
    for mode, n_keep in (("train", 8), ("val", 8), ("test", 8)):
        runs = {s: run_recipe(mode, frames, idx, N, SL, crop, size, s) for s in range(1, 17)}
        pick = next(c for c in itertools.combinations(range(1, 17), n_keep) if covered([runs[s][1] for s in c], mode))
        for s in pick:
            out[f"{mode}::{s}"] = runs[s][0]
        out[f"seeds::{mode}"] = np.array(pick, np.int32)
        out[f"branches::{mode}"] = np.array([runs[s][1] for s in pick], np.int8)
        print(mode, "seeds", pick, "branches (sized crop, flip, jitter)", [runs[s][1] for s in pick])
    FL = 42
    video = long_video(frames, FL)
    out["item_F"] = np.array([FL], np.int32)
    for name, cls_name, vlen, n, sl, d in (("ucf101", "UCF101_3d", 42, 2, 2, 3), ("hmdb51", "HMDB51_3d", 42, 4, 1, 3), ("short", "UCF101_3d", 29, 2, 2, 3)):
        item = dataset_item(cls_name, video, vlen, n, sl, d, crop, size)
        out[f"item::{name}"] = item
        out[f"item_params::{name}"] = np.array([vlen, n, sl, d], np.int32)
        print(name, "item", item.shape)
    path = os.path.join(HERE, "lc_data.npz")
    np.savez_compressed(path, **out)
    nbytes = os.path.getsize(path)
    print("wrote", path, nbytes, "bytes")
    assert nbytes <= MAX_BYTES, "drop seeds before shrinking geometry"


if __name__ == "__main__":
    main()
