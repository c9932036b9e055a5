"""The data kernels of a --resident step alone (docs/design_parts/10_beyond.md, "Resident frames"): the draw kernel
(dpc_draw_recipe) and the gather launches (dpc_store_to_input), timed by events around --calls calls after a warm-up, and their
share of the whole resident train step (load_resident + train_step on a replayed hipGraph).

    python scripts/data_bench.py --dataset k400 --B 128 --size 128 --W0 340 --H0 256
    python scripts/data_bench.py --dataset lc --B 32 --W0 320 --H0 240 [--train_what head]   # the classifier's train recipe (lc_main --resident):
                                                                         # dpc_draw_recipe_ex with the label gather, LCEngine's step
    python scripts/data_bench.py --make-array clips.npy --clips 128      # the dense k400 array the entry measurements read

Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def random_frames(shape, seed=0):
    n = int(np.prod(shape))
    return np.frombuffer(np.random.Generator(np.random.PCG64(seed)).bytes(n), np.uint8).reshape(shape)


def timed(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="k400", choices=["k400", "ucf101", "lc"])
    ap.add_argument("--net", default="resnet18")
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--W0", type=int, default=340)
    ap.add_argument("--H0", type=int, default=256)
    ap.add_argument("--frames_per_video", type=int, default=201)
    ap.add_argument("--videos", type=int, default=0, help="default: one batch")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--make-array", default="", help="write a dense uint8 [clips, F, H0, W0, 3] array here and exit")
    ap.add_argument("--clips", type=int, default=128)
    ap.add_argument("--train_what", default="all", choices=["all", "head"], help="--dataset lc: the whole model or the linear probe")
    ap.add_argument("--crop", type=int, default=224)
    a = ap.parse_args()
    if a.make_array:
        out = np.lib.format.open_memmap(a.make_array, mode="w+", dtype=np.uint8, shape=(a.clips, a.frames_per_video, a.H0, a.W0, 3))
        for i in range(a.clips):
            out[i] = random_frames(out.shape[1:], i)
        out.flush()
        print(json.dumps({"array": a.make_array, "shape": list(out.shape), "GB": out.nbytes / 1e9}))
        return
    from dpc_amd import data as D
    from dpc_amd.engine import DPCEngine
    from dpc_amd.model import DPC_RNN
    dev = torch.device("cuda:0")
    cdt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    N, SL, pred = 8, 5, 3
    lc = a.dataset == "lc"
    if lc:
        from dpc_amd.lc import LC, LCEngine
        eng = LCEngine(a.net, a.size, N, SL, a.B, dev, cdt, lr=1e-3, wd=1e-3, dropout=0.5, num_class=101, seed=666)
        eng.load_params({k: v.detach() for k, v in LC(a.size, N, SL, a.net, 0.5, 101, seed=0).state_dict().items()})
        if a.train_what == "head":
            eng.set_param_groups([{"params": [k for k in eng.offsets if k.startswith(("final_bn.", "final_fc."))], "lr": 1e-3, "weight_decay": 1e-3}])
    else:
        eng = DPCEngine(a.net, a.size, N, SL, pred, a.B, dev, cdt, seed=233)
        eng.load_params({k: v.detach() for k, v in DPC_RNN(a.size, N, SL, pred, a.net, seed=0).named_parameters()})
    videos = a.videos or a.B
    one = random_frames((a.frames_per_video, a.H0, a.W0, 3))
    frames = np.tile(one, (videos, 1, 1, 1))   # every video the same bytes: the kernels' time does not depend on them
    store = D.FrameStore(frames, np.arange(videos + 1, dtype=np.int64) * a.frames_per_video).to_device(dev, reserve=eng.resident_reserve())
    if lc:
        src = D.ResidentLabelledSource(store, np.arange(videos) % 101, "ucf101", N, SL, 3, a.size, a.B, 101, dev, "train", crop=a.crop, seed=1)
    else:
        src = D.ResidentFrameSource(store, a.dataset, N, SL, 3, a.size, a.B, dev, crop=a.crop, seed=1)
    src.begin_epoch()
    src.cursor.fill_(1)
    u8 = torch.empty(a.B * N * SL * a.size * a.size * 3, dtype=torch.uint8, device=dev)
    ls = torch.empty(a.B * N * SL, dtype=torch.int64, device=dev)

    def draw():
        src.draw_recipe(eng.lib, target=eng.target if lc else None)

    def gather():
        D.store_to_input(eng.lib, store.dev, src.aug, src.clip_first, src.gray, src.rs, src.jitter, N, SL, src.ds, a.size, None, eng.x_s2d, u8, ls)

    train = (lambda: eng.train_step(None, None)) if lc else (lambda: eng.train_step(None))

    def refill():   # the step's own sequence, with the cursor held on the first batch
        eng.load_resident(src)
        src.cursor.fill_(0)

    ms_draw, ms_gather = timed(draw, a.calls), timed(gather, a.calls)
    for _ in range(2):
        refill()
        train()
    step = eng.capture_train_step(None, warmup=0, refill=refill)
    ms_step = timed(step, a.calls)
    compute = eng.capture_train_step(None, warmup=0)
    ms_compute = timed(compute, a.calls)
    print(json.dumps({"dataset": a.dataset, **({"train_what": a.train_what, "crop": a.crop} if lc else {}), "B": a.B, "size": a.size, "frame": [a.W0, a.H0], "dtype": a.dtype, "KS": src.KS,
                      "store_GB": round(store.nbytes / 1e9, 3), "draw_ms": round(ms_draw, 4), "gather_ms": round(ms_gather, 4),
                      "resident_step_ms": round(ms_step, 3), "step_without_data_ms": round(ms_compute, 3),
                      "data_share_of_step": round((ms_draw + ms_gather) / ms_step, 4),
                      "resident_clips_per_s": round(a.B * 1e3 / ms_step, 1)}))


if __name__ == "__main__":
    main()
