"""Training entry with the reference's command line (dpc/main.py:27-47), MI355X-native.

    python -m dpc_amd.main --net resnet18 --img_dim 128 --batch_size 128 --gpu 0,1,2,3 --synthetic 50

Same flags and defaults as the reference's ``main.py``.  What differs is the execution model:
``--gpu 0,1,..`` starts ONE PROCESS PER GPU (the reference wraps the model in nn.DataParallel,
dpc/main.py:65); each process owns a DPCEngine; ``--batch_size`` is the GLOBAL batch, as in the
reference (DataParallel scatters it along dim 0), so each GPU sees batch_size / n_gpu clips; gradients
are averaged with one RCCL all-reduce (dpc_amd/parallel.py).  Datasets / augmentation / tensorboard are outside this build's scope
(SURVEY.md §2 rows 8,9,11): the input is the synthetic N(0,1) video of ``--synthetic`` batches per
epoch with the dataset's tensor layout [B, num_seq, 3, seq_len, H, W] (dpc/dataset_3d.py:109-111), or -- ``--frames clips.npy`` --
decoded uint8 frames [clips, F, H0, W0, 3] on which the training transform of ``--dataset`` (dpc/main.py:114-132) runs on the GPU
(dpc_amd/data.py FrameSource -> engine.load_recipe -> train_step(None): SURVEY.md §8 f4).  ``--resident`` uploads that array (or,
with ``--offsets``, a packed store of videos of any length) to HBM once and draws the transform on the device
(data.ResidentFrameSource -> engine.load_resident): no host work per step; a different, equally distributed sample of clips.
``--graph`` runs every step after a short eager warm-up as a replay of one captured train step and one captured validation step
(entry.StepDriver over the engine's capture_train_step / capture_eval_step; the rank processes are entry.launch /
entry.open_rank, shared with dpc_amd.lc_main); the synthetic input is then drawn on the device inside the graph (engine.fill_synthetic) instead of by torch.randn.
Checkpoints are the reference's dictionary (``module.``-prefixed state_dict incl. alias keys, torch-Adam-layout
``optimizer``; dpc/main.py:166-174, utils/utils.py:14-26) written and read by ``dpc_amd/checkpoint.py``: a file
written here resumes in the reference and vice versa (tests/test_checkpoint.py).
"""
from __future__ import annotations

import argparse
import math
import os
import re
import time

import torch

from .entry import (GuardLog, LambLog, StepDriver, accum_epoch, accum_line, add_accum_flags, check_accum_flags, open_accum, add_optimizer_flags, check_optimizer_flags, average_over_ranks, add_ema_flags, add_guard_flags, add_schedule_flags, check_ema_flags,
                    check_schedule_flags, launch, open_ema, open_rank, open_schedule, world_size)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    parser.add_argument('--net', default='resnet18', type=str)
    parser.add_argument('--model', default='dpc-rnn', type=str)
    parser.add_argument('--dataset', default='ucf101', type=str)
    parser.add_argument('--seq_len', default=5, type=int, help='number of frames in each video block')
    parser.add_argument('--num_seq', default=8, type=int, help='number of video blocks')
    parser.add_argument('--pred_step', default=3, type=int)
    parser.add_argument('--ds', default=3, type=int, help='frame downsampling rate')
    parser.add_argument('--batch_size', default=4, type=int)
    parser.add_argument('--lr', default=1e-3, type=float, help='learning rate')
    parser.add_argument('--wd', default=1e-5, type=float, help='weight decay')
    parser.add_argument('--resume', default='', type=str, help='path of model to resume')
    parser.add_argument('--pretrain', default='', type=str, help='path of pretrained model')
    parser.add_argument('--epochs', default=10, type=int, help='number of total epochs to run')
    parser.add_argument('--start-epoch', default=0, type=int, help='manual epoch number (useful on restarts)')
    parser.add_argument('--gpu', default='0,1', type=str)
    parser.add_argument('--print_freq', default=5, type=int, help='frequency of printing output during training')
    parser.add_argument('--reset_lr', action='store_true', help='Reset learning rate when resume training?')
    parser.add_argument('--prefix', default='tmp', type=str, help='prefix of checkpoint filename')
    parser.add_argument('--train_what', default='all', type=str)
    parser.add_argument('--img_dim', default=128, type=int)
    # additions of this build
    parser.add_argument('--synthetic', default=20, type=int, help='synthetic batches per epoch (the data source unless --frames is given)')
    parser.add_argument('--dtype', default='bf16', choices=['bf16', 'f32'], help='compute dtype (f32 = parity mode)')
    parser.add_argument('--save_dir', default='', type=str, help='where to write checkpoints (default: none)')
    parser.add_argument('--frames', default='', type=str, help='uint8 .npy [clips, F, H0, W0, 3] of decoded frames: the training transform of '
                        '--dataset runs on the GPU (dpc_amd/data.py); replaces --synthetic')
    parser.add_argument('--val_frames', default='', type=str, help='frames for validate() (default: the --frames array; the reference validates '
                        'with the training transform too, dpc/main.py:135-136)')
    parser.add_argument('--crop', default=224, type=int, help='RandomCrop size of the ucf101 recipe (dpc/main.py:117)')
    parser.add_argument('--graph', action='store_true', help='train and validate on replayed hipGraph steps: the first two train steps and '
                        'the first validation step of the run are eager (warm-up), every later step replays one captured step, and rank 0 '
                        'prints the replayed steps\' ms/step after each training epoch.  Synthetic input is then drawn on the device inside '
                        'the graph (engine.fill_synthetic, seed 1000 + rank) instead of by torch.randn: the batches differ from a run '
                        'without --graph.  --frames input is unchanged: the same draws and bit-identical results.  HIP device only')
    parser.add_argument('--resident', action='store_true', help='hold the --frames array in HBM (uploaded once; every GPU holds a whole copy) '
                        'and draw the training transform on the device: per step nothing crosses the host, and --graph replays the draw '
                        'and the gather with the step.  The draws come from Philox (stream 4, seeded per rank), not from Python\'s random: '
                        'the clips are a different, equally distributed sample than a run without --resident sees.  Needs --frames')
    parser.add_argument('--offsets', default='', type=str, help='int64 .npy [videos + 1]: --frames is then a packed uint8 array '
                        '[total_frames, H0, W0, 3] of videos of any length, video v = frames[offsets[v]:offsets[v + 1]].  Needs --resident')
    parser.add_argument('--val_offsets', default='', type=str, help='--offsets of the --val_frames array')
    add_guard_flags(parser)
    add_ema_flags(parser)
    add_schedule_flags(parser)
    add_optimizer_flags(parser)
    add_accum_flags(parser)
    parser.add_argument('--neg_queue', default=0, type=int, metavar='K', help='negative queue: the keys (encoded future blocks) of the last K '
                        'training batches stay on the GPU and are extra negatives of every training row (engine.set_neg_queue): the loss '
                        'and the printed training accuracies are then over R + K R candidates.  A memory bank -- keys up to K updates old, '
                        'no momentum encoder; per GPU; not checkpointed; validation never uses it.  1 .. 64, bf16 only.  0: off')
    parser.add_argument('--neg_weight', default='1,1,1', type=str, metavar='S,T,E', help='weights of the three classes of negatives inside the '
                        'training loss\'s softmax (engine.set_neg_classes): spatial (same video, another position), temporal (same video and '
                        'position, another predicted step), easy (another video, and the --neg_queue keys).  0 takes a class out of the '
                        'loss.  The printed accuracies stay the unweighted ranks; validation is never weighted.  Each within [0, 65536]')
    parser.add_argument('--neg_report', action='store_true', help='end every printed training line with the mean shares of the softmax mass '
                        '(positive / spatial / temporal / easy) and the fraction of rows with a column of each class above the target')
    parser.add_argument('--loss_sym', default=0.0, type=float, metavar='W', help='symmetric InfoNCE (engine.set_loss_sym): over the same logits '
                        'each key also picks its prediction among the rows, and the training loss is (1 - W) x the prediction-to-key term + W x '
                        'the key-to-prediction term; 0.5 is the symmetric loss of CLIP / NT-Xent.  Every printed training line then ends in the '
                        'two terms and the column top-1; the printed accuracies stay the row ranks; validation is never symmetric.  Within '
                        '[0, 1]; not with --neg_weight / --neg_report.  0: off')
    parser.add_argument('--score_norm', default='dot', choices=['dot', 'cosine'], help='form of the contrastive score (engine.set_score_norm): '
                        'dot = pred . feature_inf, the reference\'s; cosine = the L2-normalised operands over --temperature, every logit in '
                        '[-1/T, 1/T] (training and validation alike).  Another model: loss and accuracies compare between runs of one T only')
    parser.add_argument('--temperature', default=1.0, type=float, metavar='T', help='temperature of --score_norm cosine (e.g. 0.07); must stay 1 '
                        'with the dot-product score')
    return parser


class AverageMeter:
    """utils/utils.py:77-113 (value, running average, 5-step local average)"""

    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0.0
        self.local = []

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count
        self.local = (self.local + [val])[-5:]

    @property
    def local_avg(self):
        return sum(self.local) / max(len(self.local), 1)


def _worker(rank: int, world: int, args, port: int):
    torch.manual_seed(0)  # dpc/main.py:50
    from .parallel import configure_rccl, default_reserve_cus
    if world > 1:
        configure_rccl(world)   # before this process's first HIP call: few long-lived RCCL channels beside the backward pass (parallel.py)
    dev, sim, dist = open_rank(rank, world, args, port)
    from .engine import DPCEngine
    from .model import DPC_RNN
    from .parallel import make_allreduce
    from . import checkpoint as ckpt

    if args.model != 'dpc-rnn':
        raise ValueError('wrong model!')  # dpc/main.py:63
    if args.train_what == 'last':
        # dpc/main.py:69-72 freezes `model.module.resnet`, an attribute DPC_RNN never had (the backbone is `.backbone`,
        # dpc/model_3d.py:29): the reference dies right there with this error, and so does the drop-in -- loudly, not by
        # silently training everything
        raise AttributeError("'DPC_RNN' object has no attribute 'resnet'")
    if args.batch_size % world:
        raise ValueError('batch_size must be divisible by the number of GPUs (drop_last semantics, dpc/main.py:313)')
    per_gpu = args.batch_size // world
    cdt = torch.bfloat16 if args.dtype == 'bf16' else torch.float32
    from .plan import LAYER_WIDTH
    widths = getattr(args, '_widths', None) or LAYER_WIDTH
    eng = DPCEngine(args.net, args.img_dim, args.num_seq, args.seq_len, args.pred_step, per_gpu, dev, cdt, widths, lib=sim, lr=args.lr, wd=args.wd,
                    seed=233 + rank, reserve_cus=default_reserve_cus(world))  # dropout stream: the reference seeds 233 (dpc/model_3d.py:18); independent per replica
    if args.graph:
        eng.check_graph_capture()   # before the first step: --graph never falls back to kernel-by-kernel launches
    init = DPC_RNN(args.img_dim, args.num_seq, args.seq_len, args.pred_step, args.net, widths=widths, seed=0)  # same on every rank
    eng.load_params({k: v.detach() for k, v in init.named_parameters()})
    best_acc, iteration = 0.0, 0
    resumed = None   # (the file's 'lr_schedule' entry, its path): compared once the run's own schedule is known (open_schedule below)
    ema_eval = open_ema(eng, args, rank)   # before the loads (each re-seeds the average; --resume then reads the file's) and before any capture
    lamb = LambLog.open(eng, args, rank)   # --optimizer: before --resume compares the file's rule with the run's, and before any capture
    open_accum(eng, args)                  # --accum_steps: before --resume continues the dropout stream, and before any capture
    if args.score_norm != 'dot':           # --score_norm: before --neg_queue (it empties the bank), --resume (it compares the file's) and any capture
        eng.set_score_norm(args.score_norm, args.temperature)
        if rank == 0:
            print('Score: {0}, temperature {1:g}'.format(args.score_norm, args.temperature), flush=True)
    if args.neg_queue:                     # --neg_queue: before --resume compares the file's K with the run's, and before any capture
        eng.set_neg_queue(args.neg_queue)
        if rank == 0:
            print('Negative queue: {0} batches ({1} keys of {2}, per GPU)'.format(args.neg_queue, args.neg_queue * eng.R, eng.D), flush=True)
    neg_w = parse_neg_weight(args.neg_weight)
    if neg_w != (1.0, 1.0, 1.0) or args.neg_report:   # --neg_weight / --neg_report: before --resume compares the file's weights, and before any capture
        eng.set_neg_classes(neg_w, report=args.neg_report)
        if rank == 0 and neg_w != (1.0, 1.0, 1.0):
            print('Negative classes: spatial {0:g} temporal {1:g} easy {2:g}'.format(*neg_w), flush=True)
    if args.loss_sym > 0:                  # --loss_sym: before --resume compares the file's weight with the run's, and before any capture
        eng.set_loss_sym(args.loss_sym)
        if rank == 0:
            print('Loss: symmetric, key-to-prediction weight {0:g}'.format(args.loss_sym), flush=True)
    if args.resume:  # dpc/main.py:88-102: strict model load + optimizer state (unless --reset_lr)
        if os.path.isfile(args.resume):
            m = re.search('_lr(.+?)_', args.resume)
            info = ckpt.resume(eng, args.resume, reset_lr=args.reset_lr, check_schedule=False)
            if 'lr_schedule' in info:
                resumed = ({'lr_schedule': info['lr_schedule']}, args.resume)
            args.start_epoch, iteration, best_acc = info['epoch'], info['iteration'], info['best_acc']
            if args.reset_lr:
                eng.lr, eng.wd = args.lr, args.wd
                if rank == 0 and m:
                    print('==== Change lr from %f to %f ====' % (float(m.group(1)), args.lr))
            if rank == 0:
                print("=> loaded resumed checkpoint '{}' (epoch {})".format(args.resume, info['epoch']))
        elif rank == 0:
            print("[Warning] no checkpoint found at '{}'".format(args.resume))
    if args.pretrain:  # dpc/main.py:104-112: key intersection (neq_load_customized)
        if os.path.isfile(args.pretrain):
            info = ckpt.pretrain(eng, args.pretrain, log=print if rank == 0 else (lambda *a: None), use_ema=args.use_ema)
            if rank == 0:
                print("=> loaded pretrained checkpoint '{}' (epoch {})".format(args.pretrain, info['epoch']))
        elif rank == 0:
            print("=> no checkpoint found at '{}'".format(args.pretrain))
    allreduce = make_allreduce(dist, world)
    gen = torch.Generator(dev).manual_seed(1000 + rank)
    shape = (per_gpu, args.num_seq, 3, args.seq_len, args.img_dim, args.img_dim)
    src_train = src_val = None
    if args.frames:   # decoded uint8 frames in, the reference's training transform on the GPU (dpc/dataset_3d.py:97-111, dpc/main.py:114-136)
        import random
        import numpy as np
        from .data import FrameSource
        random.seed(rank)
        np.random.seed(rank)      # dpc/main.py:51 seeds 0; one stream per rank like one per loader worker
        mk = lambda path: FrameSource(path, args.dataset, args.num_seq, args.seq_len, args.ds, args.img_dim, per_gpu, rank, world, args.crop)  # noqa: E731
        if args.resident:   # the store goes to HBM once; validation reads it (or its own) through a second source with its own draw stream
            from .data import FrameStore, ResidentFrameSource
            store = FrameStore(args.frames, args.offsets or None).to_device(dev, reserve=eng.resident_reserve())
            store_val = (FrameStore(args.val_frames, args.val_offsets or None).to_device(dev, reserve=eng.resident_reserve())
                         if args.val_frames else store)
            # Philox keys: the rank in the low word, the role (0 train, 1 validation) in the high one -- never seed + k (csrc/philox.h)
            mk = lambda st, role: ResidentFrameSource(st, args.dataset, args.num_seq, args.seq_len, args.ds, args.img_dim, per_gpu, dev, rank,  # noqa: E731
                                                      world, args.crop, seed=(role << 32) | rank)
            src_train, src_val = mk(store, 0), mk(store_val, 1)
            # the draw counters are not in the checkpoint (the engine keeps none of its counters there): a resumed run derives them
            # from the epochs already run, which is what they were
            src_train.set_draw(args.start_epoch * accum_epoch(args, len(src_train))[0])
            src_val.set_draw(args.start_epoch * len(src_val))
            if rank == 0 and (src_train.skipped or src_val.skipped):
                print('{0} training / {1} validation videos skipped (too short for one clip)'.format(src_train.skipped, src_val.skipped), flush=True)
        else:
            if args.offsets or args.val_offsets:
                raise ValueError('--offsets describes a packed frame store, which only --resident reads: --resident is missing')
            src_train = mk(args.frames)
            src_val = mk(args.val_frames) if args.val_frames else src_train

    # Where the operand of a step comes from.  Synthetic input under --graph: `refill` draws the batch on the device in front of the
    # step (inside the graph once the step is a replay); --frames: load_recipe fills the operand eagerly before each step and the graph starts
    # from it; --resident: `refill` advances the source's cursor, draws the recipe and gathers from the store, all on the device
    # (engine.load_resident) -- in front of every eager step, also without --graph, and inside the graph
    refill = refill_val = (lambda: eng.fill_synthetic(1000 + rank)) if args.graph and not args.frames else None
    if args.resident:
        refill, refill_val = (lambda: eng.load_resident(src_train)), (lambda: eng.load_resident(src_val))
    guard = GuardLog.open(eng, args)   # before the first capture: the guard's settings are baked into a captured step
    # a training epoch under --accum_steps N: whole cycles only; the schedule, the guard's line and LAMB's count its optimizer steps
    n_all = len(src_train) if src_train is not None else args.synthetic
    n_train, n_opt = accum_epoch(args, n_all)
    if rank == 0 and args.accum_steps > 1:
        print(accum_line(args, n_all, per_gpu, world), flush=True)
    lr_tail = open_schedule(eng, args, n_opt, rank)   # before the first capture, like the guard
    if resumed is not None:
        ckpt.check_lr_schedule(eng, *resumed)
    steps = StepDriver(eng, args.graph, allreduce, refill, refill_val)

    def validate(block):   # validate(): dropout off, BN still batch statistics (dpc/main.py:249-282, model_3d.py:28)
        eng.forward(block, train=False, materialise=False)  # loss / top-k only: the score is never written (bf16)
        return eng.loss_topk(with_grad=False)

    def run_epoch(train: bool, epoch: int):
        losses, accs = AverageMeter(), [AverageMeter() for _ in range(3)]
        nonlocal iteration
        src = src_train if train else src_val
        n_batches = n_train if train else (len(src) if src is not None else args.synthetic)
        feed = src.epoch(dev) if src is not None and not args.resident else None
        if args.resident:
            src.begin_epoch()   # the epoch's permutation to the device, the cursor to 0: the one host-to-device copy of the epoch
        for idx in range(n_batches):
            tic = time.time()
            block = None
            if feed is not None:
                frames, starts, clips = next(feed)
                eng.load_recipe(frames, starts, clips, ds=src.ds)   # fills the stem's operand; no f32 video in between
            elif not args.graph and not args.resident:
                block = torch.randn(shape, device=dev, generator=gen)
            res, _ = steps.step(train, (lambda: eng.train_step(block, allreduce=allreduce)) if train else (lambda: validate(block)))
            if idx % args.print_freq == 0 or not train:
                vals = average_over_ranks(dist, res.clone(), world)
                loss, t1, t3, t5 = vals.cpu().tolist()  # ONE packed D2H (the reference does five .item() syncs per step)
                losses.update(loss, per_gpu)
                for a, v in zip(accs, (t1, t3, t5)):
                    a.update(v, per_gpu)
                if train and rank == 0:
                    print('Epoch: [{0}][{1}/{2}]\t Loss {3:.6f} ({4:.4f})\t Acc: top1 {5:.4f}; top3 {6:.4f}; top5 {7:.4f} T:{8:.2f}\t'.format(
                        epoch, idx, n_batches, loss, losses.local_avg, t1, t3, t5, time.time() - tic) + (guard.gnorm() if guard else '') + (lr_tail() if lr_tail else '') +
                        (neg_report_tail(eng) if args.neg_report else '') + (loss_sym_tail(eng) if args.loss_sym > 0 else ''), flush=True)
                if train:
                    iteration += 1
        line = steps.replay_line(args.batch_size)
        if line and rank == 0:
            print(line, flush=True)
        if train and guard and rank == 0:
            print(guard.epoch_line(n_opt), flush=True)
        if train and lamb and rank == 0:
            print(lamb.epoch_line(), flush=True)
        return losses.local_avg, accs[0].local_avg, [a.local_avg for a in accs]

    for epoch in range(args.start_epoch, args.epochs):
        run_epoch(True, epoch)
        with ema_eval():   # --ema_eval: the averaged weights are swapped into flat_p for the validation epoch
            val_loss, val_acc, val_list = run_epoch(False, epoch)
        if rank == 0:
            print('[{0}/{1}] Loss {2:.4f}\t Acc: top1 {3:.4f}; top3 {4:.4f}; top5 {5:.4f} \t'.format(epoch, args.epochs, val_loss, *val_list), flush=True)
            if args.save_dir:
                os.makedirs(args.save_dir, exist_ok=True)
                is_best = val_acc > best_acc
                best_acc = max(val_acc, best_acc)
                fn = os.path.join(args.save_dir, 'epoch%s.pth.tar' % str(epoch + 1))
                # dpc/main.py:166-174 + utils/utils.py:14-26: same dictionary, same file rotation
                ckpt.save_checkpoint(ckpt.build_state(eng, epoch + 1, args.net, best_acc, iteration), is_best, filename=fn,
                                     keep_all=False)
    if rank == 0:
        print('Training from ep %d to ep %d finished' % (args.start_epoch, args.epochs))
    probe = getattr(args, '_probe', None)   # tests only: every rank leaves its parameter arena behind (identical on all ranks by construction)
    if probe:
        torch.save({'flat_p': eng.flat_p.detach().cpu(), 'flat_m': eng.flat_m.detach().cpu(), 'step': eng.step_count,
                    'rank': rank, 'world': world, 'per_gpu': per_gpu, 'seed': eng.seed,
                    **({'flat_ema': eng.flat_ema.detach().cpu()} if eng.ema_decay is not None else {})}, os.path.join(probe, f'rank{rank}.pt'))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def check_neg_queue_flags(args):
    """--neg_queue, refused before a rank starts"""
    if args.neg_queue < 0 or args.neg_queue > 64:
        raise ValueError('--neg_queue must be 0 (off) or 1 .. 64')
    if args.neg_queue and args.dtype == 'f32':
        raise ValueError('--neg_queue needs --dtype bf16 (f32 is the parity mode against a reference that has no bank)')


def parse_neg_weight(text: str):
    """'S,T,E' -> the three float32 weights; ValueError for anything the launcher would refuse"""
    from . import _lib as L
    parts = text.split(',')
    try:
        vals = [float(p) for p in parts]
    except ValueError:
        vals = []
    if len(parts) != 3 or len(vals) != 3:
        raise ValueError('--neg_weight takes three comma-separated numbers S,T,E (spatial, temporal, easy), got {0!r}'.format(text))
    try:
        return L.neg_class_weights(vals)
    except ValueError as e:
        raise ValueError('--neg_weight: {0}'.format(e)) from None


def check_neg_class_flags(args):
    """--neg_weight / --neg_report, refused before a rank starts"""
    w = parse_neg_weight(args.neg_weight)
    if args.neg_queue and w[2] == 0.0:
        raise ValueError('--neg_weight: the easy class cannot have the weight 0 with --neg_queue (the bank\'s keys are easy negatives)')


def neg_report_tail(eng) -> str:
    """--neg_report: the tail of a printed training line (one 32-byte read-back)"""
    s = eng.neg_class_stats()
    return ' neg P/S/T/E {0:.3f}/{1:.3f}/{2:.3f}/{3:.3f} above S/T/E {4:.3f}/{5:.3f}/{6:.3f}'.format(
        s['mass_pos'], s['mass_S'], s['mass_T'], s['mass_E'], s['above_S'], s['above_T'], s['above_E'])


def check_loss_sym_flags(args):
    """--loss_sym, refused before a rank starts"""
    if not (math.isfinite(args.loss_sym) and 0.0 <= args.loss_sym <= 1.0):
        raise ValueError('--loss_sym must be a weight within [0, 1]')
    if args.loss_sym > 0 and (parse_neg_weight(args.neg_weight) != (1.0, 1.0, 1.0) or args.neg_report):
        raise ValueError('--loss_sym: not with --neg_weight / --neg_report (the column direction of the class weights is not built)')


def loss_sym_tail(eng) -> str:
    """--loss_sym: the tail of a printed training line (one 32-byte read-back)"""
    s = eng.loss_sym_stats()
    return ' Lr {0:.4f} Lc {1:.4f} c@1 {2:.4f}'.format(s['loss_row'], s['loss_col'], s['col_top1'])


def check_score_flags(args):
    """--score_norm / --temperature, refused before a rank starts"""
    if not (math.isfinite(args.temperature) and args.temperature > 0):
        raise ValueError('--temperature must be finite and positive')
    if args.score_norm == 'dot' and args.temperature != 1.0:
        raise ValueError('--temperature other than 1 needs --score_norm cosine (the dot-product score is the reference\'s)')


def main(argv=None, _simulator=None, _widths=None, _probe=None):
    args = build_parser().parse_args(argv)
    args._simulator, args._widths, args._probe = _simulator, _widths, _probe   # tests/test_entries.py: the CPU tier runs the entry on the simulator
    check_ema_flags(args)
    check_accum_flags(args)
    check_neg_queue_flags(args)
    check_neg_class_flags(args)
    check_loss_sym_flags(args)
    check_score_flags(args)
    check_schedule_flags(args, 0 if args.frames else args.synthetic // args.accum_steps)
    check_optimizer_flags(args)
    if args.resident and not args.frames:
        raise SystemExit('--resident holds the --frames array in HBM: --frames is missing')
    if _simulator is not None and world_size(args) != 1:
        args._simulator = 'emu'   # the rank processes (gloo instead of RCCL) load the simulator themselves
    launch(_worker, args)


if __name__ == '__main__':
    main()
