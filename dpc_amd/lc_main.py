"""Entry of the downstream classifier with the reference's command line (eval/test.py:26-48), MI355X-native.

    python -m dpc_amd.lc_main --net resnet18 --img_dim 128 --batch_size 128 --gpu 0 --pretrain <dpc checkpoint> --synthetic 20

train() / validate() / test() follow eval/test.py:218-343 on the LCEngine (one process per GPU, RCCL gradient
all-reduce as in dpc_amd.main: entry.launch / entry.open_rank; ``--graph`` steps go through entry.StepDriver, which replays the
engine's capture_train_step / capture_eval_step).  Data: without ``--frames`` the input is synthetic N(0,1) video with random labels in the
dataset's tensor layout; with

    python -m dpc_amd.lc_main --frames videos.npy --labels labels.npy [--lengths lengths.npy] --pretrain <dpc checkpoint> --save_dir out
    python -m dpc_amd.lc_main --frames videos.npy --labels labels.npy [--lengths lengths.npy] --test out/epoch10.pth.tar --gpu 0

it is decoded uint8 frames [clips, F, H0, W0, 3] with integer labels [clips] (and the real frame count of each video, <= F):
fine-tuning and validation run the train / val transforms of eval/test.py:161-176 on the GPU (dpc_amd/data.py: draw_lc,
LabelledFrameSource -> engine.load_recipe -> train_step(None, labels)); ``--test`` runs the reference's video-level protocol
(eval/test.py:303-343 + eval/dataset_3d_lc.py:72-127): every frame at stride ``--ds`` cut into ``seq_len`` blocks, a
``num_seq``-block window slid with half overlap (3/4 for hmdb51), all windows through the model in eval mode from ONE uploaded
copy of the video (csrc/input_pipeline.hip: dpc_video_windows_to_input), softmax averaged over the windows for top-1 / top-5,
logits averaged for the loss and the confusion matrix -- reduced on the device (csrc/lc_test.hip), read back once after the last
video.  It prints the reference's result line, writes ``<ckpt>.confusion.npy`` (int64 [num_class, num_class], [pred][target])
where the reference draws ``<ckpt>.svg`` and appends the reference's paragraph to ``test_log.md`` beside the checkpoint.  Video
decoding, csv split files and tensorboard stay outside this build's scope: whatever produces these arrays plugs in.

    python -m dpc_amd.lc_main --frames videos.npy --labels labels.npy [--lengths lengths.npy | --offsets offsets.npy] --resident [--graph] ...

``--resident`` uploads the frames (and the labels) ONCE and keeps them in HBM: the train / val recipes are drawn on the device
(csrc/recipe_draw.hip: dpc_draw_recipe_ex), the clips gathered from the store and the labels by ``video_idx``
(data.ResidentLabelledSource -> engine.load_resident): no host work per step, and under ``--graph`` all of it inside the replayed
graph.  The draws are Philox words, not those of Python's ``random``: a ``--resident`` run sees a different, equally distributed
sample of clips than the run without it.  ``--test`` / ``--retrieval`` with it read every video as a slice of the store: the
same launches on the same bytes, no upload per video.
``--pretrain`` loads a DPC-RNN checkpoint
by key intersection (neq_load_customized, backbone/resnet_2d3d.py:310-333): backbone + ConvGRU weights are taken, the
running buffers and the head stay at their initial values -- exactly what the reference does with its own checkpoints.

Learning rate: the reference wraps Adam in ``LambdaLR(MultiStepLR_Restart_Multiplier)`` and calls ``scheduler.step(epoch)`` after
every epoch (eval/test.py:93-100,197,408-423): epoch e > start runs at ``lr * multiplier(e - 1)``, the first epoch of a run at
the constructor's ``lr * multiplier(0)`` (or the checkpoint's saved lr on ``--resume`` without ``--reset_lr``).  ``lr_multiplier``
below restates the multiplier; the fused Adam takes ``eng.lr`` per step.
``--train_what ft``: the reference gives parameters whose NAME contains 'resnet' or 'rnn' a 10x smaller lr
(eval/test.py:76-84) -- but LC's parameters are called ``backbone.*`` / ``agg.*`` / ``final_*`` (model_3d_lc.py:29-45), so the
filter never matches and every parameter trains at ``--lr``.  This entry does what the reference effectively does: one lr.
Two values of this build give what the flag was meant to do, both through the grouped fused Adam (engine.set_param_groups; the
epoch schedule scales every group, checkpoints written in these modes resume in them):
``--train_what ft_backbone``: ``backbone.*`` and ``agg.*`` train at ``--lr / 10``, ``final_bn`` / ``final_fc`` at ``--lr``;
``--train_what head``: only ``final_bn.*`` and ``final_fc.*`` train -- a linear probe on a frozen extractor.  The backward stops in
front of the ConvGRU; the extractor's BatchNorm layers keep using batch statistics and updating their running buffers in train()
(requires_grad = False in torch, and the only sensible mode after ``--pretrain``: a DPC checkpoint has no running statistics).

    python -m dpc_amd.lc_main --frames q.npy --labels ql.npy [--lengths ..] --retrieval out/epoch10.pth.tar --gpu 0
        [--gallery_frames g.npy --gallery_labels gl.npy [--gallery_lengths ..]] [--retrieval_k 1,5,10,20,50] [--retrieval_bn running|batch]

``--retrieval`` (an addition of this build) answers "how good is this checkpoint?" without a fine-tuning run: one L2-normalised
embedding per video (the mean over its test windows of the context vector ahead of ``final_bn``), cosine nearest neighbours in the
gallery -- or leave-one-out inside the query set -- recall@k and the 1-NN confusion matrix, all on the device (csrc/retrieval.hip),
one readback.  The checkpoint loads like ``--test`` (strict, else by key intersection, so a DPC checkpoint gives its backbone and
ConvGRU; pass ``--retrieval_bn batch`` for one: it has no running statistics).  Prints ``R@1: .. R@5: ..  (Nq queries, Ng gallery
videos, leave-one-out|cross, bn running|batch)``, appends it to ``retrieval_log.md`` beside the checkpoint and writes
``<ckpt>.retrieval.npz``.
"""
from __future__ import annotations

import argparse
import os
import time

import torch

from .entry import (GuardLog, LambLog, StepDriver, accum_epoch, accum_line, add_accum_flags, check_accum_flags, open_accum, add_optimizer_flags, check_optimizer_flags, average_over_ranks, add_ema_flags, add_guard_flags, add_schedule_flags, check_ema_flags,
                    check_schedule_flags, launch, open_ema, open_rank, open_schedule, world_size)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    parser.add_argument('--net', default='resnet18', type=str)
    parser.add_argument('--model', default='lc', type=str)
    parser.add_argument('--dataset', default='ucf101', type=str)
    parser.add_argument('--split', default=1, type=int)
    parser.add_argument('--seq_len', default=5, type=int)
    parser.add_argument('--num_seq', default=8, type=int)
    parser.add_argument('--num_class', default=101, type=int)
    parser.add_argument('--dropout', default=0.5, type=float)
    parser.add_argument('--ds', default=3, type=int)
    parser.add_argument('--batch_size', default=4, type=int)
    parser.add_argument('--lr', default=1e-3, type=float)
    parser.add_argument('--wd', default=1e-3, type=float, help='weight decay')
    parser.add_argument('--resume', default='', type=str)
    parser.add_argument('--pretrain', default='random', type=str)
    parser.add_argument('--test', default='', type=str)
    parser.add_argument('--epochs', default=10, type=int, help='number of total epochs to run')
    parser.add_argument('--start-epoch', default=0, type=int, help='manual epoch number (useful on restarts)')
    parser.add_argument('--gpu', default='0,1', type=str)
    parser.add_argument('--print_freq', default=5, type=int)
    parser.add_argument('--reset_lr', action='store_true', help='Reset learning rate when resume training?')
    parser.add_argument('--train_what', default='last', type=str, help='Train what parameters?  ft / last / all as the reference; '
                        'ft_backbone: backbone.* and agg.* at lr / 10; head: only final_bn.* and final_fc.* (frozen extractor)')
    parser.add_argument('--prefix', default='tmp', type=str)
    parser.add_argument('--img_dim', default=128, type=int)
    # additions of this build
    parser.add_argument('--synthetic', default=20, type=int, help='synthetic batches per epoch (the data source unless --frames is given)')
    parser.add_argument('--dtype', default='bf16', choices=['bf16', 'f32'])
    parser.add_argument('--save_dir', default='', type=str)
    parser.add_argument('--frames', default='', type=str, help='uint8 .npy [clips, F, H0, W0, 3] of decoded frames: the transforms of '
                        'eval/test.py:121-126,161-176 run on the GPU (dpc_amd/data.py); replaces --synthetic.  With --test: the video-level '
                        'test protocol over the videos in file order')
    parser.add_argument('--labels', default='', type=str, help='integer .npy [clips] of 0-based class ids (required with --frames)')
    parser.add_argument('--lengths', default='', type=str, help='integer .npy [clips]: the real frame count of each video, <= F (default: F)')
    parser.add_argument('--val_frames', default='', type=str, help='frames for validate() (default: the --frames array.  The reference '
                        'validates on a 30 %% pandas sample of its TEST split, eval/dataset_3d_lc.py:44-46,69: a property of its csv files, not '
                        'of this build -- pass that sample here)')
    parser.add_argument('--val_labels', default='', type=str, help='labels of --val_frames')
    parser.add_argument('--val_lengths', default='', type=str, help='lengths of --val_frames')
    parser.add_argument('--resident', action='store_true', help='hold the --frames array and its labels in HBM (uploaded once; every GPU holds '
                        'a whole copy) and draw the train / val recipes on the device: no host work per step, and under --graph the draw, '
                        'the gather and the labels are part of the replayed graph.  The draws come from Philox, not from Python\'s random: '
                        'the clips are a different, equally distributed sample than a run without --resident sees.  --test / --retrieval '
                        'read each video as a slice of the store (same results, no upload per video).  Needs --frames')
    parser.add_argument('--offsets', default='', type=str, help='int64 .npy [videos + 1]: --frames is then a packed uint8 array '
                        '[total_frames, H0, W0, 3] of videos of any length, video v = frames[offsets[v]:offsets[v + 1]] (instead of '
                        '--lengths).  Needs --resident')
    parser.add_argument('--val_offsets', default='', type=str, help='offsets of --val_frames')
    parser.add_argument('--crop', default=224, type=int, help='side of RandomSizedCrop / CenterCrop in the recipes (eval/test.py:122,162,170)')
    parser.add_argument('--graph', action='store_true', help='after two eager train steps and one eager validation step, replay ONE captured '
                        'hipGraph per kind of step (HIP device only; a changed learning rate captures a new step).  Synthetic input: batch '
                        'and labels are drawn on the device inside the graph (LCEngine.fill_synthetic) -- NOT the batches of a run without '
                        '--graph; with --frames the batches, parameters and log lines are those of the run without it.  With --test '
                        '--frames: the per-chunk forward of the video-level test is a replayed graph, same totals')
    parser.add_argument('--retrieval', default='', type=str, help='checkpoint (or "random"): nearest-neighbour video retrieval instead of '
                        'training -- one L2-normalised embedding per video of --frames (LCEngine.embed_video), cosine neighbours '
                        '(csrc/retrieval.hip), recall@k and the 1-NN confusion matrix; loaded like --test')
    parser.add_argument('--gallery_frames', default='', type=str, help='the gallery the queries of --frames are matched against '
                        '(default: leave-one-out inside the query set)')
    parser.add_argument('--gallery_labels', default='', type=str, help='labels of --gallery_frames')
    parser.add_argument('--gallery_lengths', default='', type=str, help='lengths of --gallery_frames')
    parser.add_argument('--retrieval_k', default='1,5,10,20,50', type=str, help='the k of recall@k, ascending, at most 64')
    parser.add_argument('--retrieval_bn', default='running', choices=['running', 'batch'], help='BatchNorm3d of the embedding forward: '
                        'running = eval mode, right for any checkpoint of this entry; batch = the statistics of each chunk of '
                        'windows, for a DPC checkpoint, which carries no running statistics (an embedding then depends on its chunk)')
    add_guard_flags(parser)
    add_ema_flags(parser)
    add_schedule_flags(parser)
    add_optimizer_flags(parser)
    add_accum_flags(parser)
    return parser


RETRIEVAL_MAX_K = 64   # dpc_knn_topk


def retrieval_ks(text: str):
    """--retrieval_k: ascending k values in [1, 64]"""
    try:
        ks = [int(k) for k in str(text).split(',') if k.strip() != '']
    except ValueError:
        raise ValueError('--retrieval_k wants integers separated by commas, got %r' % text) from None
    if not ks or ks[0] < 1 or any(a >= b for a, b in zip(ks, ks[1:])):
        raise ValueError('--retrieval_k wants ascending positive integers, got %r' % text)
    if ks[-1] > RETRIEVAL_MAX_K:
        raise ValueError('--retrieval_k: the neighbour search keeps at most %d neighbours, got %d' % (RETRIEVAL_MAX_K, ks[-1]))
    return ks


def retrieval(args, eng, mk, dev, log, num_epoch: int, probe=None):
    """--retrieval: every video long enough for a window is embedded (file order), each query's K = max(--retrieval_k) nearest gallery
    videos are looked up -- in --gallery_frames, or leave-one-out inside the query set -- and recall@k, the first hits and the 1-NN
    confusion matrix [label of the neighbour][label of the query] are counted on the device; ONE readback at the end."""
    import numpy as np
    from . import retrieval as R
    ks = retrieval_ks(args.retrieval_k)
    t0 = time.time()

    def embed(frames, labels, lengths, offsets=''):
        src = mk(frames, labels, lengths, 'test', offsets) if args.resident else mk(frames, labels, lengths, 'test')
        if len(src.keep) == 0:
            raise ValueError('no video of %s is long enough for %d x %d frames at stride %d' % (frames, args.num_seq, args.seq_len, args.ds))
        emb = torch.zeros(len(src.keep), eng.D, dtype=torch.float32, device=dev)
        labs = []
        for row, (_, fr, label, starts, clip) in enumerate(src.videos()):
            eng.embed_video(fr, starts, clip, emb[row], ds=args.ds, graph=args.graph, bn=args.retrieval_bn)
            labs.append(label)
        return emb, torch.tensor(labs, dtype=torch.int64).to(dev), src.skipped

    q_emb, q_lab, skipped = embed(args.frames, args.labels, args.lengths, args.offsets)
    cross = bool(args.gallery_frames)
    if cross:
        g_emb, g_lab, g_skipped = embed(args.gallery_frames, args.gallery_labels, args.gallery_lengths)
        skipped += g_skipped
        skip = None
    else:
        g_emb, g_lab = q_emb, q_lab
        skip = torch.arange(q_emb.shape[0], dtype=torch.int32).to(dev)
    top_idx, top_sim = R.knn_topk(eng.lib, q_emb, g_emb, ks[-1], skip=skip)
    hits, first_hit, confusion = R.recall_at_k(eng.lib, top_idx, q_lab, g_lab, ks, args.num_class)
    nq, ng = q_emb.shape[0], g_emb.shape[0]
    # the ONE readback of the run
    out = {k: v.cpu().numpy() for k, v in (('query_emb', q_emb), ('gallery_emb', g_emb), ('query_labels', q_lab), ('gallery_labels', g_lab),
                                           ('top_idx', top_idx), ('top_sim', top_sim), ('first_hit', first_hit), ('hits', hits),
                                           ('confusion', confusion))}
    out['ks'] = np.array(ks, np.int32)
    out['recall'] = out.pop('hits').astype(np.float64) / nq
    line = ' '.join('R@{}: {:.4f}'.format(k, r) for k, r in zip(ks, out['recall'])) + '  ({} queries, {} gallery videos, {}, bn {})'.format(
        nq, ng, 'cross' if cross else 'leave-one-out', args.retrieval_bn)
    log(line)
    log('(retrieval checkpoint epoch {})'.format(num_epoch))
    log('{} videos skipped (too short for {} x {} frames at stride {}), {:.1f} s'.format(skipped, args.num_seq, args.seq_len, args.ds,
                                                                                        time.time() - t0))
    if args.retrieval != 'random':
        np.savez(args.retrieval + '.retrieval.npz', **out)
        write_log(content=line, epoch=num_epoch, filename=os.path.join(os.path.dirname(args.retrieval), 'retrieval_log.md'))
    if probe:
        np.savez(os.path.join(probe, 'retrieval.npz'), **out)


def write_log(content: str, epoch: int, filename: str):
    """utils/utils.py:160-168"""
    with open(filename, 'a') as f:
        f.write('## Epoch %d:\n' % epoch)
        f.write('time: %s\n' % str(time.strftime('%Y_%m_%d_%H_%M_%S', time.localtime())))
        f.write(content + '\n\n')


def lr_multiplier(epoch: int, gamma: float, milestones, repeat: int) -> float:
    """MultiStepLR_Restart_Multiplier (eval/test.py:408-423): gamma^(milestones passed) inside a cycle of max(milestones) epochs,
    restarting `repeat` times, then pinned at the last decay level"""
    period = max(milestones)
    if epoch // period >= repeat:
        return gamma ** (len(milestones) - 1)
    return gamma ** sum(1 for m in milestones if epoch % period >= m)


def lr_milestones(dataset: str, img_dim: int):
    """eval/test.py:93-99"""
    if dataset == 'hmdb51':
        return [150, 250, 300]
    if dataset == 'ucf101':
        return [300, 400, 500] if img_dim == 224 else [60, 80, 100]
    raise ValueError('no learning-rate schedule for dataset %r (eval/test.py:93-99 defines ucf101 and hmdb51)' % dataset)


def _worker(rank: int, world: int, args, port: int):
    dev, sim, dist = open_rank(rank, world, args, port)
    from . import checkpoint as ckpt
    from .lc import LC, LCEngine
    from .parallel import make_allreduce

    if args.dataset == 'ucf101':
        args.num_class = 101   # eval/test.py:55-56
    elif args.dataset == 'hmdb51':
        args.num_class = 51
    if args.model != 'lc':
        raise ValueError('wrong model!')
    if args.batch_size % world:
        raise ValueError('batch_size must be divisible by the number of GPUs')
    per_gpu = args.batch_size // world
    cdt = torch.bfloat16 if args.dtype == 'bf16' else torch.float32
    from .plan import LAYER_WIDTH
    widths = getattr(args, '_widths', None) or LAYER_WIDTH
    eng = LCEngine(args.net, args.img_dim, args.num_seq, args.seq_len, per_gpu, dev, cdt, widths, lib=sim, lr=args.lr, wd=args.wd,
                   dropout=args.dropout, num_class=args.num_class, seed=666 + rank)  # model_3d_lc.py:16 seeds 666
    if args.graph:
        eng.check_graph_capture()   # before the first step: --graph never falls back to kernel-by-kernel launches
    init = LC(args.img_dim, args.num_seq, args.seq_len, args.net, args.dropout, args.num_class, widths=widths, seed=0)
    eng.load_params({k: v.detach() for k, v in init.state_dict().items()})
    log = print if rank == 0 else (lambda *a, **k: None)
    if args.train_what == 'ft':
        log("=> finetune backbone with smaller lr  [the reference's name filter ('resnet' / 'rnn') matches no LC parameter: one lr]")
    num_epoch, best_acc, iteration = 0, 0.0, 0
    base_lr = args.lr
    milestones = lr_milestones(args.dataset, args.img_dim)
    # --train_what ft_backbone / head (additions of this build): parameter groups of the fused Adam, [(names, lr before the schedule)]
    groups = None
    extractor = [k for k in eng.offsets if k.startswith(('backbone.', 'agg.'))]
    if args.train_what == 'ft_backbone':   # what eval/test.py:76-84 was written to do: the extractor at lr / 10
        groups = [(extractor, base_lr / 10), ([k for k in eng.offsets if k not in extractor], base_lr)]
        log('=> finetune backbone with smaller lr  [backbone.* and agg.* at lr / 10]')
    elif args.train_what == 'head':        # linear probe: only final_bn.* and final_fc.* train; the backward stops in front of the ConvGRU
        groups = [([k for k in eng.offsets if k.startswith(('final_bn.', 'final_fc.'))], base_lr)]
        log('=> train only final_bn / final_fc on a frozen backbone + ConvGRU (batch statistics, running buffers updated)')

    # --graph, synthetic input: `refill` draws batch and labels on the device in front of the step (inside the graph once it is a replay);
    # --frames: load_recipe and set_labels fill operand and labels eagerly before each step and the graph starts from them;
    # --resident: the two refills advance their source's cursor, draw the recipe, gather clips and labels on the device
    # (engine.load_resident) -- in front of every eager step, also without --graph, and inside the graph.  They are made ONCE: the
    # engine's capture cache keys on their identity, and set_lr asks for a new capture after every milestone.
    # lr / wd / the segment table are baked into a capture: set_lr drops the driver's handles, and the next step asks the engine again
    # -- the replay that exists when nothing changed, a new capture (the old one stays parked) when the schedule passed a milestone
    allreduce = make_allreduce(dist, world)
    refill = refill_val = (lambda: eng.fill_synthetic(1000 + rank)) if args.graph and not args.frames else None
    if args.resident:
        refill, refill_val = (lambda: eng.load_resident(src_train)), (lambda: eng.load_resident(src_val))
    # the gradient guard is on before the first capture and stays on: its settings are among the baked values, so the captures
    # set_lr asks for after a milestone carry it too
    guard = GuardLog.open(eng, args)
    # the parameter average likewise, and before the loads below: each load re-seeds it, --resume then reads the file's own
    ema_eval = open_ema(eng, args, rank)
    # the update rule likewise (--optimizer): its kind and tables are baked values too, and --resume compares the file's rule with it
    lamb = LambLog.open(eng, args, rank)
    # the accumulation likewise (--accum_steps): a baked value, and --resume continues the dropout stream at steps x N
    open_accum(eng, args)
    steps = StepDriver(eng, args.graph, allreduce, refill, refill_val)

    def set_lr(mult, saved=None):
        """the schedule scales every group; saved: the groups' lrs of a resumed checkpoint"""
        steps.invalidate()
        eng.lr = base_lr * mult
        if groups is not None:
            lrs = saved if saved is not None else [lr * mult for _, lr in groups]
            eng.set_param_groups([{'params': ks, 'lr': lr, 'weight_decay': args.wd} for (ks, _), lr in zip(groups, lrs)])
            eng.lr = lrs[-1]   # the log line's lr: the head group's
        if args.optimizer != 'adam':   # the rule's own tables follow the new values here, eagerly: the next capture finds them uploaded
            eng.set_optimizer(args.optimizer, args.wd_exclude_1d)

    set_lr(lr_multiplier(0, 0.1, milestones, 1))  # LambdaLR's constructor step
    resumed = None
    for path, what in ((args.test, 'test'), (args.retrieval, 'test'), (args.resume, 'resume'), (args.pretrain, 'pretrain')):   # --retrieval loads like --test
        if not path or path == 'random' or (what == 'pretrain' and args.resume):
            continue
        if not os.path.isfile(path):
            if what == 'test':
                raise ValueError()  # eval/test.py:121-122
            log("=> no checkpoint found at '{}'".format(path))
            continue
        ck = torch.load(path, map_location='cpu', weights_only=False)
        if args.use_ema and what != 'resume':   # --use_ema: the parameters of the file's averaged model, the buffers of its own
            ck['state_dict'] = ckpt.averaged_state_dict(eng, ck, path)
        # --resume: nn.Module.load_state_dict, strict in both directions (eval/test.py:145); --test: strict, falling back to the
        # key intersection with a warning (:113-116); --pretrain: key intersection (neq_load_customized, :160)
        try:
            missing, unexpected = ckpt.load_model_state(eng, ck['state_dict'], strict=what != 'pretrain')
        except RuntimeError:
            if what != 'test':
                raise
            log('=> [Warning]: weight structure is not equal to test model; Use non-equal load ==')
            missing, unexpected = ckpt.load_model_state(eng, ck['state_dict'], strict=False)
        log("=> loaded {} checkpoint '{}' (epoch {}; {} keys not in the file, {} keys of the file unused)".format(
            what, path, ck.get('epoch', 0), len(missing), len(unexpected)))
        num_epoch = ck.get('epoch', 0)
        if what == 'resume':
            args.start_epoch = ck['epoch']
            best_acc = float(ck.get('best_acc', 0.0))
            iteration = int(ck.get('iteration', 0))
            ckpt.load_ema_state(eng, ck, path)
            ckpt.check_optimizer_kind(eng, ck, path)
            ckpt.check_accum_steps(eng, ck, path)
            if 'lr_schedule' in ck:   # compared once the run's own schedule is known (open_schedule below)
                resumed = ({'lr_schedule': ck['lr_schedule']}, path)
            if not args.reset_lr and 'optimizer' in ck:
                if groups is None:
                    ckpt.load_optimizer_state(eng, ck['optimizer'])  # restores the group's lr as optimizer.load_state_dict does
                else:
                    saved = ck['optimizer']['param_groups']
                    if [len(g['params']) for g in saved] != [len(ks) for ks, _ in groups]:
                        raise ValueError("the checkpoint's optimizer groups are not those of --train_what %s" % args.train_what)
                    ckpt.load_optimizer_state(eng, ck['optimizer'], names=[k for ks, _ in groups for k in ks])
                    set_lr(1.0, saved=[float(g['lr']) for g in saved])
    probe = getattr(args, '_probe', None)   # tests only: the rank leaves its arenas (and in test mode the totals) behind
    src_train = src_val = None
    if args.frames:   # labelled uint8 frames in (eval/dataset_3d_lc.py + the transforms of eval/test.py:121-126,161-176 on the GPU)
        import random
        import numpy as np
        from .data import LabelledFrameSource
        if not args.labels:
            raise ValueError('--frames needs --labels')
        if bool(args.val_frames) != bool(args.val_labels):
            raise ValueError('--val_frames and --val_labels come together')
        torch.manual_seed(0)      # the epoch permutation (RandomSampler): the same on every rank, each takes its shard
        random.seed(rank)
        np.random.seed(rank)      # as dpc_amd.main: one stream per rank like one per loader worker (eval/test.py seeds nothing)
        mk = lambda fr, lb, ln, recipe: LabelledFrameSource(fr, lb, args.dataset, args.num_seq, args.seq_len, args.ds, args.img_dim, per_gpu,  # noqa: E731
                                                            args.num_class, recipe, ln or None, rank, world, args.crop)
        if args.resident:   # every store goes to HBM once; a source is a view of one with its own recipe and draw stream
            from .data import FrameStore, ResidentLabelledSource
            stores = {}

            def mk(fr, lb, ln, recipe, offsets='', role=0):
                key = (fr, ln or '', offsets)
                if key not in stores:
                    stores[key] = FrameStore(fr, offsets or None, ln or None).to_device(dev, reserve=eng.resident_reserve())
                # Philox keys: the rank in the low word, the role (0 train, 1 validation) in the high one -- never seed + k (csrc/philox.h)
                return ResidentLabelledSource(stores[key], lb, args.dataset, args.num_seq, args.seq_len, args.ds, args.img_dim, per_gpu,
                                              args.num_class, dev, recipe, rank, world, args.crop, seed=(role << 32) | rank)
        if args.retrieval:
            retrieval(args, eng, mk, dev, log, num_epoch, probe)
            return
        if args.test:
            src_test = mk(args.frames, args.labels, args.lengths, 'test', args.offsets) if args.resident else mk(args.frames, args.labels, args.lengths, 'test')
            t0 = time.time()
            eng.test_reset()
            for _, frames, label, starts, clip in src_test.videos():
                eng.test_video(frames, label, starts, clip, ds=args.ds, graph=args.graph)
            loss_sum, top1, top5, n_vid = eng.test_totals.cpu().tolist()   # the ONE readback of the run (+ the confusion matrix below)
            confusion = eng.test_confusion.cpu()
            n = max(n_vid, 1.0)
            line = 'Loss {:.4f}\t Acc top1: {:.4f} Acc top5: {:.4f} \t'.format(loss_sum / n, top1 / n, top5 / n)
            log(line)
            log('(test checkpoint epoch {})'.format(num_epoch))
            log('{} videos tested, {} skipped (too short for {} x {} frames at stride {}), {:.1f} s'.format(
                int(n_vid), src_test.skipped, args.num_seq, args.seq_len, args.ds, time.time() - t0))
            if args.test != 'random':   # where the reference writes <ckpt>.svg and test_log.md (eval/test.py:338-341)
                np.save(args.test + '.confusion.npy', confusion.numpy())
                write_log(content=line, epoch=num_epoch, filename=os.path.join(os.path.dirname(args.test), 'test_log.md'))
            if probe:
                torch.save({'totals': [loss_sum, top1, top5, n_vid], 'confusion': confusion, 'skipped': src_test.skipped,
                            'flat_p': eng.flat_p.detach().cpu(), 'flat_m': eng.flat_m.detach().cpu(), 'step': eng.step_count},
                           os.path.join(probe, f'rank{rank}.pt'))
            return
        if args.resident:
            src_train = mk(args.frames, args.labels, args.lengths, 'train', args.offsets, 0)
            src_val = (mk(args.val_frames, args.val_labels, args.val_lengths, 'val', args.val_offsets, 1) if args.val_frames
                       else mk(args.frames, args.labels, args.lengths, 'val', args.offsets, 1))
            # the draw counters are not in the checkpoint: a resumed run derives them from the epochs already run, which is what they were
            src_train.set_draw(args.start_epoch * accum_epoch(args, len(src_train))[0])
            src_val.set_draw(args.start_epoch * len(src_val))
            if src_train.skipped or src_val.skipped:
                log('{0} training / {1} validation videos skipped (too short for one clip)'.format(src_train.skipped, src_val.skipped), flush=True)
        else:
            src_train = mk(args.frames, args.labels, args.lengths, 'train')
            src_val = mk(args.val_frames, args.val_labels, args.val_lengths, 'val') if args.val_frames else mk(args.frames, args.labels, args.lengths, 'val')
    gen = torch.Generator(dev).manual_seed(1000 + rank)
    shape = (per_gpu, args.num_seq, 3, args.seq_len, args.img_dim, args.img_dim)

    def batch():
        return (torch.randn(shape, device=dev, generator=gen),
                torch.randint(0, args.num_class, (per_gpu,), device=dev, generator=gen))

    def reduce(res):
        return average_over_ranks(dist, res.clone(), world).cpu().tolist()  # one packed D2H per logged step

    if args.test:  # eval/test.py:306-343: eval mode; softmax averaged over the clip's sequences, top-1 / top-5
        top1 = top5 = loss_sum = 0.0
        for _ in range(args.synthetic):
            x, y = batch()
            out, _ = eng.forward(x, y, train=False)
            prob = torch.softmax(out, 2).mean((0, 1), keepdim=False).view(1, -1)
            tgt = y[:1]
            top = prob.topk(5, 1).indices
            top1 += float((top[:, :1] == tgt[:, None]).any())
            top5 += float((top == tgt[:, None]).any())
            loss_sum += torch.nn.functional.cross_entropy(out.mean((0, 1)).view(1, -1), tgt).item()
        n = max(args.synthetic, 1)
        log('Loss {:.4f}\t Acc top1: {:.4f} Acc top5: {:.4f} \t'.format(loss_sum / n, top1 / n, top5 / n))
        log('(test checkpoint epoch {})'.format(num_epoch))
    else:
        def step(train: bool, feed):
            """one train / validation step, eager or replayed; returns its device f32[2]"""
            x = y = None
            if feed is not None:
                frames, starts, clips, y = next(feed)
                eng.load_recipe(frames, starts, clips, ds=args.ds)   # fills the stem's operand; no f32 video in between
            elif not args.graph and not args.resident:   # --resident: the refill has filled operand and labels
                x, y = batch()

            def eager():
                if train:
                    return eng.train_step(x, y, allreduce=allreduce)
                eng.forward(x, y, train=False)
                return eng.result

            # a replay reads the labels as they stand: the feed's are set in front of it (synthetic ones are drawn inside the graph)
            return steps.step(train, eager, (lambda: eng.set_labels(y)) if y is not None else None)[0]

        # The per-step schedule multiplies whatever the epoch schedule (set_lr) has put into eng.lr / the segment table: on before the
        # first capture, and among the baked values, so the captures set_lr asks for after a milestone carry it too
        # a training epoch under --accum_steps N: whole cycles only; the schedule, the guard's line and LAMB's count its optimizer steps
        n_all = len(src_train) if src_train is not None else args.synthetic
        n_train, n_opt = accum_epoch(args, n_all)
        if args.accum_steps > 1:
            log(accum_line(args, n_all, per_gpu, world), flush=True)
        lr_tail = open_schedule(eng, args, n_opt, rank)
        if resumed is not None:
            ckpt.check_lr_schedule(eng, *resumed)
        for epoch in range(args.start_epoch, args.epochs):
            feed = src_train.epoch(dev) if src_train is not None and not args.resident else None
            if args.resident:
                src_train.begin_epoch()   # the epoch's permutation to the device, the cursor to 0: the one host-to-device copy of the epoch
            for idx in range(n_train):  # train(): eval/test.py:218-271
                res = step(True, feed)
                if idx % args.print_freq == 0:
                    loss, acc = reduce(res)
                    log('Epoch: [{0}][{1}/{2}]\t Loss {3:.4f}\t Acc: {4:.4f}\t lr {5:g}'.format(epoch, idx, n_train, loss, acc, eng.lr) +
                        (guard.gnorm() if guard and rank == 0 else '') + (lr_tail() if lr_tail and rank == 0 else ''), flush=True)
                    iteration += 1  # advanced on logged steps only, as the reference does (eval/test.py:262-270)
            line = steps.replay_line(args.batch_size)
            if line:
                log(line, flush=True)
            if guard and rank == 0:
                log(guard.epoch_line(n_opt), flush=True)
            if lamb and rank == 0:
                log(lamb.epoch_line(), flush=True)
            vl = va = 0.0
            n_val = len(src_val) if src_val is not None else max(args.synthetic // 4, 1)
            feed = src_val.epoch(dev) if src_val is not None and not args.resident else None
            if args.resident:
                src_val.begin_epoch()
            with ema_eval():   # --ema_eval: the averaged weights are swapped into flat_p for the validation epoch
                for idx in range(n_val):  # validate(): eval/test.py:273-304 (eval mode, running statistics)
                    loss, acc = reduce(step(False, feed))
                    vl += loss
                    va += acc
            nv = max(n_val, 1)
            val_acc = va / nv
            log('Loss {:.4f}\t Acc: {:.4f} \t'.format(vl / nv, val_acc), flush=True)
            set_lr(lr_multiplier(epoch, 0.1, milestones, 1))  # scheduler.step(epoch), eval/test.py:197
            is_best = val_acc > best_acc  # eval/test.py:205-214
            best_acc = max(val_acc, best_acc)
            if rank == 0 and args.save_dir:
                os.makedirs(args.save_dir, exist_ok=True)
                state = {'epoch': epoch + 1, 'net': args.net, 'state_dict': {'module.' + k: v.cpu() for k, v in eng.state_dict().items()},
                         'best_acc': best_acc, 'iteration': iteration,
                         'optimizer': (ckpt.optimizer_state_dict(eng) if groups is None else
                                       ckpt.grouped_optimizer_state_dict(eng, [g for g in eng.param_groups if not g['frozen']]))}
                if eng.lr_schedule is not None:
                    state['lr_schedule'] = ckpt.lr_schedule_entry(eng)
                if eng.ema_decay is not None:
                    state['ema'] = ckpt.ema_entry(eng, state['state_dict'])
                if eng.optimizer_kind != 'adam':
                    state['optimizer_kind'] = eng.optimizer_kind
                if eng.accum_steps > 1:
                    state['accum_steps'] = eng.accum_steps
                ckpt.save_checkpoint(state, is_best, filename=os.path.join(args.save_dir, 'epoch%s.pth.tar' % str(epoch + 1)))
        log('Training from ep %d to ep %d finished' % (args.start_epoch, args.epochs))
        if probe:
            torch.save({'flat_p': eng.flat_p.detach().cpu(), 'flat_m': eng.flat_m.detach().cpu(), 'step': eng.step_count, 'rank': rank,
                        'world': world, 'per_gpu': per_gpu, **({'flat_ema': eng.flat_ema.detach().cpu()} if eng.ema_decay is not None else {})},
                       os.path.join(probe, f'rank{rank}.pt'))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def main(argv=None, _simulator=None, _widths=None, _probe=None):
    args = build_parser().parse_args(argv)
    args._simulator, args._widths, args._probe = _simulator, _widths, _probe   # tests/test_entries.py: the CPU tier runs the entry on the simulator
    check_ema_flags(args)
    check_accum_flags(args)
    check_schedule_flags(args, 0 if args.frames else args.synthetic // args.accum_steps)
    check_optimizer_flags(args)
    world = world_size(args)
    if args.resident and not args.frames:
        raise ValueError('--resident holds the --frames array in HBM: --frames is missing')
    if (args.offsets or args.val_offsets) and not args.resident:
        raise ValueError('--offsets describes a packed frame store, which only --resident reads: --resident is missing')
    if (args.lengths and args.offsets) or (args.val_lengths and args.val_offsets):
        raise ValueError('--lengths goes with the dense --frames array and --offsets with a packed one: pass --lengths or --offsets, not both')
    if args.val_offsets and not args.val_frames:
        raise ValueError('--val_offsets describes the packed store of --val_frames: --val_frames is missing')
    if args.test and args.frames and world != 1:   # the reference's DataParallel over the windows of a video is not reproduced
        raise ValueError('--test with --frames runs on one GPU (the windows of a video are chunked on it): pass --gpu 0')
    if args.retrieval:
        if args.test:
            raise ValueError('--retrieval and --test are two runs: pass one of them')
        if not args.frames:
            raise ValueError('--retrieval needs --frames and --labels')
        if bool(args.gallery_frames) != bool(args.gallery_labels):
            raise ValueError('--gallery_frames and --gallery_labels come together')
        if world != 1:   # the rule of --test --frames
            raise ValueError('--retrieval runs on one GPU (the windows of a video are chunked on it): pass --gpu 0')
        retrieval_ks(args.retrieval_k)
        if args.graph and args.retrieval_bn == 'batch':
            raise ValueError('--graph replays the eval-mode step: it cannot be combined with --retrieval_bn batch')
    if _simulator is not None and world != 1:
        args._simulator = 'emu'   # the rank processes (gloo instead of RCCL) load the simulator themselves
    launch(_worker, args)


if __name__ == '__main__':
    main()
