"""What the two command-line entries (dpc_amd.main, dpc_amd.lc_main) share and neither owns: starting one process per GPU
(``launch``), bringing a rank up (``open_rank``), averaging the logged metrics (``average_over_ranks``) and ``StepDriver``, the
``--graph`` protocol of a run -- a short eager warm-up per kind of step, then one captured step per kind, replayed
(engine.BackboneEngine.capture_train_step / capture_eval_step).  Argument checks, engines, checkpoints, data
sources, schedules and log lines stay in the entries.
"""
from __future__ import annotations

import contextlib
import os

import torch


def world_size(args) -> int:
    """one rank per id of ``--gpu 0,1,..``"""
    return max(len([g for g in str(args.gpu).split(',') if g != '']), 1)


def launch(worker, args):
    """``worker(rank, world, args, port)`` in this process for one GPU, else in one spawned process per GPU"""
    world = world_size(args)
    if world == 1:
        worker(0, 1, args, 0)
    else:
        import torch.multiprocessing as mp
        mp.spawn(worker, args=(world, args, 29500 + os.getpid() % 2000), nprocs=world, join=True)


def open_rank(rank: int, world: int, args, port: int):
    """(device, simulator handle or None, torch.distributed or None) of this rank: its GPU made current and, for world > 1, the
    process group -- RCCL bound to the device, or gloo between the simulator's rank processes (CPU tier)"""
    gpus = [int(g) for g in str(args.gpu).split(',') if g != '']
    sim = getattr(args, '_simulator', None)   # tests only (CPU tier): the host-side SIMT simulator handle; the command line cannot set it
    if sim == 'emu':   # a spawned rank of the CPU tier loads its own handle (a ctypes library does not pickle)
        from . import _lib
        sim = _lib.load_emulator()
    dev = torch.device('cpu') if sim is not None else torch.device('cuda', gpus[rank] if world > 1 else gpus[0])
    if sim is None:
        torch.cuda.set_device(dev)
    if world <= 1:
        return dev, sim, None
    import torch.distributed as dist
    if sim is None:
        dist.init_process_group('nccl', init_method=f'tcp://127.0.0.1:{port}', rank=rank, world_size=world, device_id=dev)
    else:
        torch.set_num_threads(max(1, (os.cpu_count() or 2) // (2 * world)))
        dist.init_process_group('gloo', init_method=f'tcp://127.0.0.1:{port}', rank=rank, world_size=world)
    return dev, sim, dist


def average_over_ranks(dist, vals: torch.Tensor, world: int) -> torch.Tensor:
    """mean over ranks of a small device tensor, in place (the logged loss / top-k: equal shards, so the mean of per-rank means is the
    reference's mean over the gathered rows, dpc/main.py:211-218).  RCCL averages in the collective; gloo (CPU tier) has no AVG."""
    if dist is None or world <= 1:
        return vals
    if dist.get_backend() == 'nccl':
        dist.all_reduce(vals, op=dist.ReduceOp.AVG)
    else:
        dist.all_reduce(vals, op=dist.ReduceOp.SUM)
        vals.div_(world)
    return vals


def add_guard_flags(parser):
    """--clip_grad / --skip_nonfinite of both entries (BackboneEngine.set_grad_guard)"""
    parser.add_argument('--clip_grad', default=0.0, type=float, help='clip the global 2-norm of the gradient to this value inside the fused '
                        'step, on the device (torch.nn.utils.clip_grad_norm_\'s formula; works under --graph and --resident).  0 = off')
    parser.add_argument('--skip_nonfinite', action='store_true', help='drop an optimizer step whose gradient holds an Inf or NaN: parameters, '
                        'Adam moments and the step count keep their values, decided on the device.  With this or --clip_grad every printed '
                        'train line ends in the gradient norm and every training epoch in a "Grad guard:" line')


class GuardLog:
    """What the entries print about the gradient guard.  ``open`` turns the guard on from the flags (before any step is captured) and
    returns None without them -- the output then stays byte for byte what it was."""

    def __init__(self, eng):
        self.eng, self.seen = eng, (0, 0)

    @classmethod
    def open(cls, eng, args):
        if not args.clip_grad >= 0.0:
            raise ValueError('--clip_grad must not be negative')
        if not (args.clip_grad > 0.0 or args.skip_nonfinite):
            return None
        eng.set_grad_guard(args.clip_grad if args.clip_grad > 0.0 else None, args.skip_nonfinite)
        return cls(eng)

    def gnorm(self) -> str:
        """tail of a printed train line: the norm of the step just taken (one 32-byte copy; every rank holds the same value)"""
        return ' gnorm {:.4f}'.format(self.eng.grad_stats()['norm'])

    def epoch_line(self, steps: int) -> str:
        st = self.eng.grad_stats()
        now = (st['n_skipped'], st['n_clipped'])
        skipped, clipped = now[0] - self.seen[0], now[1] - self.seen[1]
        self.seen = now
        return 'Grad guard: {0} skipped, {1} clipped of {2} steps'.format(skipped, clipped, steps)


def add_ema_flags(parser):
    """--ema / --ema_eval / --use_ema of both entries (BackboneEngine.set_ema)"""
    parser.add_argument('--ema', default=0.0, type=float, metavar='DECAY', help='keep an exponential moving average of the parameters with '
                        'this decay inside the fused optimizer step (no extra launch; warm-up min(decay, (1 + t) / (10 + t)); works under '
                        '--graph and --resident); checkpoints gain an \'ema\' entry.  0 = off')
    parser.add_argument('--ema_eval', action='store_true', help='validate each epoch with the averaged weights (best-checkpoint selection '
                        'follows).  Needs --ema')
    parser.add_argument('--use_ema', action='store_true', help='read the checkpoints given to --pretrain / --test / --retrieval through their '
                        'averaged weights (the \'ema\' entry; an error when a file has none)')


def check_ema_flags(args):
    """what the entries refuse before they start a rank"""
    if not 0.0 <= args.ema < 1.0:
        raise ValueError('--ema must lie in (0, 1) (0 = off)')
    if args.ema_eval and not args.ema > 0.0:
        raise ValueError('--ema_eval needs --ema')


def open_ema(eng, args, rank: int = 0):
    """turns the average on from the flags (before any load re-seeds it and before any step is captured) and returns the context
    the entry validates in: ``eng.ema_weights`` with --ema_eval, else a no-op.  Without --ema nothing is printed"""
    check_ema_flags(args)
    if args.ema > 0.0:
        eng.set_ema(args.ema)
        if rank == 0:
            print('EMA: decay {}'.format(args.ema), flush=True)
    return eng.ema_weights if args.ema_eval else contextlib.nullcontext


def add_schedule_flags(parser):
    """--lr_schedule and its parameters, of both entries (BackboneEngine.set_lr_schedule)"""
    parser.add_argument('--lr_schedule', default='', choices=['', 'constant', 'cosine', 'linear', 'multistep'], help='scale the learning rate '
                        'of every parameter group by a per-step multiplier evaluated on the device inside the fused optimizer step (no extra '
                        'launch, no host work per step; works under --graph and --resident): after --warmup_steps of linear warm-up, constant, '
                        'cosine or linear decay to --lr_min_mult at --total_steps, or --lr_gamma at each of --lr_milestones.  Counted in '
                        'completed optimizer steps: a skipped step does not advance it, a resumed run continues it.  Default: off')
    parser.add_argument('--warmup_steps', default=0, type=int, help='optimizer steps of linear warm-up, multiplier (k + 1) / N at step k; alone it '
                        'means --lr_schedule constant')
    parser.add_argument('--total_steps', default=0, type=int, help='where cosine / linear decay ends (default: epochs x steps per epoch of this rank; with --frames that is known only once '
                        'a rank has opened its source, so pass the value to have it checked before the ranks start)')
    parser.add_argument('--lr_min_mult', default=0.0, type=float, help='the multiplier cosine / linear decay ends at and keeps, in [0, 1]')
    parser.add_argument('--lr_milestones', default='', type=str, help='multistep: comma-separated optimizer steps, strictly ascending, at most 8')
    parser.add_argument('--lr_gamma', default=0.1, type=float, help='multistep: the factor per milestone, in (0, 1]')


def schedule_from_flags(args, default_total: int = 0):
    """the LRSchedule the flags describe, or None without them; raises ValueError on what the launcher would refuse.  While
    --total_steps is left to its default and `default_total` is not known yet, the decay's end is not checked"""
    from .optim import LRSchedule
    kind = args.lr_schedule or ('constant' if args.warmup_steps else '')
    if not kind:
        stray = [f for f, given in (('--total_steps', args.total_steps != 0), ('--lr_min_mult', args.lr_min_mult != 0.0),
                                    ('--lr_milestones', args.lr_milestones != ''), ('--lr_gamma', args.lr_gamma != 0.1)) if given]
        if stray:
            raise ValueError('{} set the parameters of --lr_schedule, which is missing'.format(' / '.join(stray)))
        return None
    try:
        milestones = tuple(int(m) for m in args.lr_milestones.split(',') if m.strip() != '')
    except ValueError:
        raise ValueError('--lr_milestones must be comma-separated step counts, got {!r}'.format(args.lr_milestones))
    if args.total_steps < 0:
        raise ValueError('--total_steps must not be negative')
    total = args.total_steps or default_total
    if kind in ('cosine', 'linear') and not total:
        total = max(args.warmup_steps, 0) + 1   # (placeholder: the other fields are checked now, the end when it is known)
    return LRSchedule(kind, args.warmup_steps, total, args.lr_min_mult, milestones, args.lr_gamma)


def check_schedule_flags(args, steps_per_epoch: int = 0):
    """what the entries refuse before they start a rank.  steps_per_epoch: of synthetic input, where it is known here, so that the
    default --total_steps is checked against --warmup_steps as well; 0 leaves that to open_schedule"""
    schedule_from_flags(args, args.epochs * steps_per_epoch)


def open_schedule(eng, args, steps_per_epoch: int, rank: int = 0):
    """turns the schedule on from the flags (before any step is captured) and returns the tail of a printed train line, ' lr 1.000e-03'
    of the step just taken (one 16-byte copy; every rank holds the same value) -- or None without the flags: the output then stays
    byte for byte what it was"""
    schedule = schedule_from_flags(args, args.epochs * steps_per_epoch)
    if schedule is None:
        return None
    eng.set_lr_schedule(schedule)
    if rank == 0:
        print('LR schedule: {}'.format(schedule.describe()), flush=True)
    return lambda: ' lr {:.3e}'.format(eng.lr_now()['lr'])


def add_optimizer_flags(parser):
    """--optimizer / --wd_exclude_1d of both entries (BackboneEngine.set_optimizer)"""
    parser.add_argument('--optimizer', default='adam', choices=['adam', 'adamw', 'lamb'], help='update rule of the fused optimizer step: adam '
                        '(torch.optim.Adam, --wd folded into the gradient: the reference\'s), adamw (torch.optim.AdamW: --wd decoupled) or lamb '
                        '(layer-wise trust ratio |p| / |u| per parameter tensor, for large batches).  All three run inside the step, on the '
                        'device, under --graph, --resident, the gradient guard, --ema and --lr_schedule')
    parser.add_argument('--wd_exclude_1d', action='store_true', help='no weight decay on parameters with at most one dimension (biases, '
                        'BatchNorm); under lamb no trust ratio for them either.  Needs --optimizer adamw or lamb')


def check_optimizer_flags(args):
    """what the entries refuse before they start a rank"""
    if args.wd_exclude_1d and args.optimizer == 'adam':
        raise ValueError('--wd_exclude_1d needs --optimizer adamw or --optimizer lamb')


class LambLog:
    """What the entries print about the update rule.  ``open`` sets it from the flags (before any step is captured) and returns None
    unless the rule is lamb; without the flags nothing is printed -- the output then stays byte for byte what it was."""

    def __init__(self, eng):
        self.eng = eng

    @classmethod
    def open(cls, eng, args, rank: int = 0):
        check_optimizer_flags(args)
        if args.optimizer == 'adam':
            return None
        eng.set_optimizer(args.optimizer, args.wd_exclude_1d)
        if rank == 0:
            print('Optimizer: {}{}'.format(args.optimizer, ', wd_exclude_1d' if args.wd_exclude_1d else ''), flush=True)
        return cls(eng) if args.optimizer == 'lamb' else None

    def epoch_line(self) -> str:
        """one read-back per epoch: the trust ratios of the epoch's last step over the adaptive, trained parameters"""
        r = sorted(v[2] for v in self.eng.lamb_stats(adaptive_only=True).values())
        if not r:
            return 'LAMB: no adaptive parameter'
        mid = len(r) // 2
        median = r[mid] if len(r) % 2 else 0.5 * (r[mid - 1] + r[mid])
        return 'LAMB: trust ratio min {:.3g} median {:.3g} max {:.3g}'.format(r[0], median, r[-1])


def add_accum_flags(parser):
    """--accum_steps of both entries (BackboneEngine.set_grad_accum)"""
    parser.add_argument('--accum_steps', default=1, type=int, metavar='N', help='gradient accumulation inside the fused step: every batch is one '
                        'micro-batch, N of them make one optimizer step on their mean gradient, with one gradient exchange (works under '
                        '--graph and --resident).  An epoch runs (batches // N) * N batches; --total_steps, --warmup_steps, --lr_milestones, '
                        'the "Grad guard:" line and the checkpoint\'s step count are in optimizer steps.  BatchNorm statistics and the '
                        'contrastive negatives stay those of one micro-batch.  1 = off')


def check_accum_flags(args):
    """what the entries refuse before they start a rank"""
    if args.accum_steps < 1:
        raise ValueError('--accum_steps must be at least 1')


def open_accum(eng, args):
    """turns the accumulation on from the flag: before --resume (which continues the dropout stream at steps x N and compares the file's
    count with the run's) and before any step is captured"""
    check_accum_flags(args)
    if args.accum_steps > 1:
        eng.set_grad_accum(args.accum_steps)


def accum_epoch(args, batches: int):
    """(batches a training epoch runs, optimizer steps in it): whole cycles only, so that every epoch, validation and checkpoint
    falls on a cycle boundary; a partial cycle at the end is dropped"""
    steps = batches // args.accum_steps
    return steps * args.accum_steps, steps


def accum_line(args, batches: int, per_gpu: int, world: int):
    """what rank 0 prints once about the accumulation, or None without the flag: the output then stays byte for byte what it was"""
    n = args.accum_steps
    if n <= 1:
        return None
    line = 'Accumulation: {0} micro-batches of {1} per optimizer step (effective batch {2})'.format(n, per_gpu, n * per_gpu * world)
    dropped = batches - accum_epoch(args, batches)[0]
    return line + (', {} batches per epoch dropped'.format(dropped) if dropped else '')


class StepDriver:
    """The steps of a run, eager or replayed.  Without ``graph`` every step is eager.  With it, per RUN (not per epoch) the first two
    train steps and the first validation step are eager -- they size every lazy buffer --; from then on the engine is asked once
    per kind for a captured step on the stem's operand (``warmup=0``) and every later step replays that handle.

    ``refill_train`` / ``refill_val`` fill the operand on the device (fill_synthetic, load_resident): called in front of an eager
    step, handed to the capture -- which runs them inside the graph -- for a replayed one.  Nothing here touches the GPU until a step
    replays; the timing events are made on the epoch's first replayed train step."""

    def __init__(self, eng, graph: bool, allreduce=None, refill_train=None, refill_val=None):
        self.eng, self.graph, self.allreduce = eng, bool(graph), allreduce
        self.refill = {True: refill_train, False: refill_val}
        self.warm = {True: 2, False: 1}
        self.invalidate()
        self.replayed, self.events = 0, None

    def invalidate(self):
        """drop the handles: the next step of each kind asks the engine again -- which hands back the replay that exists when nothing
        it bakes in has changed, and captures a new step otherwise (a new learning rate).  The warm-up is not repeated."""
        self.captured = {True: None, False: None}

    def step(self, train: bool, eager, before_replay=None):
        """one train / validation step -> (its device result, whether it was a replay).  ``eager()`` is the entry's own step, run
        when this one is not replayed; ``before_replay()`` is host work a replay needs in front of it and an eager step does itself"""
        refill = self.refill[train]
        if not self.graph or self.warm[train]:
            if self.graph:
                self.warm[train] -= 1
            if refill is not None:
                refill()
            return eager(), False
        if before_replay is not None:
            before_replay()
        if self.captured[train] is None:
            self.captured[train] = (self.eng.capture_train_step(None, allreduce=self.allreduce, warmup=0, refill=refill) if train
                                    else self.eng.capture_eval_step(refill))
        if train and self.events is None:
            self.events = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.events[0].record()
        res = self.captured[train]()
        if train:
            self.events[1].record()
            self.replayed += 1
        return res, True

    def replay_line(self, batch_size: int):
        """ends a training epoch: its ``Graph replay:`` line -- device time from the first replayed train step of the epoch to the end
        of its last one -- or None when none was replayed"""
        n, events = self.replayed, self.events
        self.replayed, self.events = 0, None
        if not n:
            return None
        events[1].synchronize()
        ms = events[0].elapsed_time(events[1]) / n
        return 'Graph replay: {0} steps, {1:.3f} ms/step, {2:.1f} clips/s'.format(n, ms, batch_size * 1e3 / ms)
