"""``dpc_amd.optim.Adam``: the reference's ``optim.Adam(params, lr=args.lr, weight_decay=args.wd)`` (dpc/main.py:80-81, eval/test.py:88)
as ONE fused kernel over the engine's flat arenas instead of torch's per-tensor update over 76 parameters.

    model = dpc_amd.model.DPC_RNN(...).to('cuda')                      # or dpc_amd.lc.LC(...)
    optimizer = dpc_amd.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    ...
    optimizer.zero_grad(); loss.backward(); optimizer.step()          # dpc/main.py:229-231, eval/test.py:253-255, unchanged

The parameters of ``DPC_RNN`` / ``LC`` are views of the engine's parameter arena and, after ``loss.backward()``, their ``.grad`` are
views of its gradient arena (dpc_amd/model.py, dpc_amd/lc.py), so ``step()`` is one launch over the arenas with torch.optim.Adam's
arithmetic (L2 weight decay added to the gradient, bias-corrected moments; tests/test_engine_gpu.py holds it to the reference's own
Adam step).

Parameter groups: any partition of (a subset of) the module's parameters, each group with its own ``lr`` / ``weight_decay`` --
``--train_what ft`` of eval/test.py:76-84 builds one group per parameter.  ``step()`` reads the groups' current values every time
(``LambdaLR`` works) and maps them onto ``engine.set_param_groups``: the segment table of ``dpc_adam_groups_dev`` is re-uploaded
only when a value changed.  A parameter that is in no group, or whose ``.grad`` is ``None`` (``requires_grad = False``, or unused),
is frozen for that step -- neither read nor written, which is torch's skip.  With ONE group that holds every parameter, all with
gradients, the step is ``dpc_adam_dev`` exactly as before.  One step counter serves all parameters: one that joins later is updated
with the run's bias corrections, where torch would restart them (``BackboneEngine.set_param_groups``).

``load_state_dict()`` wants the file's groups to match this optimizer's in number and sizes, as torch's does (the one-group
optimizer used to read the file's first group whatever followed it).
``state_dict()`` / ``load_state_dict()`` speak torch.optim.Adam's layout (dpc_amd/checkpoint.py) -- with groups: one ``param_groups``
entry per group and state only for parameters that have been updated -- so checkpoints move both ways.
The engine is created by the module's first forward; a step before that has nothing to update and raises.

Gradient guard: ``Adam(..., max_grad_norm=1.0, skip_nonfinite=True)`` clips the global 2-norm of the gradients this step updates
and drops a step whose gradient holds an Inf or NaN, inside the fused step on the device (``BackboneEngine.set_grad_guard``; the
``.grad`` tensors are not rewritten).  ``clip_grad_norm_(parameters, max_norm)`` is ``torch.nn.utils.clip_grad_norm_`` over the
arena: three launches whatever the number of parameters, the norm returned as a device tensor.

Parameter average: ``Adam(..., ema_decay=0.999)`` keeps an exponential moving average of the parameters inside the same fused step
(``BackboneEngine.set_ema``); ``with ema_weights(optimizer):`` shows the averaged values through ``model.parameters()`` for
evaluation and puts the trained ones back on exit.

Learning-rate schedule: ``Adam(..., lr_schedule=LRSchedule("cosine", warmup_steps=500, total_steps=20000))`` scales every group's
``lr`` by a multiplier the device evaluates from its own step counter inside the fused step (``BackboneEngine.set_lr_schedule``):
no host write per step, and it works in a replayed hipGraph.  The groups' ``lr`` stay the base values.  ``lr_multiplier(k,
schedule)`` is the same function on the host, e.g. for ``LambdaLR(optimizer, lambda k: lr_multiplier(k, schedule))`` over a torch
optimizer; ``LambdaLR`` over this optimizer keeps working as before (use one or the other).
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple

import torch

import ctypes as C

from . import _lib as L
from . import checkpoint as ckpt
from .engine import engine_of


LR_KINDS = {"constant": L.LR_CONSTANT, "cosine": L.LR_COSINE, "linear": L.LR_LINEAR, "multistep": L.LR_MULTISTEP}


@dataclasses.dataclass(frozen=True)
class LRSchedule:
    """A learning-rate multiplier as a function of k, the number of completed optimizer steps (see lr_multiplier).  Step counts, not
    epochs; one multiplier for all parameter groups.  Checked where it is built, on the conditions the launcher refuses."""
    kind: str = "constant"
    warmup_steps: int = 0
    total_steps: int = 0              # cosine, linear: where the decay ends
    min_mult: float = 0.0             # cosine, linear: the multiplier from total_steps on
    milestones: Tuple[int, ...] = ()  # multistep: optimizer steps, strictly ascending, at most 8
    gamma: float = 0.1                # multistep

    def __post_init__(self):
        object.__setattr__(self, "milestones", tuple(int(m) for m in self.milestones))
        for f in ("warmup_steps", "total_steps"):
            object.__setattr__(self, f, int(getattr(self, f)))
        for f in ("min_mult", "gamma"):
            object.__setattr__(self, f, float(getattr(self, f)))
        if self.kind not in LR_KINDS:
            raise ValueError(f"LRSchedule: kind must be one of {sorted(LR_KINDS)}, got {self.kind!r}")
        if not 0 <= self.warmup_steps < 2 ** 31:
            raise ValueError(f"LRSchedule: warmup_steps must be a non-negative step count, got {self.warmup_steps}")
        if self.kind in ("cosine", "linear"):
            if not self.warmup_steps < self.total_steps < 2 ** 31:
                raise ValueError(f"LRSchedule: {self.kind} needs total_steps > warmup_steps, got {self.total_steps} and {self.warmup_steps}")
            if not 0.0 <= self.min_mult <= 1.0:
                raise ValueError(f"LRSchedule: min_mult must lie in [0, 1], got {self.min_mult}")
        if self.kind == "multistep":
            ms = self.milestones
            if len(ms) > L.LR_MAX_MILESTONES:
                raise ValueError(f"LRSchedule: at most {L.LR_MAX_MILESTONES} milestones, got {len(ms)}")
            if any(not 0 <= m < 2 ** 31 for m in ms) or any(b <= a for a, b in zip(ms, ms[1:])):
                raise ValueError(f"LRSchedule: milestones must be non-negative and strictly ascending, got {ms}")
            if not 0.0 < self.gamma <= 1.0:
                raise ValueError(f"LRSchedule: gamma must lie in (0, 1], got {self.gamma}")

    def descriptor(self) -> "L.LrSchedule":
        """struct dpc_lr_schedule, with the fields the kind does not read left at zero"""
        d = L.LrSchedule(kind=LR_KINDS[self.kind], warmup_steps=self.warmup_steps)
        if self.kind in ("cosine", "linear"):
            d.total_steps, d.min_mult = self.total_steps, self.min_mult
        if self.kind == "multistep":
            d.n_milestones, d.gamma = len(self.milestones), self.gamma
            for i, m in enumerate(self.milestones):
                d.milestones[i] = m
        return d

    def to_dict(self) -> dict:
        """the fields the kind reads (the checkpoint's 'lr_schedule' entry)"""
        out = {"kind": self.kind, "warmup_steps": self.warmup_steps}
        if self.kind in ("cosine", "linear"):
            out.update(total_steps=self.total_steps, min_mult=self.min_mult)
        if self.kind == "multistep":
            out.update(milestones=list(self.milestones), gamma=self.gamma)
        return out

    def describe(self) -> str:
        d = self.to_dict()
        return d.pop("kind") + "".join(f", {k} {v}" for k, v in d.items())


def lr_multiplier(k: int, schedule: LRSchedule) -> float:
    """The multiplier of the step taken after k completed optimizer steps -- what the device writes into its record, rounded to f32
    there.  Python floats (doubles), one rounding per operation, in the kernel's order (csrc/loss.hip: lr_mult)."""
    s, k = schedule, int(k)
    W = s.warmup_steps
    if k < W:
        return (k + 1) / W
    if s.kind in ("cosine", "linear"):
        m0 = s.min_mult
        x = (k - W) / (s.total_steps - W)
        if x >= 1.0:
            return m0
        shape = 0.5 * (1.0 + math.cos(3.141592653589793 * x)) if s.kind == "cosine" else 1.0 - x
        return m0 + (1.0 - m0) * shape
    mult = 1.0
    if s.kind == "multistep":
        for m in s.milestones:
            if m <= k:
                mult *= s.gamma
    return mult


class Adam(torch.optim.Optimizer):
    _kind, _exclude_1d = "adam", False   # the engine's update rule (BackboneEngine.set_optimizer); AdamW and LAMB below change it

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, amsgrad: bool = False,
                 max_grad_norm=None, skip_nonfinite: bool = False, ema_decay=None, lr_schedule: Optional[LRSchedule] = None):
        if amsgrad:
            raise ValueError("amsgrad is not supported (the reference does not use it, dpc/main.py:80-81)")
        if tuple(betas) != (0.9, 0.999) or eps != 1e-8:
            raise ValueError("dpc_amd.optim.Adam runs the reference's configuration: betas (0.9, 0.999), eps 1e-8")
        params = list(params)
        if params and isinstance(params[0], dict) and any(("betas" in g and tuple(g["betas"]) != (0.9, 0.999)) or g.get("eps", 1e-8) != 1e-8
                                                          or g.get("amsgrad") for g in params):
            raise ValueError("dpc_amd.optim.Adam runs the reference's configuration in every group: betas (0.9, 0.999), eps 1e-8, no amsgrad")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        for g in self.param_groups:
            if g.get("amsgrad") or tuple(g["betas"]) != (0.9, 0.999) or g["eps"] != 1e-8:
                raise ValueError("dpc_amd.optim.Adam runs the reference's configuration in every group: betas (0.9, 0.999), eps 1e-8, no amsgrad")
        if max_grad_norm is not None and not (0.0 < float(max_grad_norm) < float("inf")):
            raise ValueError(f"max_grad_norm must be None or a finite positive number, got {max_grad_norm}")
        self._guard = (max_grad_norm, bool(skip_nonfinite))   # (None, False): the engine's guard is left as it is
        if ema_decay is not None and not 0.0 < float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be None or lie in (0, 1), got {ema_decay}")
        self._ema = ema_decay   # None: the engine's average is left as it is
        if lr_schedule is not None and not isinstance(lr_schedule, LRSchedule):
            raise ValueError(f"lr_schedule must be None or an LRSchedule, got {lr_schedule!r}")
        self._lr_schedule = lr_schedule   # None: the engine's schedule is left as it is
        self._pending_state = None
        self._by_ptr = None     # (engine, {arena address: parameter name})
        self._updated = set()   # names of the parameters that have been updated at least once (torch creates their state then)

    def _engine(self):
        ps = [p for g in self.param_groups for p in g["params"]]
        eng = engine_of(ps[0]) if ps else None
        if eng is None:
            raise RuntimeError("dpc_amd.optim.Adam: the parameters are not backed by an engine yet -- run a forward of the "
                               "dpc_amd module (DPC_RNN / LC) they belong to first (it moves them into the engine's arena)")
        if self._by_ptr is None or self._by_ptr[0] is not eng:
            self._by_ptr = (eng, {t.data_ptr(): k for k, t in eng.PRM.items()})
        by_ptr = self._by_ptr[1]
        names = []
        for g in self.param_groups:
            ks = [by_ptr.get(p.data_ptr()) for p in g["params"]]
            if any(k is None for k in ks):
                raise RuntimeError("dpc_amd.optim.Adam updates parameters of ONE dpc_amd module (views of its engine's arena)")
            names.append(ks)
        return eng, names

    def _plain(self, eng, names) -> bool:
        """one group holding every parameter in registration order: the one-group update, exactly as without groups"""
        return len(names) == 1 and names[0] == list(eng.PRM.keys())

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        eng, names = self._engine()
        if self._pending_state is not None:
            self._load_into(eng, names, self._pending_state)
            self._pending_state = None
        live = []
        for g, ks in zip(self.param_groups, names):
            have = []
            for p, k in zip(g["params"], ks):
                if p.grad is None:   # torch skips it: frozen for this step
                    continue
                if p.grad.data_ptr() != eng.G[k].data_ptr():   # gradients that did not come from the engine's backward: bring them in
                    eng.G[k].copy_(p.grad)
                have.append(k)
            live.append(have)
        if self._plain(eng, names) and live == names:
            g = self.param_groups[0]
            eng.set_param_groups(None)
            eng.lr, eng.wd = float(g["lr"]), float(g["weight_decay"])
        else:
            if not any(live):
                return loss   # nothing has a gradient: torch's step would do nothing either
            eng.set_param_groups([{"params": have, "lr": float(g["lr"]), "weight_decay": float(g["weight_decay"])}
                                  for g, have in zip(self.param_groups, live)])
        if self._guard != (None, False):
            eng.set_grad_guard(*self._guard)
        if self._ema is not None and eng.ema_decay != float(self._ema):
            eng.set_ema(self._ema)
        if self._lr_schedule is not None and eng.lr_schedule != self._lr_schedule:
            eng.set_lr_schedule(self._lr_schedule)
        if (eng.optimizer_kind, eng.optimizer_exclude_1d) != (self._kind, self._exclude_1d):
            eng.set_optimizer(self._kind, self._exclude_1d)
        eng.adam_step()
        self._updated.update(k for have in live for k in have)
        eng.packed_for_step = -1
        return loss

    def _groups_for_state(self, names):
        return [{"params": ks, "lr": float(g["lr"]), "weight_decay": float(g["weight_decay"])} for g, ks in zip(self.param_groups, names)]

    def state_dict(self):
        try:
            eng, names = self._engine()
        except RuntimeError:
            return super().state_dict()   # nothing has run yet: torch's own (empty) state
        if self._plain(eng, names) and (not self._updated or len(self._updated) == len(names[0])):
            return ckpt.optimizer_state_dict(eng)
        return ckpt.grouped_optimizer_state_dict(eng, self._groups_for_state(names), self._updated)

    def _load_into(self, eng, names, state_dict):
        flat = [k for ks in names for k in ks]
        ckpt.load_optimizer_state(eng, state_dict, names=flat)
        ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        self._updated = {k for k, i in zip(flat, ids) if i in state_dict["state"]}

    def load_state_dict(self, state_dict):
        saved = state_dict["param_groups"]
        if len(saved) != len(self.param_groups) or any(len(a["params"]) != len(b["params"]) for a, b in zip(saved, self.param_groups)):
            raise ValueError("loaded state dict has a different number of parameter groups, or a group of another size "
                             "(torch.optim.Optimizer.load_state_dict raises the same way)")
        for g, sg in zip(self.param_groups, saved):
            g["lr"] = float(sg["lr"])
            g["weight_decay"] = float(sg.get("weight_decay", 0.0))
            if "initial_lr" in sg:
                g["initial_lr"] = sg["initial_lr"]
        try:
            eng, names = self._engine()
        except RuntimeError:
            self._pending_state = state_dict   # the engine does not exist yet: applied at the first step
            return
        self._load_into(eng, names, state_dict)


class AdamW(Adam):
    """``torch.optim.AdamW`` on the engine's fused step: the weight decay decoupled from the gradient (dpc_adamw_dev /
    dpc_adamw_groups_dev, one launch as Adam).  Same keyword arguments as Adam; weight_decay defaults to torch's 1e-2."""
    _kind = "adamw"

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kw)


class LAMB(Adam):
    """LAMB (You et al. 2020, bias-corrected) on the engine's fused step: per parameter tensor the step lr * u is scaled by the trust
    ratio |p| / |u| (dpc_lamb_moments / dpc_lamb_ratios / dpc_lamb_apply).  exclude_1d: parameters with at most one dimension (biases,
    BatchNorm) get no weight decay and no trust ratio.  Same keyword arguments as Adam otherwise."""
    _kind = "lamb"

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 exclude_1d: bool = False, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kw)
        self._exclude_1d = bool(exclude_1d)


def ema_weights(optimizer: Adam):
    """``with ema_weights(optimizer):`` -- inside, the parameters the optimizer updates (views of the engine's arena) hold their
    averaged values; on exit the trained values are back, bit for bit.  Evaluation only: a step inside the block raises."""
    eng, _ = optimizer._engine()
    return eng.ema_weights()


def _arena_names(params, who: str):
    """(engine, names) of parameters that are views of ONE engine's arena"""
    eng = engine_of(params[0]) if params else None
    if eng is None:
        raise RuntimeError(f"{who}: the parameters are not backed by an engine yet -- run a forward of the "
                           "dpc_amd module (DPC_RNN / LC) they belong to first (it moves them into the engine's arena)")
    by_ptr = {t.data_ptr(): k for k, t in eng.PRM.items()}
    names = [by_ptr.get(p.data_ptr()) for p in params]
    if any(k is None for k in names):
        raise RuntimeError(f"{who} works on parameters of ONE dpc_amd module (views of its engine's arena)")
    return eng, names


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm: float) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_(parameters, max_norm)`` (2-norm) over the engine's gradient arena: the total norm of the
    gradients of the given parameters that have one, then those gradients scaled in place by ``min(1, max_norm / (norm + 1e-6))``.
    Returns the norm as a 0-dim f32 device tensor (no read-back).  A non-finite norm is returned as such and nothing is scaled; it
    never skips anything.  dpc_grad_sumsq -> dpc_grad_verdict -> dpc_grad_scale over a segment table of the parameters' slices."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = list(parameters)
    max_norm = float(max_norm)
    eng, names = _arena_names(params, "dpc_amd.optim.clip_grad_norm_")
    have = []
    for p, k in zip(params, names):
        if p.grad is None:
            continue
        if p.grad.data_ptr() != eng.G[k].data_ptr():   # a gradient that did not come from the engine's backward: bring it in, as step() does
            eng.G[k].copy_(p.grad)
        have.append((p, k))
    if not have:
        return torch.zeros((), dtype=torch.float32, device=eng.device)
    live = {k for _, k in have}
    segs = []   # the parameters' 16-byte slots in arena order, neighbours merged (engine.set_param_groups builds its table the same way)
    for k, (o, n) in eng.offsets.items():
        if k not in live:
            continue
        e = o + (n + 3) // 4 * 4
        if segs and segs[-1][1] == o:
            segs[-1][1] = e
        else:
            segs.append([o, e])
    tab = (L.AdamSegment * len(segs))(*[L.AdamSegment(b, e, 0.0, 0.0, 1, 0) for b, e in segs])
    tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(eng.device)
    partials = torch.empty(L.GRAD_PARTIALS, dtype=torch.float64, device=eng.device)
    state = torch.zeros(C.sizeof(L.GradState), dtype=torch.uint8, device=eng.device)
    eng.call("dpc_grad_sumsq", eng.flat_g, eng.numel, tab_dev, len(segs), partials)
    eng.call("dpc_grad_verdict", partials, L.GRAD_PARTIALS, max_norm if max_norm > 0.0 else 0.0, 0, state)
    eng.call("dpc_grad_scale", eng.flat_g, eng.numel, tab_dev, len(segs), state)
    for p, k in have:   # a .grad that is a tensor of its own sees the scaled values too
        if p.grad.data_ptr() != eng.G[k].data_ptr():
            p.grad.copy_(eng.G[k])
    return state[8:12].view(torch.float32).reshape(()).clone()
