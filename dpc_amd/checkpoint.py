"""Checkpoint compatibility with the reference.

The reference saves, once per epoch (dpc/main.py:166-174 through utils/utils.py:14-26),

    {'epoch', 'net', 'state_dict': DataParallel(model).state_dict()   # 'module.'-prefixed, alias keys included
     'best_acc', 'optimizer': torch.optim.Adam(...).state_dict(), 'iteration'}

and reads it back strictly on ``--resume`` (model AND optimizer, dpc/main.py:88-102) or by key
intersection on ``--pretrain`` (backbone/resnet_2d3d.py:310-333).  This module produces and consumes
exactly that dictionary from the engine's flat f32 arenas, so a file written here resumes in the
reference and a file written by the reference resumes here -- Adam moments and step count included.

The Adam state is laid out as ``torch.optim.Adam.state_dict()`` lays it out: ``state[i]`` for the i-th
entry of ``model.parameters()`` (the reference's registration order == the arena order, alias
parameters deduplicated) holds ``step`` (0-dim f32 tensor), ``exp_avg`` and ``exp_avg_sq`` with the
parameter's shape; ``param_groups`` is one group whose hyper-parameter keys are taken from the
installed torch (so ``optimizer.load_state_dict`` of that torch accepts it).
"""
from __future__ import annotations

import glob
import os
import warnings
from typing import Dict, Iterable, List, Tuple

import torch

ALIAS_FROM, ALIAS_TO = "agg.ConvGRUCell_00.", "agg.cell_list.0."  # backbone/convrnn.py:55-58


def _strip(k: str) -> str:
    return k[7:] if k.startswith("module.") else k


def model_state_dict(eng, prefix: str = "module.") -> "Dict[str, torch.Tensor]":
    """reference-layout state_dict of the engine's parameters (CPU copies; alias keys share storage)"""
    out: Dict[str, torch.Tensor] = {}
    for k, v in eng.PRM.items():
        out[prefix + k] = v.detach().cpu().clone()
    # the reference lists the alias keys right after the cell's own keys (ModuleList registered second)
    ordered: Dict[str, torch.Tensor] = {}
    cell = [k for k in out if k.startswith(prefix + ALIAS_FROM)]
    for k, v in out.items():
        ordered[k] = v
        if cell and k == cell[-1]:
            for c in cell:
                ordered[c.replace(ALIAS_FROM, ALIAS_TO)] = out[c]
    return ordered


def _adam_group_defaults(lr: float, wd: float, kind: str = "adam") -> dict:
    """hyper-parameter keys/values torch.optim.Adam(params, lr=lr, weight_decay=wd) of the installed torch writes -- under the
    engine's "adamw" update rule torch.optim.AdamW's, so that the file continues there (LAMB, which torch does not have, keeps Adam's)"""
    cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
    probe = cls([torch.nn.Parameter(torch.zeros(1))], lr=lr, weight_decay=wd)
    g = dict(probe.state_dict()["param_groups"][0])
    g.pop("params")
    return g


def optimizer_state_dict(eng) -> dict:
    """the engine's fused-Adam state in torch.optim.Adam.state_dict() layout"""
    names = list(eng.PRM.keys())
    state = {}
    if eng.step_count > 0:  # torch creates the per-parameter state lazily at the first step
        for i, k in enumerate(names):
            o, n = eng.offsets[k]
            state[i] = {"step": torch.tensor(float(eng.step_count)),
                        "exp_avg": eng.flat_m[o:o + n].detach().cpu().clone().view(eng.shapes[k]),
                        "exp_avg_sq": eng.flat_v[o:o + n].detach().cpu().clone().view(eng.shapes[k])}
    group = _adam_group_defaults(eng.lr, eng.wd, eng.optimizer_kind)
    group["params"] = list(range(len(names)))
    return {"state": state, "param_groups": [group]}


def grouped_optimizer_state_dict(eng, groups, updated=None) -> dict:
    """the fused-Adam state under parameter groups, as torch.optim.Adam.state_dict() lays it out: ``param_groups`` has one entry per
    group ({'params': [parameter names], 'lr', 'weight_decay'} each), parameter ids count through the groups in order, and ``state``
    holds only the parameters named in `updated` (default: every grouped parameter once a step has run) -- torch creates a
    parameter's state at its first update, so a frozen one has none.  ``step`` is the engine's one counter for all of them."""
    state, out_groups, i = {}, [], 0
    for g in groups:
        ks = list(g["params"])
        for k in ks:
            if eng.step_count > 0 and (updated is None or k in updated):
                o, n = eng.offsets[k]
                state[i] = {"step": torch.tensor(float(eng.step_count)),
                            "exp_avg": eng.flat_m[o:o + n].detach().cpu().clone().view(eng.shapes[k]),
                            "exp_avg_sq": eng.flat_v[o:o + n].detach().cpu().clone().view(eng.shapes[k])}
            i += 1
        og = _adam_group_defaults(float(g["lr"]), float(g.get("weight_decay", 0.0)), eng.optimizer_kind)
        if "initial_lr" in g:
            og["initial_lr"] = g["initial_lr"]
        og["params"] = list(range(i - len(ks), i))
        out_groups.append(og)
    return {"state": state, "param_groups": out_groups}


def load_optimizer_state(eng, opt_sd: dict, use_saved_lr: bool = True, names=None) -> None:
    """inverse of optimizer_state_dict / grouped_optimizer_state_dict; accepts what the reference's torch.optim.Adam wrote.
    names: the parameter names the file's ids count through, group after group (default: every parameter in registration
    order); the moments of every other parameter are zeroed"""
    names = list(eng.PRM.keys()) if names is None else list(names)
    groups = opt_sd["param_groups"]
    ids = [i for g in groups for i in g["params"]]
    if len(ids) != len(names):
        raise ValueError(f"loaded state dict contains {len(ids)} parameters, the model has {len(names)} "
                         "(torch.optim.Optimizer.load_state_dict raises the same way)")
    g0 = groups[0]
    for g in groups:
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("amsgrad / maximize checkpoints are not supported (the reference uses neither, dpc/main.py:80-81)")
        if tuple(g.get("betas", (0.9, 0.999))) != (0.9, 0.999) or float(g.get("eps", 1e-8)) != 1e-8:
            raise ValueError("non-default Adam betas / eps in the checkpoint (the reference uses the defaults)")
    # validate everything BEFORE touching the arenas: a rejected file must leave the engine's Adam state as it was
    steps, todo = set(), []
    for pos, i in enumerate(ids):
        st = opt_sd["state"].get(i)
        if st is None:
            continue
        k = names[pos]
        for field in ("exp_avg", "exp_avg_sq"):
            if tuple(st[field].shape) != tuple(eng.shapes[k]):
                raise ValueError(f"optimizer state {i} ({field}) has shape {tuple(st[field].shape)}, parameter {k} is {eng.shapes[k]}")
        steps.add(int(float(st["step"])))
        todo.append((k, st))
    if len(steps) > 1:
        raise ValueError(f"per-parameter Adam step counts differ ({sorted(steps)}): the fused optimizer keeps one")
    eng.flat_m.zero_()
    eng.flat_v.zero_()
    for k, st in todo:
        o, n = eng.offsets[k]
        eng.flat_m[o:o + n].copy_(st["exp_avg"].reshape(-1).to(torch.float32))
        eng.flat_v[o:o + n].copy_(st["exp_avg_sq"].reshape(-1).to(torch.float32))
    eng.step_count = steps.pop() if steps else 0
    if use_saved_lr:  # optimizer.load_state_dict restores the group's hyper-parameters (dpc/main.py:97-98)
        eng.lr = float(g0["lr"])
        eng.wd = float(g0.get("weight_decay", eng.wd))


def load_model_state(eng, state_dict: "Dict[str, torch.Tensor]", strict: bool = True) -> Tuple[List[str], List[str]]:
    """strict=True: nn.Module.load_state_dict semantics (dpc/main.py:96) -- raises RuntimeError on missing or
    unexpected keys or a shape mismatch.  strict=False: neq_load_customized (backbone/resnet_2d3d.py:310-333) --
    keys present on both sides are loaded, the rest is reported.  Returns (missing, unexpected)."""
    sd = {_strip(k): v for k, v in state_dict.items()}
    bufs = getattr(eng, "BUF", {})  # BatchNorm running buffers of the LC classifier's engine (empty for DPC-RNN)
    mine = set(eng.PRM.keys()) | set(bufs.keys())
    aliases = {k.replace(ALIAS_FROM, ALIAS_TO) for k in mine if k.startswith(ALIAS_FROM)}
    unexpected = [k for k in sd if k not in mine and k not in aliases]
    missing = [k for k in list(eng.PRM.keys()) + list(bufs.keys()) + sorted(aliases) if k not in sd]
    if strict and (missing or unexpected):
        raise RuntimeError(f"Error(s) in loading state_dict for {'LC' if bufs else 'DPC_RNN'}:\n\tMissing key(s) in state_dict: "
                           f"{missing}.\n\tUnexpected key(s) in state_dict: {unexpected}.")
    load = {}
    for k, v in sd.items():
        tgt = k.replace(ALIAS_TO, ALIAS_FROM) if k in aliases else k
        if tgt not in mine:
            continue
        want = tuple(eng.shapes[tgt]) if tgt in eng.shapes else tuple(bufs[tgt].shape)
        if tuple(v.shape) != want:
            raise RuntimeError(f"size mismatch for {k}: copying a param with shape {tuple(v.shape)} from checkpoint, "
                               f"the shape in current model is {want}.")
        if tgt in load and k in aliases:
            continue  # the cell's own key wins over its alias (they hold the same tensor in reference files)
        load[tgt] = v
    eng.load_params(load)
    return missing, unexpected


def ema_entry(eng, keys: Iterable[str]) -> dict:
    """the checkpoint's top-level 'ema' entry while the engine keeps a parameter average (BackboneEngine.set_ema): the decay and the
    averaged model under the keys of the file's 'state_dict', in their order (prefixed, alias keys, CPU; running buffers, which are
    not averaged, as they are).  The reference reads named keys only, so a file with this entry still resumes there."""
    av = eng.ema_state_dict()
    return {"decay": float(eng.ema_decay), "state_dict": {k: av[_strip(k)].cpu() for k in keys}}


def lr_schedule_entry(eng) -> dict:
    """the checkpoint's top-level 'lr_schedule' entry while the engine steps by a schedule (BackboneEngine.set_lr_schedule): the
    schedule's own fields.  The optimizer's 'lr' stays the base value and the multiplier is a function of the step count the optimizer
    state already holds, so the reference resumes the file as before and nothing else needs storing."""
    return eng.lr_schedule.to_dict()


def check_lr_schedule(eng, ck: dict, path: str) -> None:
    """a resumed run takes its schedule from the flags or the caller, never from the file; one warning if the file was written under
    another one (or the run has none).  A file without the entry says nothing."""
    if "lr_schedule" not in ck:
        return
    mine = eng.lr_schedule.to_dict() if eng.lr_schedule is not None else None
    if mine != ck["lr_schedule"]:
        warnings.warn(f"{path} was written under the learning-rate schedule {ck['lr_schedule']}, this run continues with {mine}")


def check_optimizer_kind(eng, ck: dict, path: str) -> None:
    """a resumed run takes its update rule from the flags or the caller, never from the file; one warning if the file was written
    under another one.  A file without the entry (every Adam run's) says nothing."""
    if "optimizer_kind" in ck and ck["optimizer_kind"] != eng.optimizer_kind:
        warnings.warn(f"{path} was written under the optimizer {ck['optimizer_kind']}, this run continues with {eng.optimizer_kind}")


def check_accum_steps(eng, ck: dict, path: str) -> None:
    """a resumed run takes its accumulation from the flags or the caller, never from the file; one warning if the file was written
    under another count.  A file without the entry (every run's without accumulation) counts as 1."""
    if int(ck.get("accum_steps", 1)) != eng.accum_steps:
        warnings.warn(f"{path} was written with {int(ck.get('accum_steps', 1))} micro-batches per optimizer step, this run continues "
                      f"with {eng.accum_steps}")


def check_neg_queue(eng, ck: dict, path: str) -> None:
    """the negative queue is not in the file (it refills in K batches) and a resumed run takes its K from the flags or the caller; one
    warning if the file was written under another K.  A file without the entry (every run's without the queue) counts as 0."""
    k = int(getattr(eng, "neg_queue", 0))
    if int(ck.get("neg_queue", 0)) != k:
        warnings.warn(f"{path} was written with a negative queue of {int(ck.get('neg_queue', 0))} batches, this run continues with {k}")


def check_neg_weight(eng, ck: dict, path: str) -> None:
    """the class weights of the training loss are a loss knob, not the model: a resumed run takes them from the flags or the caller, and
    there is one warning if the file was written under others.  A file without the entry (every run's at weights 1, 1, 1) counts as
    (1, 1, 1)."""
    w = tuple(getattr(eng, "neg_classes", ((1.0, 1.0, 1.0), False))[0])
    e = ck.get("neg_weight") or {}
    was = (float(e.get("spatial", 1.0)), float(e.get("temporal", 1.0)), float(e.get("easy", 1.0)))
    if was != w:
        warnings.warn(f"{path} was written with the negative-class weights spatial {was[0]:g} temporal {was[1]:g} easy {was[2]:g}, this run "
                      f"continues with spatial {w[0]:g} temporal {w[1]:g} easy {w[2]:g}")


def check_loss_sym(eng, ck: dict, path: str) -> None:
    """the weight of the symmetric loss's column direction is a property of the loss, not of the model: a resumed run takes it from the
    flags or the caller, and there is one warning if the file was written under another.  A file without the entry counts as 0."""
    w = float(getattr(eng, "loss_sym", 0.0))
    was = float(ck.get("loss_sym", 0.0))
    if was != w:
        warnings.warn(f"{path} was written with the symmetric-loss weight {was:g}, this run continues with {w:g}")


def check_score_norm(eng, ck: dict, path: str) -> None:
    """the form of the score is part of the model: a file written under another form or temperature than the run's is another model,
    whose loss and validation numbers do not continue this one's -- an error, not a warning.  A file without the entry (every run's
    with the dot-product score) counts as ("dot", 1)."""
    kind, t = getattr(eng, "score_norm", ("dot", 1.0))
    entry = ck.get("score_norm") or {"kind": "dot", "temperature": 1.0}
    if entry.get("kind") != kind or float(entry.get("temperature", 1.0)) != float(t):
        raise ValueError(f"{path} was trained with the {entry.get('kind')} score at temperature {float(entry.get('temperature', 1.0)):g}, "
                         f"this run scores {kind} at temperature {float(t):g}: a different model (set --score_norm / --temperature, or "
                         "set_score_norm, to the file's)")


def build_state(eng, epoch: int, net: str, best_acc: float, iteration: int) -> dict:
    """the dictionary of dpc/main.py:167-172 (epoch = the NEXT epoch to run, as the reference stores epoch+1); with the learning-rate
    schedule on, plus 'lr_schedule' (lr_schedule_entry); with the parameter average on, plus 'ema' (ema_entry); under another update
    rule than Adam, plus 'optimizer_kind' ("adamw" / "lamb"); under gradient accumulation, plus 'accum_steps'; with the negative queue on,
    plus 'neg_queue' (its slot count -- the bank is not in the file); with class weights other than (1, 1, 1) in the loss, plus
    'neg_weight' ({'spatial', 'temporal', 'easy'}); under the symmetric loss, plus 'loss_sym' (its weight); under the cosine score, plus 'score_norm' ({'kind', 'temperature'}).  Refused while an
    accumulation cycle is open: the sum so far is not part of the file"""
    eng._not_swapped("build_state")
    eng._not_mid_cycle("build_state")
    state = {"epoch": epoch, "net": net, "state_dict": model_state_dict(eng), "best_acc": best_acc,
             "optimizer": optimizer_state_dict(eng), "iteration": iteration}
    if eng.lr_schedule is not None:
        state["lr_schedule"] = lr_schedule_entry(eng)
    if eng.ema_decay is not None:
        state["ema"] = ema_entry(eng, state["state_dict"])
    if eng.optimizer_kind != "adam":
        state["optimizer_kind"] = eng.optimizer_kind
    if eng.accum_steps > 1:
        state["accum_steps"] = eng.accum_steps
    if getattr(eng, "neg_queue", 0) > 0:   # the slot count only: the bank itself is never written
        state["neg_queue"] = eng.neg_queue
    nw = tuple(getattr(eng, "neg_classes", ((1.0, 1.0, 1.0), False))[0])
    if nw != (1.0, 1.0, 1.0):
        state["neg_weight"] = {"spatial": nw[0], "temporal": nw[1], "easy": nw[2]}
    if getattr(eng, "loss_sym", 0.0) > 0:
        state["loss_sym"] = float(eng.loss_sym)
    if getattr(eng, "score_norm", ("dot", 1.0))[0] != "dot":
        state["score_norm"] = {"kind": eng.score_norm[0], "temperature": eng.score_norm[1]}
    return state


def averaged_state_dict(eng, ck: dict, path: str) -> "Dict[str, torch.Tensor]":
    """the file's model with its parameters taken from ck['ema']['state_dict'] (--use_ema); buffers still come from 'state_dict'"""
    if "ema" not in ck or "state_dict" not in ck["ema"]:
        raise KeyError(f"{path} holds no averaged weights (no 'ema' entry: it was written without --ema)")
    bufs = getattr(eng, "BUF", {})
    sd = dict(ck["state_dict"])
    sd.update({k: v for k, v in ck["ema"]["state_dict"].items() if _strip(k) not in bufs})
    return sd


def load_ema_state(eng, ck: dict, path: str) -> None:
    """after the file's parameters were loaded (load_params has seeded flat_ema with them): the file's average into flat_ema.  With
    the average off the file's entry is ignored; on and the file has none: one warning, the seed stays."""
    if eng.ema_decay is None:
        return
    if "ema" not in ck:
        warnings.warn(f"{path} holds no averaged weights: the average starts from the loaded parameters")
        return
    sd = {_strip(k): v for k, v in ck["ema"]["state_dict"].items()}
    for k, (o, n) in eng.offsets.items():
        eng.flat_ema[o:o + n].copy_(sd[k].to(torch.float32).reshape(-1))


def save_checkpoint(state: dict, is_best: bool = False, gap: int = 1, filename: str = "models/checkpoint.pth.tar",
                    keep_all: bool = False) -> None:
    """utils/utils.py:14-26: write, drop the previous epoch's file, keep ONE model_best_* file"""
    torch.save(state, filename)
    d = os.path.dirname(filename)
    if not keep_all:
        last = os.path.join(d, "epoch%s.pth.tar" % str(state["epoch"] - gap))
        if os.path.exists(last):
            os.remove(last)
    if is_best:
        for old in glob.glob(os.path.join(d, "model_best_*.pth.tar")):
            try:
                os.remove(old)
            except OSError:
                pass
        torch.save(state, os.path.join(d, "model_best_epoch%s.pth.tar" % str(state["epoch"])))


def resume(eng, path: str, reset_lr: bool = False, check_schedule: bool = True) -> dict:
    """--resume (dpc/main.py:88-102): strict model load, optimizer state unless reset_lr.  Returns the bookkeeping
    fields {'epoch', 'iteration', 'best_acc'}, plus the file's 'lr_schedule' entry when it has one.  The learning-rate schedule is not
    read from the file: the engine's own is compared with it (check_lr_schedule) -- unless check_schedule is False, for a caller
    that sets its schedule only after the load and compares then."""
    ck = torch.load(path, map_location="cpu", weights_only=False)
    check_score_norm(eng, ck, path)   # before anything is loaded: a file of another score form leaves the engine as it was
    load_model_state(eng, ck["state_dict"], strict=True)
    if not reset_lr:
        if "optimizer" in ck:
            load_optimizer_state(eng, ck["optimizer"])
        elif "optimizer_flat" in ck:  # files written by round 1 of this build
            st = ck["optimizer_flat"]
            eng.flat_m.copy_(st["m"])
            eng.flat_v.copy_(st["v"])
            eng.step_count = int(st["step"])
        else:
            warnings.warn(f"{path} holds no optimizer state: Adam moments and step count start from zero")
    load_ema_state(eng, ck, path)
    check_optimizer_kind(eng, ck, path)
    check_accum_steps(eng, ck, path)
    check_neg_queue(eng, ck, path)   # (load_params above has emptied the bank)
    check_neg_weight(eng, ck, path)
    check_loss_sym(eng, ck, path)
    if check_schedule:
        check_lr_schedule(eng, ck, path)
    info = {"epoch": ck["epoch"], "iteration": ck.get("iteration", 0), "best_acc": ck.get("best_acc", 0.0)}
    if "lr_schedule" in ck:
        info["lr_schedule"] = ck["lr_schedule"]
    return info


def pretrain(eng, path: str, log=print, use_ema: bool = False) -> dict:
    """--pretrain (dpc/main.py:104-112): key-intersection load, with the reference's report of unused keys.
    use_ema: the parameters come from the file's averaged weights (KeyError when it has none)"""
    ck = torch.load(path, map_location="cpu", weights_only=False)
    missing, unexpected = load_model_state(eng, averaged_state_dict(eng, ck, path) if use_ema else ck["state_dict"], strict=False)
    log("\n=======Check Weights Loading======")
    log("Weights not used from pretrained file:")
    for k in unexpected:
        log(k)
    log("---------------------------")
    log("Weights not loaded into new model:")
    for k in missing:
        log(k)
    log("===================================\n")
    return {"epoch": ck.get("epoch", 0)}
