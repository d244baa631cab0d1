"""Resumable checkpoints.

The reference pickles the whole module object each epoch (`torch.save(model, ...)`, TRAIN:464-472) and keeps no optimizer,
scheduler or RNG state, so a run can be evaluated but not resumed.  Here a checkpoint is a plain dict of tensors keyed by
the REFERENCE's parameter names (the modules mirror `src/models`, so `state_dict()` of a reference model built from the
same config loads it and vice versa), plus everything the continuation of a run depends on — weights, AdamW moments, schedule position and
the dropout RNG are restored EXACTLY (the first step after a resume reproduces the uninterrupted run to fp32 round-off, 2e-5); later steps
agree to ~1e-3 because a step itself is not run-to-run deterministic: the split-K weight gradients, the LayerNorm parameter gradients and the
embedding scatter sum through fp32 atomics whose order varies (VACNIC_WGRAD_GROUP_MAX_M=1000000 removes the first source):
  model      {reference parameter name: fp32 tensor}   (the fp32 master copies; the bf16 shadow is derived)
  optimizer  {"exp_avg": {name: tensor}, "exp_avg_sq": {name: tensor}, "lr": float, "step": int}   — torch.optim.AdamW layout;
             with FusedAdamW(skip_nonfinite=True) also "skipped": steps dropped so far (absent = 0; the run of consecutive drops
             restarts at 0).  "step" counts the steps APPLIED: it lags meta["step"], the trainer's data position, by "skipped";
             the two are restored separately.  With FusedAdamW(ema_decay=...) also "ema": {name: tensor}, the moving average of
             the weights (load_checkpoint(..., weights="ema") loads it as the model's weights).  With FusedAdamW(accum_steps=k > 1)
             also "groups": groups of k batches completed so far (applied or dropped; absent = 0).
  schedule   {"base_lr", "num_warmup_steps", "num_training_steps", ...; "param_groups": the optimizer's parameter-group spec as plain
             data — present only when it has one; loading into an optimizer with another spec (or none) raises;
             "ema_decay", "ema_warmup": present only with an average, informative (a resume may choose another decay);
             "accum_steps": batches per optimizer step (absent = 1).  A checkpoint is written on a group boundary only (no
             half-accumulated gradient is stored), and loads into an optimizer with the same accum_steps only: the schedule
             is sized in optimizer steps and meta["step"], the data position, in batches}
  rng        {"seed", "counter", "device_counter"}      — Philox dropout seeds (ops.Rng); `seed` is rank-free, rank r uses seed + r
  meta       {"format": 1, "step": int, ...caller extras}
Everything is moved to the CPU before `torch.save`, so a checkpoint loads on any box."""
import torch

from . import ops
from .ddp import DistributedDataParallel

FORMAT = 1


def _net(model):
    return model.module if isinstance(model, DistributedDataParallel) else model


def _named_trainable(net):
    seen = set()
    for name, p in net.named_parameters():
        if name.startswith("clip_model.") or id(p) in seen:
            continue
        seen.add(id(p))
        yield name, p


def model_state(model):
    """reference-named fp32 weights (tied lm_head / decoder embedding listed once, under `model.shared.weight`, plus the
    aliases the reference's state_dict carries)."""
    net = _net(model)
    sd = {}
    for name, t in net.state_dict().items():
        if name.startswith("clip_model."):
            continue
        sd[name] = t.detach().to("cpu", torch.float32).clone()
    return sd


def optimizer_state(model, optimizer):
    net, a = _net(model), optimizer.arena
    with_ema = getattr(optimizer, "ema_decay", None) is not None
    ea, es, em = {}, {}, {}
    for name, p in _named_trainable(net):
        if id(p) not in a.slots:
            continue
        o, n, _ = a.slots[id(p)]
        ea[name] = a.exp_avg[o:o + n].view(p.shape).detach().cpu().clone()
        es[name] = a.exp_avg_sq[o:o + n].view(p.shape).detach().cpu().clone()
        if with_ema:
            em[name] = a.ema[o:o + n].view(p.shape).detach().cpu().clone()
    hyper = optimizer.hyper.detach().cpu()
    sd = {"exp_avg": ea, "exp_avg_sq": es, "lr": float(hyper[0]), "step": int(hyper[1])}
    if with_ema:
        sd["ema"] = em
    if getattr(optimizer, "guard", None) is not None:
        sd["skipped"] = int(optimizer.guard[1].item())
    if getattr(optimizer, "accum", None) is not None:
        _, pending, groups, _ = optimizer.accum.tolist()       # (the device is idle: hyper was read above)
        if pending != 0:
            raise RuntimeError(f"save_checkpoint in the middle of an accumulation group: {pending} of {optimizer.accum_steps} batches "
                               "are summed in the gradient arena, which a checkpoint does not store; save after the group's last batch")
        sd["groups"] = int(groups)
    return sd


def save_checkpoint(path, model, optimizer=None, step=0, rank=0, **extra):
    """rank: the saving process's data-parallel rank (its dropout seed offset)."""
    if getattr(optimizer, "ema_swapped", False):
        raise RuntimeError("save_checkpoint inside ema_weights(): the file would label the average as the weights; save outside it "
                           "(the average is stored either way: load_checkpoint(..., weights='ema') reads it)")
    ck = {"model": model_state(model), "meta": dict(extra, format=FORMAT, step=int(step))}
    if optimizer is not None:
        ck["optimizer"] = optimizer_state(model, optimizer)
        ck["schedule"] = {"base_lr": optimizer.lr, "num_warmup_steps": optimizer.warmup, "num_training_steps": optimizer.total,
                          "weight_decay": optimizer.wd, "betas": tuple(optimizer.betas), "eps": optimizer.eps}
        if getattr(optimizer, "param_groups", None) is not None:
            ck["schedule"]["param_groups"] = [dict(e, match=list(e["match"]) if isinstance(e["match"], list) else e["match"])
                                              for e in optimizer.param_groups]
        if getattr(optimizer, "ema_decay", None) is not None:
            ck["schedule"].update(ema_decay=optimizer.ema_decay, ema_warmup=optimizer.ema_warmup)
        if getattr(optimizer, "accum_steps", 1) != 1:
            ck["schedule"]["accum_steps"] = optimizer.accum_steps
    dev = ops.Rng.dev
    # `seed` is the run's seed WITHOUT the saving rank's offset (the trainer seeds rank r with seed + r): a resumed rank
    # re-derives its own base, so the data-parallel replicas keep drawing different dropout masks
    ck["rng"] = {"seed": (ops.Rng.base - int(rank)) & 0xFFFFFFFF, "counter": ops.Rng.counter,
                 "device_counter": int(dev.item()) if dev is not None else 0}
    torch.save(ck, path)
    return ck


def ema_as_model(ck):
    """A checkpoint dict like `ck` whose "model" entry holds the stored moving average of every parameter that has one in place of
    its weights (keyed like the moments: by a parameter's first name) — what load_checkpoint(..., weights="ema") loads, and what
    tools/export_ema.py writes as a file of its own, which any loader of checkpoints then reads as plain weights (the stand-alone
    caption generator among them).  Optimizer state, schedule and RNG are dropped: the result is for inference, not for a resume;
    meta gains "weights": "ema".  KeyError if `ck` stores no average.  Tensors are shared with `ck`, nothing is copied."""
    stored = ck.get("optimizer", {}).get("ema")
    if not stored:
        raise KeyError("the checkpoint stores no moving average of the weights (it was written without ema_decay)")
    return {"model": dict(ck["model"], **stored), "meta": dict(ck.get("meta", {}), weights="ema")}


def load_checkpoint(path_or_dict, model, optimizer=None, strict=True, rank=0, weights="model"):
    """restore weights (+ optimizer moments, LR-schedule position and dropout RNG when an optimizer is given); returns meta.
    weights="ema": the model gets the stored moving average of every parameter that has one in place of its weights (inference from
    a training checkpoint); KeyError if the checkpoint holds none.
    The average of an optimizer built with ema_decay: restored when the checkpoint has one (whatever decay it was written with — the
    optimizer's own holds from here on), otherwise set to the restored weights.  An optimizer without one ignores a stored average."""
    ck = torch.load(path_or_dict, map_location="cpu", weights_only=False) if isinstance(path_or_dict, (str, bytes)) or hasattr(path_or_dict, "read") else path_or_dict
    if ck.get("meta", {}).get("format") != FORMAT:
        raise ValueError(f"unknown checkpoint format {ck.get('meta', {}).get('format')!r}")
    if weights not in ("model", "ema"):
        raise ValueError(f"load_checkpoint: weights={weights!r} must be 'model' or 'ema'")
    if getattr(optimizer, "ema_swapped", False):
        raise RuntimeError("load_checkpoint inside ema_weights(): the weights and their average are swapped")
    net = _net(model)
    stored_ema = ck.get("optimizer", {}).get("ema")
    sd = ema_as_model(ck)["model"] if weights == "ema" else ck["model"]
    # every refusal comes before the first write: a load that raises leaves the model, the optimizer and its average as they were
    own = {k for k in net.state_dict().keys() if not k.startswith("clip_model.")}
    missing, unexpected = sorted(own - set(sd)), sorted(set(sd) - own)
    if strict and (missing or unexpected):
        raise KeyError(f"checkpoint/model mismatch: missing {missing[:4]}, unexpected {unexpected[:4]}")
    targets = [(name, p) for name, p in list(net.named_parameters()) + list(net.named_buffers()) if name in sd]
    for name, p in targets:
        if tuple(sd[name].shape) != tuple(p.shape):
            raise ValueError(f"shape mismatch for {name}: {tuple(sd[name].shape)} vs {tuple(p.shape)}")
    if optimizer is not None and "optimizer" in ck:
        # the moments of a parameter mean what its group made of them: resume with the spec the run was started with
        saved, mine = ck.get("schedule", {}).get("param_groups"), getattr(optimizer, "param_groups", None)
        if saved != mine:
            raise ValueError(f"checkpoint was written with param_groups={saved!r}, the optimizer has param_groups={mine!r}")
        saved, mine = int(ck.get("schedule", {}).get("accum_steps", 1)), getattr(optimizer, "accum_steps", 1)
        if saved != mine:
            raise ValueError(f"checkpoint was written with accum_steps={saved}, the optimizer has accum_steps={mine}: the schedule "
                             "position counts optimizer steps of that many batches")
    with torch.no_grad():
        for name, p in targets:
            p.data.copy_(sd[name])
    if getattr(net, "arena", None) is not None:
        net.arena.refresh_shadow()                       # bf16 compute copies follow the restored fp32 masters
    if getattr(optimizer, "ema_decay", None) is not None:
        a = optimizer.arena
        a.ema.copy_(a.flat32)                            # no stored average (or none for some parameter): the restored weights
        for name, p in _named_trainable(net):
            if stored_ema and name in stored_ema and id(p) in a.slots:
                off, n, _ = a.slots[id(p)]
                a.ema[off:off + n].copy_(stored_ema[name].reshape(-1))
    if optimizer is not None and "optimizer" in ck:
        a, o = optimizer.arena, ck["optimizer"]
        a.exp_avg.zero_(); a.exp_avg_sq.zero_()
        for name, p in _named_trainable(net):
            if name in o["exp_avg"] and id(p) in a.slots:
                off, n, _ = a.slots[id(p)]
                a.exp_avg[off:off + n].copy_(o["exp_avg"][name].reshape(-1))
                a.exp_avg_sq[off:off + n].copy_(o["exp_avg_sq"][name].reshape(-1))
        optimizer.hyper.copy_(torch.tensor([o["lr"], float(o["step"])]))
        if getattr(optimizer, "guard", None) is not None:
            optimizer.guard.copy_(torch.tensor([0, int(o.get("skipped", 0)), 0, -1], dtype=torch.int64))
        if getattr(optimizer, "accum", None) is not None:
            optimizer.accum.copy_(torch.tensor([0, 0, int(o.get("groups", 0)), 0], dtype=torch.int64))
            a.grad.zero_()                               # a group begins: no batch of the run loaded over is pending any more
        r = ck.get("rng")
        if r is not None:
            seed = r["seed"] if "seed" in r else r["base"]          # "base": checkpoints written before the per-rank fix
            ops.Rng.base = (int(seed) + int(rank)) & 0xFFFFFFFF      # per-rank base: replicas must not share dropout masks
            ops.Rng.counter = r["counter"]
            if optimizer.hyper.is_cuda:
                ops.Rng.device_counter().fill_(r["device_counter"])
    return ck["meta"]
