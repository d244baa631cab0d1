"""One VACNIC training step on gfx950 kernels — the body of train_epoch (TRAIN:253-383) without the
host syncs: ViT features -> multimodal BART (+ fused lm_head/CE) -> frozen guide BART -> CoLaM ->
SECLA -> backward -> DDP all-reduce -> fused AdamW with on-device linear-warmup schedule.
"""
import contextlib
import math
from dataclasses import dataclass

import torch

from . import kernels as K
from . import ops
from . import streams
from .config import ClipVisionConfig, VacnicConfig
from .ddp import DistributedDataParallel
from .models.clip_vit import CLIPVisualOnly, extract_clip_img_feat
from .models.guide_bart import BartForConditionalGeneration
from .models.mmbart import BartForMultiModalGeneration


@dataclass
class TrainArgs:
    """the trainer flags that shape the step (names/defaults of TRAIN:5-82, values of run_full_train.sh)."""
    lr_bart: float = 3e-5
    weight_decay: float = 0.01
    warmup_rate: float = 0.05
    num_training_steps: int = 100000
    margin: float = 1.0
    alpha: float = 0.5
    mapping_loss_weight: float = 1.0
    use_secla: bool = True
    no_mapping: bool = False
    no_clip_norm: bool = True
    clip_norm: float = 0.1
    prompt_mlp_type: str = "clipcap"
    # parameter groups (param_group_spec): all off = one learning rate and one weight decay for every parameter, nothing frozen
    no_decay_bias_ln: bool = False        # --no_decay_bias_ln: weight decay 0 on every bias and LayerNorm parameter
    lr_scale: tuple = ()                  # --lr_scale REGEX=FLOAT (repeatable): ((regex, multiple of the scheduled lr), ...)
    freeze: tuple = ()                    # --freeze REGEX (repeatable)
    skip_nonfinite: bool = False          # --skip_nonfinite: drop a step whose reduced gradient is not finite (FusedAdamW)
    ema_decay: float = 0.0                # --ema_decay: moving average of the weights inside the AdamW step (FusedAdamW); 0 = off
    grad_stats_every: int = 0             # --grad_stats_every N: per-parameter gradient / weight statistics every N steps (FusedAdamW)
    grad_accum_steps: int = 1             # --grad_accum_steps K: K batches per optimizer step (FusedAdamW(accum_steps=K)); one process
    deterministic: bool = False           # --deterministic True: the step runs in ops.set_deterministic mode (bitwise reproducible run to run)
    loss_norm: str = "tokens"             # --loss_norm: divisor of a weighted text loss (batch["loss_weights"]): the non-pad tokens, or "weights" = their weight sum


def param_group_spec(model, args: TrainArgs):
    """FusedAdamW(param_groups=...) for the trainers' three flags, or None when all are off.  Order: freeze, then lr_scale, then
    no-decay; every entry sets ONE field and every field resolves by its own first match (arena.resolve_spec), so a parameter can be
    scaled AND un-decayed, and a frozen one stays frozen whatever else matches it."""
    from .arena import no_decay_spec
    spec = [{"match": rx, "frozen": True} for rx in args.freeze]
    spec += [{"match": rx, "lr_scale": float(f)} for rx, f in args.lr_scale]
    if args.no_decay_bias_ln:
        spec += no_decay_spec(model.module if isinstance(model, DistributedDataParallel) else model)
    return spec or None


class FusedAdamW:
    """optim.AdamW(betas=(0.9,0.999), eps=1e-8) + get_linear_schedule_with_warmup (TRAIN:91,99-107) over the
    gradient arena: one lr kernel + one AdamW kernel per step, lr and step counter in device memory."""

    def __init__(self, arena, lr, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8, num_warmup_steps=0.0,
                 num_training_steps=1.0, world_size=1, param_groups=None, named_parameters=None, skip_nonfinite=False,
                 ema_decay=None, ema_warmup=True, grad_stats_every=None, accum_steps=1):
        """accum_steps: k > 1 makes k calls of step() one optimizer step over the mean of k batch gradients (gradient accumulation).
        Backward accumulates into the fp32 gradient arena already; every step() issues the launches of a full step, and a counter on
        the device (K.lr_step_accum) lets the first k - 1 of a group leave at once: weights, moments, the shadow, the average, the
        schedule position and Adam's t stay, the gradient is kept.  The k-th applies AdamW to the sum scaled by 1 / k and zeroes it.
        Eager steps, launch plans and graphs therefore run unchanged, whichever micro-batch they were recorded on.  The guard, the
        clip norm and the statistics see the group's mean gradient, once per group; the dropout counter advances per batch.
        accum_report() reads the counters.  One process only (world_size == 1).  1 (default): the launches of before.
        grad_stats_every: N >= 1 records per-parameter statistics of the averaged gradient and of the weights (K.param_stats:
        norm and largest magnitude of both, non-finite and exactly-zero gradient elements) on every step whose 1-based count is a
        multiple of N, and on every step the guard drops; decided on the device, so eager steps, launch plans and graphs run the
        same launches.  grad_stats() reads the most recent record.  They do not depend on parameter groups (a frozen parameter's
        gradient is computed and reported) and change nothing the step writes.  0 or None (default): off, the launches of before.
        ema_decay: a decay in (0, 1) keeps arena.ema, an fp32 exponential moving average of the weights, updated by the AdamW
        kernel itself (K.adamw_ema: the new weight is in registers there): ema = d ema + (1 - d) p after every applied step, with
        d = ema_decay, or under ema_warmup (default) min(ema_decay, (1 + t) / (10 + t)) for Adam's step count t.  It starts as a
        copy of the weights; frozen parameters and dropped steps leave it alone.  swap_ema() / ema_weights() put it in the weights'
        place for evaluation.  None (default): no average, the launches of before.
        skip_nonfinite: a step whose gradient (averaged over the ranks, frozen parameters left out) holds a NaN or an Inf, or
        whose sum of squares overflows fp32, is dropped whole, decided on the device without a sync (K.grad_guard): p, m, v and
        the shadow stay, the gradient is zeroed, neither Adam's t nor the schedule position advances, and the step is counted
        (guard_report()).  Off (default): the launches and results of before.
        param_groups: a spec (arena.py "parameter groups") giving ranges of the arena their own multiple of the scheduled learning
        rate, their own weight decay, or freezing them — torch.optim.AdamW(param_groups) under one LambdaLR; it needs
        named_parameters=model.named_parameters() to match against.  A frozen parameter keeps p, m, v and its bf16 shadow untouched,
        its gradient is still computed by backward and zeroed by the step, and it does not count in the clip norm.
        None (default): one group, the ungrouped kernels."""
        if ema_decay is not None and not 0.0 < float(ema_decay) < 1.0:
            raise ValueError(f"FusedAdamW: ema_decay={ema_decay!r} must lie in (0, 1) (None: no average)")
        if grad_stats_every is not None and int(grad_stats_every) < 0:
            raise ValueError(f"FusedAdamW: grad_stats_every={grad_stats_every!r} must be >= 0 (0 or None: off)")
        if int(accum_steps) != accum_steps or int(accum_steps) < 1:
            raise ValueError(f"FusedAdamW: accum_steps={accum_steps!r} must be an integer >= 1 (1: every batch is an optimizer step)")
        if int(accum_steps) > 1 and world_size > 1:
            raise ValueError(f"FusedAdamW: accum_steps={accum_steps} with world_size={world_size}: the reducer all-reduces the gradient "
                             "arena in place, so a second micro-batch's reduction would multiply the already reduced sums by the "
                             "world size; accumulation runs in one process")
        self.arena = arena
        arena.init_optimizer_state()
        self.ema_decay, self.ema_warmup = None if ema_decay is None else float(ema_decay), bool(ema_warmup)
        self.ema_swapped = False          # the average currently sits in the weights' place (swap_ema)
        if self.ema_decay is not None:
            arena.init_ema()              # here, not in the first step: a launch plan replays the recorded addresses
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, betas, eps
        self.warmup, self.total = float(num_warmup_steps), float(num_training_steps)
        self.world = world_size
        self.hyper = torch.zeros(2, device=arena.device, dtype=torch.float32)      # {lr, step}
        self.clip = None                  # {clip coefficient, total grad norm} of the last clipped step (device)
        self._clip_scratch = None
        self.param_groups, self.table = None, None
        if param_groups is not None:
            from .arena import normalize_spec
            if named_parameters is None:
                raise ValueError("FusedAdamW(param_groups=...) needs named_parameters=model.named_parameters()")
            self.param_groups = normalize_spec(param_groups)                 # plain data: state_dict() and checkpoints carry it
            # built and validated on the host, uploaded once: no per-step host work
            self.table = arena.group_table(named_parameters, self.param_groups, weight_decay).to(arena.device)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guard = None                 # int64 {skip flag, skipped total, consecutive skips, first non-finite arena index}
        if self.skip_nonfinite:
            # allocated here, not in the first step: a launch plan replays the recorded addresses
            self.guard = K.guard_state(arena.device)
            self.clip = torch.zeros(2, device=arena.device, dtype=torch.float32)
            self._clip_scratch = torch.empty(1024, device=arena.device, dtype=torch.float32)
            self._guard_scratch = torch.empty(1024, device=arena.device, dtype=torch.int64)
        self.accum_steps = int(accum_steps)
        self.accum = None                 # int64 {step word, micro-batches pending, groups completed, 0} (K.lr_step_accum)
        if self.accum_steps > 1:
            # allocated here, not in the first step: a launch plan replays the recorded addresses
            self.accum = K.accum_state(arena.device)
        self.grad_stats_every = int(grad_stats_every or 0)
        self._stats = None                # (table, workspace, out_f, out_i, stamp) of K.param_stats
        if self.grad_stats_every:
            # allocated here, not in the first step: a launch plan replays the recorded addresses
            from .arena import stats_table
            tab = stats_table(arena).to(arena.device)
            self._stats = (tab, K.param_stats_workspace(tab, arena.device),
                           torch.zeros(tab.nslot, 4, device=arena.device, dtype=torch.float32),
                           torch.zeros(tab.nslot, 2, device=arena.device, dtype=torch.int64),
                           torch.zeros(4, device=arena.device, dtype=torch.int64))

    def step(self, clip_norm=None):
        """clip_norm: max total gradient norm (torch.nn.utils.clip_grad_norm_, TRAIN:365-366) or None.  The norm is taken
        over the averaged gradient (after the 1/world scaling), as DDP hands it to clip_grad_norm_ in the reference; the
        coefficient stays in device memory and is applied where the AdamW kernel reads the gradient."""
        a = self.arena
        self._not_swapped("step()")
        scale = self._grad_scale()
        if self.accum is None:
            K.lr_step(self.hyper, self.lr, self.warmup, self.total, ops.Rng.device_counter())   # also advances the dropout counter
        else:
            # the same launches on every micro-batch; on the first k - 1 of a group each of them reads the step word and leaves
            K.lr_step_accum(self.hyper, self.lr, self.warmup, self.total, self.accum, self.accum_steps, ops.Rng.device_counter())
        clip = None
        if self.skip_nonfinite:
            # the guard's norm pass is the clip's: one pass gives the verdict and {coefficient, norm}
            K.grad_guard(a.grad, a.n, self.hyper, self.guard, 0.0 if clip_norm is None else float(clip_norm), self.table,
                         scale, self._clip_scratch, self._guard_scratch, self.clip, hold=self.accum)
            clip = None if clip_norm is None else self.clip
        elif clip_norm is not None:
            if self.clip is None:
                self.clip = torch.zeros(2, device=a.device, dtype=torch.float32)
                self._clip_scratch = torch.empty(1024, device=a.device, dtype=torch.float32)
            if self.accum is not None:         # (the entry point that takes `hold`; without a table it is the ungrouped pass)
                clip = K.grad_clip_coef_groups(a.grad, a.n, float(clip_norm), self.table, scale, self._clip_scratch, self.clip,
                                               hold=self.accum)
            elif self.table is None:
                clip = K.grad_clip_coef(a.grad, a.n, float(clip_norm), scale, self._clip_scratch, self.clip)
            else:
                clip = K.grad_clip_coef_groups(a.grad, a.n, float(clip_norm), self.table, scale, self._clip_scratch, self.clip)
        # the step word AdamW and the statistics read: the guard's verdict (which carries a hold on), else the accumulation counter's
        word = self.guard if self.guard is not None else self.accum
        if self._stats is not None:
            # after the guard (its verdict fires the record of a dropped step), before the update zeroes the gradient
            tab, work, out_f, out_i, stamp = self._stats
            K.param_stats(a.grad, a.flat32, a.n, tab, self.hyper, self.grad_stats_every, word, scale, work, out_f, out_i, stamp)
        self._update(0, a.n, clip, word)

    def _grad_scale(self):
        """what turns the arena's sum into the mean gradient: over the ranks, and over the micro-batches of a group"""
        return 1.0 / (self.world * self.accum_steps)

    def _update(self, start, end, clip, skip):
        """the AdamW launch over arena elements [start, end): the one place that chooses among the three entry points."""
        a = self.arena
        r = slice(start, end)
        bufs = (a.flat32[r], a.grad[r], a.exp_avg[r], a.exp_avg_sq[r], a.flat16[r], self.hyper, end - start)
        kw = dict(beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, grad_scale=self._grad_scale(), zero_grad=True,
                  clip_coef=clip, skip=skip)
        if self.ema_decay is not None:
            K.adamw_ema(*bufs, a.ema[r], self.ema_decay, self.ema_warmup, self.table, start, weight_decay=self.wd, **kw)
        elif self.table is None:
            K.adamw(*bufs, weight_decay=self.wd, **kw)
        else:
            K.adamw_groups(*bufs, self.table, start, **kw)

    def guard_report(self, named_parameters=None):
        """The one method of the guard that synchronises (a 32-byte read): {"skipped": steps dropped so far, "in_a_row": current
        run of consecutive drops, "first_nonfinite": first name (arena.first_names) of the parameter holding the first non-finite
        gradient element of the most recent dropped step — None if there was none, if only the sum of squares overflowed, if the
        element lies in padding, or if no named_parameters are given —, "offset": that element's arena index or -1}."""
        if self.guard is None:
            raise RuntimeError("guard_report(): the optimizer was built with skip_nonfinite=False")
        _, skipped, run, first = (int(x) for x in self.guard.tolist())
        name = None
        if first >= 0 and named_parameters is not None:
            from .arena import name_at
            name = name_at(self.arena, named_parameters, first)
        return {"skipped": skipped, "in_a_row": run, "first_nonfinite": name, "offset": first}

    def accum_report(self):
        """The one method of gradient accumulation that synchronises (a 32-byte read): {"accum_steps": k, "pending": micro-batches
        added to the gradient since the last optimizer step, "groups": groups of k completed so far, dropped ones included}."""
        if self.accum is None:
            raise RuntimeError("accum_report(): the optimizer was built with accum_steps=1")
        _, pending, groups, _ = (int(x) for x in self.accum.tolist())
        return {"accum_steps": self.accum_steps, "pending": pending, "groups": groups}

    def grad_stats(self, named_parameters):
        """The one method of the statistics that synchronises: the most recent record as
        {"fires": records so far, "step": the 1-based step it describes (after a dropped step: the count the guard restored),
         "dropped": the guard dropped that step, "total_grad_norm": float64 sqrt of the sum of the slot sums,
         "params": {first name: {"grad_norm", "grad_absmax", "weight_norm", "weight_absmax", "nonfinite", "zeros", "numel"}}}
        over the gradient averaged over the ranks; non-finite gradient elements are counted and left out of grad_norm and
        grad_absmax.  Names are arena.first_names(): a tied parameter appears once.  Before the first record: "fires": 0 and no
        params."""
        if self._stats is None:
            raise RuntimeError("grad_stats(): the optimizer was built with grad_stats_every=0")
        tab, _, out_f, out_i, stamp = self._stats
        fires, t, dropped, _ = (int(x) for x in stamp.tolist())
        out = {"fires": fires, "step": t, "dropped": bool(dropped), "total_grad_norm": 0.0, "params": {}}
        if fires == 0:
            return out
        from .arena import first_names
        f, c = out_f.double().cpu(), out_i.cpu()
        index = {o: s for s, (o, _) in enumerate(tab.slots)}
        for name, p in first_names(self.arena, named_parameters):
            s = index[self.arena.slots[id(p)][0]]
            out["params"][name] = {"grad_norm": float(f[s, 0].sqrt()), "grad_absmax": float(f[s, 1]), "weight_norm": float(f[s, 2].sqrt()),
                                   "weight_absmax": float(f[s, 3]), "nonfinite": int(c[s, 0]), "zeros": int(c[s, 1]),
                                   "numel": tab.slots[s][1]}
        out["total_grad_norm"] = float(f[:, 0].sum().sqrt())
        return out

    def begin_step(self):
        """first half of step() for a range-wise update (DistributedDataParallel.reduce_and_step): schedule + counters once."""
        if self.skip_nonfinite:
            raise RuntimeError("skip_nonfinite needs the whole reduced gradient before any range is updated: use step()")
        if self.grad_stats_every:
            raise RuntimeError("grad_stats_every needs the whole reduced gradient before any range is zeroed: use step()")
        if self.accum_steps > 1:
            raise RuntimeError("accum_steps > 1 holds the whole update back until the group's last batch: use step()")
        self._not_swapped("begin_step()")
        K.lr_step(self.hyper, self.lr, self.warmup, self.total, ops.Rng.device_counter())

    def step_range(self, start, end):
        """AdamW on arena elements [start, end) (a DDP bucket whose all-reduce has finished); begin_step() comes first."""
        self._update(start, end, None, None)

    def zero_grad(self):
        pass            # fused into step(): the AdamW kernel clears the gradient arena it just consumed (and keeps it on a held micro-batch)

    # ---- moving average of the weights ------------------------------------------------------------------------------------
    def _not_swapped(self, what):
        if self.ema_swapped:
            raise RuntimeError(f"{what} while the averaged weights are swapped in (ema_weights() / swap_ema()): the update would "
                               "train the average and average the weights; swap back first")

    def swap_ema(self):
        """Exchange the weights and their average once: the CONTENTS of arena.flat32 and arena.ema, with the bf16 shadow re-derived
        (one kernel, K.ema_swap).  Addresses stay, so Parameter.data views, launch plans and graphs keep reading the right buffers —
        forward sees the other set of weights through the shadow and through the fp32 views alike.  A second call undoes it
        bitwise.  The caller pairs the calls (ema_weights() does): after an odd number of them step(), save_checkpoint and
        load_checkpoint refuse to run (ema_swapped).  While a launch plan is being recorded it raises: the swap would become part
        of every replayed step."""
        a = self.arena
        if self.ema_decay is None:
            raise RuntimeError("swap_ema(): the optimizer was built without ema_decay")
        if K.recording():
            raise RuntimeError("swap_ema() while a launch plan is being recorded: every replay would swap again")
        K.ema_swap(a.flat32, a.ema, a.flat16)
        for hook in a.refresh_hooks:      # packed copies of weights follow the shadow, as after refresh_shadow()
            hook()
        self.ema_swapped = not self.ema_swapped

    @contextlib.contextmanager
    def ema_weights(self):
        """`with optimizer.ema_weights():` — validation, caption generation or export with the averaged weights: swapped in on entry,
        out on exit (also when the body raises).  step() inside it raises."""
        self._not_swapped("ema_weights()")
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def state_dict(self):
        sd = {"exp_avg": self.arena.exp_avg, "exp_avg_sq": self.arena.exp_avg_sq, "hyper": self.hyper}
        if self.ema_decay is not None:
            sd["ema"] = self.arena.ema
        if self.param_groups is not None:
            sd["param_groups"] = self.param_groups
        return sd


def build_models(cfg: VacnicConfig, vcfg: ClipVisionConfig, device="cuda", seed=0, init="device", state_dicts=None, with_guide=True):
    """Random-init (or state-dict) construction of the three networks of the step, finalized in HBM arenas.
    init='device': N(0, 0.02) drawn on the GPU (fast, for benchmarks); init='synthetic': name-keyed numpy
    weights identical to the oracle's (parity tests)."""
    from . import synthetic
    clip_model = CLIPVisualOnly(vcfg)
    model = BartForMultiModalGeneration(cfg, enc_fusion_layer=cfg.enc_fusion_layer, dim_common=cfg.dim_common, img_size=768,
                                        prompt_mlp_type=cfg.prompt_mlp_type, map_size=cfg.map_size, prompt_size=cfg.prompt_size, clip_model=None,
                                        freeze_clip=True, max_ner_type_len=cfg.max_ner_type_len,
                                        max_ner_type_len_gt=cfg.max_ner_type_len_gt, only_image=cfg.only_image,
                                        init_attn_weight=cfg.init_attn_weight)
    guide = BartForConditionalGeneration(cfg) if with_guide else None      # with_guide=False: inference (no CoLaM teacher)
    if init == "synthetic" or state_dicts is not None:
        sds = state_dicts or (synthetic.make_state_dict(synthetic.mmbart_param_shapes(cfg), seed=seed + 1),
                              synthetic.make_state_dict(synthetic.guide_bart_param_shapes(cfg), seed=seed + 2),
                              synthetic.make_state_dict(synthetic.clip_visual_param_shapes(vcfg), seed=seed + 4, std=0.05))
        load_named(model, sds[0]); load_named(clip_model.visual, sds[2])
        if guide is not None:
            load_named(guide, sds[1])
    model.finalize(device)
    if guide is not None:
        guide.finalize(device)
    clip_model.finalize(device)
    if init == "device" and state_dicts is None:
        # one generator per network: the frozen CLIP tower a trainer drew from `seed` is reproducible without building the guide
        for k, (m, std) in enumerate(((model, cfg.init_std), (guide, cfg.init_std), (clip_model.visual, 0.02))):
            if m is None:
                continue
            g = torch.Generator(device=device).manual_seed(seed + 7919 * k)
            for name, p in m.named_parameters():
                if p.dim() >= 2 or "embedding" in name:
                    p.data.normal_(0.0, std, generator=g)
                elif name.endswith("weight"):
                    p.data.fill_(1.0)
                else:
                    p.data.zero_()
            m.arena.refresh_shadow()
    model.clip_model = clip_model                     # the reference keeps CLIP inside the model (MFULL:1892; TRAIN:274)
    return model, guide, clip_model


def load_named(module, sd):
    params = dict(module.named_parameters())
    missing = [k for k in params if k not in sd and not k.endswith("embed_tokens.weight") and k != "lm_head.weight"]
    if missing:
        raise KeyError(f"state dict lacks {missing[:5]} ...")
    with torch.no_grad():
        for k, p in params.items():
            if k in sd:
                if tuple(sd[k].shape) != tuple(p.shape):
                    raise ValueError(f"shape mismatch for {k}: {tuple(sd[k].shape)} vs {tuple(p.shape)}")
                p.data.copy_(sd[k])


def to_device(batch, device):
    return {k: v.to(device, non_blocking=True) for k, v in batch.items()}


def image_feature_index(cfg):
    """which output of extract_clip_img_feat feeds `image_features`: the ln_post CLS vector for the ClipCap prompt MLP, the
    ln_post patch tokens for `--prompt_mlp_type mlp` (the reference trainers branch the same way at every model call)."""
    return 1 if cfg.prompt_mlp_type == "clipcap" else 0


_PLAN = None          # the PlannedTrainStep being recorded (forward_losses leaves marks in it)


def _tower_host(what, towers, batch=None, ready=None, by_plan=False):
    """The host's part in a step whose frozen towers are hipGraph replays (FrozenTowerGraphs), each action written once:
      'launch'           start both replays for (batch, ready); the compute stream waits for the image feature only
      'join_guide'       the compute stream waits for the guide's output (before the CoLaM loss)
      'towers_consumed'  the towers' static outputs have been read: the next replay may overwrite them
    This is torch-side stream work, which a launch plan cannot hold.  An eager step acts where it stands; while a plan is being
    recorded the point goes to the plan (PlannedTrainStep.mark), which acts through this function (by_plan=True) at recording
    and at the same point of every replay."""
    if _PLAN is not None and not by_plan:
        _PLAN.mark(what)
    elif what == "launch":
        towers.launch(batch, ready)
        torch.cuda.current_stream().wait_event(towers.ev_vit)
        if not by_plan:
            # an eager step hands the tower streams a loader-owned batch, which the allocator may recycle once the caller drops it
            # (a plan's caller keeps its batches resident: no record_stream there — see streams on the allocator's polling cost)
            batch["article_ids"].record_stream(streams.aux_stream())
            batch["caption_ids"].record_stream(streams.aux_stream())
            batch["img_tensor"].record_stream(streams.vit_stream())
    elif what == "join_guide":
        torch.cuda.current_stream().wait_stream(streams.aux_stream())
    elif what == "towers_consumed":
        towers.mark_consumed()


def forward_losses(model, guide, batch, args: TrainArgs, ready=None, towers=None):
    """Forward of one step; returns (total, out4={total, txt, secla, colam}, model_out).  With config.label_smoothing > 0 `txt` is the
    smoothed loss, as torch's CrossEntropyLoss(label_smoothing=) reports it.  `model` may be the DDP wrapper
    (like TRAIN:274 `model.module`).  `ready`: optional event after which the batch tensors are valid in HBM; with side
    streams enabled the frozen towers then start on it instead of on the compute stream's tail (= the previous AdamW)."""
    net = model.module if isinstance(model, DistributedDataParallel) else model
    cfg = net.config
    feat = image_feature_index(cfg)
    if not args.no_mapping and not args.use_secla and not cfg.only_image:
        # TRAIN:331-345 (`--use_secla False`): re-runs the model with add_ner_ffn=False, which the reference's encoder rejects
        # with a mask-shape ValueError (see BartEncoderLayer) — there is no working behaviour to reproduce
        raise ValueError("--use_secla False with --no_mapping False: the reference's pooled face-name branch (TRAIN:331-345) "
                         "fails inside its own encoder (add_ner_ffn=False, attention-mask size); use --use_secla True or --no_mapping True")
    src, tgt = batch["article_ids"], batch["caption_ids"]
    main = torch.cuda.current_stream()
    aux, vis = streams.aux_stream(), streams.vit_stream()
    if aux is None:
        if ready is not None:
            main.wait_event(ready)           # single-stream schedule: the loader's copy stream still has to hand the batch over
        src_mask, _ = K.prep_ids(src, cfg.pad_token_id)                                      # create_src_mask_bart, TRAIN:268
        tgt_mask, tgt_in = K.prep_ids(tgt, cfg.pad_token_id, start_id=cfg.eos_token_id)     # shift_tokens_right, TRAIN:267,296
        img_cls = extract_clip_img_feat(net.clip_model, batch["img_tensor"])[feat]            # TRAIN:274-276
    elif towers is not None:
        # frozen towers as two hipGraph replays on their side streams (FrozenTowerGraphs), started and joined by the host
        # (_tower_host); the id preprocessing runs on the compute stream (inside the plan, when one is recorded)
        _tower_host("launch", towers, batch, ready)
        src_mask, _ = K.prep_ids(src, cfg.pad_token_id)
        tgt_mask, tgt_in = K.prep_ids(tgt, cfg.pad_token_id, start_id=cfg.eos_token_id)
        img_cls, gh = towers.img_cls, towers.gh
    else:
        # id preprocessing + frozen guide forward + frozen ViT on the side streams: they depend only on the batch, so they fill
        # the bubbles of the main chain (and of the previous step's AdamW); launched through kernels.launch_on and ordered by
        # kernels.fence, so that the whole step can be recorded into a launch plan (see streams)
        main_raw, aux_raw, vis_raw = K._stream(), streams.raw("aux"), streams.raw("vit")
        if ready is None:
            K.fence(main_raw, aux_raw)
            K.fence(main_raw, vis_raw)
        else:                                   # (a torch event of the loader: not part of a plan — plans refresh their inputs in place)
            aux.wait_event(ready)
            vis.wait_event(ready)
        with K.launch_on(aux_raw):
            src_mask, _ = K.prep_ids(src, cfg.pad_token_id)
            tgt_mask, tgt_in = K.prep_ids(tgt, cfg.pad_token_id, start_id=cfg.eos_token_id)
        K.fence(aux_raw, main_raw)              # the student needs the masks now, the guide's output only at the CoLaM loss
        with K.launch_on(vis_raw):              # the student's encoder input needs the image feature: ViT goes first
            img_cls = extract_clip_img_feat(net.clip_model, batch["img_tensor"])[feat]
        K.fence(vis_raw, main_raw)              # (before the guide is enqueued: the towers share one stream)
        if guide is not None:
            with K.launch_on(aux_raw):
                gh = guide(input_ids=src, attention_mask=src_mask, decoder_input_ids=tgt_in)["decoder_hidden_states"][-1]   # TRAIN:293-294
    kw = {}
    if not cfg.only_image:
        names_mask, _ = K.prep_ids(batch["names_art_ids"], cfg.pad_token_id)                 # TRAIN:270
        kw = dict(face_features=batch["face_emb"], face_mask=K.face_mask(batch["face_emb"]), name_ids=batch["names_art_ids"],
                  name_mask=names_mask)
    if batch.get("loss_weights") is not None:
        # optional batch key: fp32 [B] (per caption) or [B, T] (per token) weights of the text loss; SECLA and CoLaM do not see them
        kw = dict(kw, loss_weights=batch["loss_weights"], loss_norm=args.loss_norm)
    out = model(input_ids=src, attention_mask=src_mask, decoder_input_ids=tgt_in, image_features=img_cls, labels=tgt,
                output_logits=False, add_ner_ffn=True, output_attentions=False, **kw)         # TRAIN:281 + fused CE (TRAIN:287); the step uses no maps
    txt = out["loss"]
    colam = secla = None
    if guide is not None:
        if aux is None:
            gh = guide(input_ids=src, attention_mask=src_mask, decoder_input_ids=tgt_in)["decoder_hidden_states"][-1]   # TRAIN:293-294
        elif towers is not None:
            _tower_host("join_guide", towers)
        else:
            K.fence(streams.raw("aux"), K._stream())
        colam = ops.ColamFn.apply(out["decoder_hidden_states"][-1], gh, tgt_mask, args.margin, args.alpha)        # TRAIN:296-307
    if towers is not None:
        _tower_host("towers_consumed", towers)
    if args.use_secla and not args.no_mapping and not cfg.only_image:
        enc = net.model.encoder
        ln = enc.layernorm_embedding_ner
        names = K.name_embed_mean(batch["names_ids"], enc.embed_tokens_ner.weight.w16, enc.embed_positions_ner.weight.w16,
                                  ln.weight.data, ln.bias.data, embed_scale=enc.embed_scale)   # get_embedding_ner, TRAIN:327
        secla = ops.SeclaFn.apply(out["hidden_states_face"], names, args.mapping_loss_weight)  # TRAIN:329
    total, out4 = ops.total_loss(txt, secla, colam, args.mapping_loss_weight, args.alpha)      # TRAIN:363
    return total, out4, out


def train_step(model, guide, optimizer, batch, args: TrainArgs, ready=None, towers=None):
    """loss.backward(); optimizer.step(); scheduler.step(); zero_grad()  (TRAIN:364-374) — returns the device-side
    loss vector {total, txt, secla, colam} WITHOUT syncing (the reference's four .item() calls per step are gone).
    args.deterministic: the step runs in ops.set_deterministic mode (so does a plan or a graph recorded from it)."""
    if args.deterministic and not ops.deterministic():
        with ops.deterministic_mode(True):
            return train_step(model, guide, optimizer, batch, args, ready, towers)
    net = model.module if isinstance(model, DistributedDataParallel) else model
    if not net.training:
        net.train()
    ops.begin_step()                         # (a previous step that raised must not leak queued weight gradients into this one)
    total, out4, _ = forward_losses(model, guide, batch, args, ready, towers)
    with torch.autograd.set_multithreading_enabled(False):     # one device: the engine's worker-thread hop only costs host time
        # explicit unit gradient from a persistent constant: backward()'s default ones_like(total) is a fill kernel into a fresh
        # block per step — the one ATen kernel left inside the step (tools/aten_in_step.py), invisible to a launch plan
        total.backward(ops.const_one(total.device))
    ops.flush_wgrads()                       # normally empty (the engine's end-of-backward callback already ran)
    clip = None if args.no_clip_norm else args.clip_norm                         # TRAIN:365-366
    # native reducer: the bucket all-reduces sit ON the weight-gradient stream, and every bucket's AdamW range waits for that
    # bucket's own event — joining the whole stream here would hold AdamW back until the LAST collective has finished
    # (the non-finite guard and the per-parameter statistics, like clipping, need the whole reduced gradient before any range is
    # updated)
    guarded = getattr(optimizer, "skip_nonfinite", False)
    if args.skip_nonfinite and not guarded:
        raise ValueError("TrainArgs.skip_nonfinite needs an optimizer built with FusedAdamW(..., skip_nonfinite=True)")
    if args.ema_decay and getattr(optimizer, "ema_decay", None) is None:
        raise ValueError("TrainArgs.ema_decay needs an optimizer built with FusedAdamW(..., ema_decay=...)")
    stats = getattr(optimizer, "grad_stats_every", 0)
    if args.grad_stats_every and not stats:
        raise ValueError("TrainArgs.grad_stats_every needs an optimizer built with FusedAdamW(..., grad_stats_every=N)")
    accum = getattr(optimizer, "accum_steps", 1)
    if args.grad_accum_steps != accum:
        raise ValueError(f"TrainArgs.grad_accum_steps={args.grad_accum_steps} but the optimizer was built with accum_steps={accum}")
    if accum > 1 and isinstance(model, DistributedDataParallel) and model.active:
        raise ValueError("grad_accum_steps > 1 under an active DistributedDataParallel: the reducer all-reduces the gradient arena in "
                         "place, which would multiply the already reduced micro-batch sums by the world size")
    pipelined = (isinstance(model, DistributedDataParallel) and model.native is not None and model.active and clip is None
                 and not guarded and not stats)
    streams.join_all(skip_wgrad=pipelined)   # side streams -> compute stream
    if isinstance(model, DistributedDataParallel):
        model.reduce_and_step(optimizer, clip)       # all-reduce tail overlapped with the optimizer of the finished buckets
        if pipelined:
            streams.release_keep()           # the last bucket's event is behind everything the weight-gradient stream was given
    else:
        optimizer.step(clip_norm=clip)
    optimizer.zero_grad()
    return out4


def _model_inputs(net, batch, graphed=False):
    """masks + frozen-tower features for one batch, as every reference loop builds them (TRAIN:267-276,408-421,491-504).
    graphed: the image tower as a hipGraph per batch shape (caption generation at batch 1: ~250 launches of microseconds each)."""
    cfg = net.config
    src = batch["article_ids"]
    src_mask, _ = K.prep_ids(src, cfg.pad_token_id)
    if graphed:
        from .models.clip_vit import graphed_clip_img_feat
        feats = graphed_clip_img_feat(net.clip_model)(batch["img_tensor"])[image_feature_index(cfg)]
    else:
        feats = extract_clip_img_feat(net.clip_model, batch["img_tensor"])[image_feature_index(cfg)]
    kw = {}
    if not cfg.only_image:
        names_mask, _ = K.prep_ids(batch["names_art_ids"], cfg.pad_token_id)
        kw = dict(face_features=batch["face_emb"], face_mask=K.face_mask(batch["face_emb"]), name_ids=batch["names_art_ids"],
                  name_mask=names_mask)
    return src, src_mask, feats, kw


@torch.no_grad()
def eval_epoch(model, batches, device="cuda"):
    """TRAIN:391-447 / TRAINV:203-250: teacher-forced validation pass in eval mode.  The validation loss is always the plain NLL
    (config.label_smoothing is a training-loss option), so best-checkpoint selection stays comparable across runs.  Returns (mean of the per-batch text
    cross-entropy, out_dict) with out_dict[step] = {"logit_output": argmax token ids per sample, "gt_cap": target ids} — the
    reference stores the same two things as decoded strings (tokenizers are outside SURVEY §8).  One host sync per batch
    (the `.item()` of TRAIN:441), like the reference."""
    net = model.module if isinstance(model, DistributedDataParallel) else model
    cfg = net.config
    was_training = net.training
    net.eval()
    val_loss, n, out_dict = 0.0, 0, {}
    for step, batch in enumerate(batches):
        batch = to_device(batch, device)
        src, src_mask, feats, kw = _model_inputs(net, batch)
        tgt = batch["caption_ids"]
        _, tgt_in = K.prep_ids(tgt, cfg.pad_token_id, start_id=cfg.eos_token_id)
        out = net(input_ids=src, attention_mask=src_mask, decoder_input_ids=tgt_in, image_features=feats, labels=tgt,
                  output_logits=True, add_ner_ffn=True, label_smoothing=0.0, **kw)
        lg = out["logits"]
        ids = K.argmax_rows(lg.view(-1, lg.shape[-1]), net.V).view(tgt.shape)
        out_dict[step] = {"logit_output": ids.tolist(), "gt_cap": tgt.tolist()}
        val_loss += float(out["loss"].item())
        n += 1
    net.train(was_training)
    return val_loss / max(n, 1), out_dict


def _scored_batches(net, batches, device, totals=None):
    """the teacher-forced pass of eval_epoch over `batches` with the fused validation head: yields (target ids as the batch
    delivered them, forward output) per batch; inputs are built exactly as eval_epoch builds them.  Nothing here waits for the
    device."""
    cfg = net.config
    for batch in batches:
        tgt_in_batch = batch["caption_ids"]
        batch = to_device(batch, device)
        src, src_mask, feats, kw = _model_inputs(net, batch)
        tgt = batch["caption_ids"]
        _, tgt_in = K.prep_ids(tgt, cfg.pad_token_id, start_id=cfg.eos_token_id)
        out = net(input_ids=src, attention_mask=src_mask, decoder_input_ids=tgt_in, image_features=feats, labels=tgt,
                  output_token_stats=True, token_totals=totals, add_ner_ffn=True, **kw)
        yield tgt_in_batch, tgt, out


def _ids_to_lists(tensors):
    """nested lists of several [B, T] id tensors with ONE device-to-host copy (host tensors are read where they are)."""
    on_dev = [t for t in tensors if t.is_cuda]
    flat = torch.cat([t.reshape(-1) for t in on_dev]).cpu() if on_dev else None
    out, pos = [], 0
    for t in tensors:
        if t.is_cuda:
            out.append(flat[pos:pos + t.numel()].view(t.shape).tolist())
            pos += t.numel()
        else:
            out.append(t.tolist())
    return out


@torch.no_grad()
def eval_epoch_fused(model, batches, device="cuda"):
    """eval_epoch with the fused validation head (model(..., output_token_stats=True)): ONE lm_head pass per batch instead of two,
    no [B*T, V] logits, and no host sync per batch — losses, predicted ids and the running totals stay on the device and are
    copied once after the last batch.  Returns (val_loss, out_dict, metrics): val_loss (mean of the per-batch plain-NLL losses)
    and out_dict[step] = {"logit_output", "gt_cap"} mean what eval_epoch's mean; metrics = {"token_accuracy", "perplexity",
    "tokens", "sequences"} over all batches (from the device-side totals: correct / tokens, exp(nll / tokens)) and
    "seq_logprob", the teacher-forced log-likelihood of every sample's caption, in order."""
    net = model.module if isinstance(model, DistributedDataParallel) else model
    was_training = net.training
    net.eval()
    try:
        totals = K.zero_(torch.empty(4, device=device, dtype=torch.float64))
        losses, preds, gts, seq_lp = [], [], [], []
        for tgt_host, tgt, out in _scored_batches(net, batches, device, totals):
            losses.append(out["loss"])
            preds.append(out["token_stats"]["pred_ids"])
            gts.append(tgt_host if not tgt_host.is_cuda else tgt)
            seq_lp.append(out["token_stats"]["seq_logprob"])
        n = len(losses)
        if n == 0:
            return 0.0, {}, {"token_accuracy": 0.0, "perplexity": float("nan"), "tokens": 0, "sequences": 0, "seq_logprob": []}
        nums = torch.cat([totals, torch.stack(losses).double()] + [s.double() for s in seq_lp]).tolist()      # the pass's one wait
        lists = _ids_to_lists(preds + gts)
    finally:
        net.train(was_training)
    nll, tokens, correct, sequences = nums[:4]
    val_loss = 0.0
    for v in nums[4:4 + n]:
        val_loss += float(v)
    out_dict = {step: {"logit_output": lists[step], "gt_cap": lists[n + step]} for step in range(n)}
    metrics = {"token_accuracy": correct / max(tokens, 1.0), "perplexity": math.exp(nll / max(tokens, 1.0)), "tokens": int(tokens),
               "sequences": int(sequences), "seq_logprob": nums[4 + n:]}
    return val_loss / n, out_dict, metrics


@torch.no_grad()
def score_captions(model, batches, device="cuda"):
    """teacher-forced scores of the captions in `batches` (inputs built as eval_epoch builds them) under the model's current
    weights: {"logprob": [...], "tokens": [...], "correct": [...]}, one entry per sample in order — the caption's log-likelihood,
    its number of non-pad tokens and how many of them the model predicts greedily.  One device-to-host copy at the end."""
    net = model.module if isinstance(model, DistributedDataParallel) else model
    was_training = net.training
    net.eval()
    try:
        rows = [torch.stack([o["token_stats"]["seq_logprob"].double(), o["token_stats"]["seq_tokens"].double(),
                             o["token_stats"]["seq_correct"].double()]) for _, _, o in _scored_batches(net, batches, device)]
        cols = torch.cat(rows, 1).tolist() if rows else [[], [], []]
    finally:
        net.train(was_training)
    return {"logprob": cols[0], "tokens": [int(v) for v in cols[1]], "correct": [int(v) for v in cols[2]]}


@torch.no_grad()
def gen_caption_from_loader_bart(model, batches, beam_size, max_length, device="cuda", length_penalty=1.0, plm_type=None, pipeline=True,
                                 **gen_kw):
    """TRAIN:480-530 (the generation half; BLEU/ROUGE/CIDEr/METEOR scoring and detokenisation are outside SURVEY §8):
    out_dict[step] = {"gt": target ids, "gen": generated ids} with `model.generate(num_beams=beam_size, max_length=max_length)`;
    `length_penalty` is the extra knob of the stand-alone generator (DDPINF:38,867).  Arguments the reference leaves to the model's
    config (no_repeat_ngram_size, early_stopping, forced BOS/EOS) default to the hub checkpoint's (config.HUB_GENERATION_DEFAULTS,
    keyed by `plm_type`); `gen_kw` overrides them.  pipeline: overlap the next caption's encoder side with this caption's beam search.
    Sampling: `do_sample=True, beam_size=1` with temperature / top_k / top_p / num_return_sequences / seed in `gen_kw` (generate());
    "gen" then holds num_return_sequences rows per caption, and with return_logprobs=True "logprobs" their per-token log-probs."""
    def entry(batch, gen):
        if isinstance(gen, tuple):
            return {"gt": batch["caption_ids"].tolist(), "gen": gen[0].tolist(), "logprobs": gen[1].tolist()}
        return {"gt": batch["caption_ids"].tolist(), "gen": gen.tolist()}

    net = model.module if isinstance(model, DistributedDataParallel) else model
    was_training = net.training
    net.eval()
    out_dict = {}
    from .config import generation_defaults
    gkw = dict(generation_defaults(plm_type), **gen_kw)        # what `model.generate(num_beams, max_length)` inherits from the hub config
    if pipeline and str(device).startswith("cuda"):
        # two-stage pipeline over the captions (generate.CaptionPipeline): image tower + encoder + cross K/V of caption i + 1 on a side
        # stream while caption i is decoded; same ids as the loop below
        from .generate import CaptionPipeline
        pipe = CaptionPipeline(net, lambda b: _model_inputs(net, b, graphed=True), beam_size, max_length=max_length,
                               length_penalty=length_penalty, add_ner_ffn=True, **gkw)
        with torch.no_grad():
            for step, (batch, gen) in enumerate(pipe(to_device(b, device) for b in batches)):
                out_dict[step] = entry(batch, gen)
        net.train(was_training)
        return out_dict
    for step, batch in enumerate(batches):
        batch = to_device(batch, device)
        src, src_mask, feats, kw = _model_inputs(net, batch)
        gen = net.generate(input_ids=src, attention_mask=src_mask, num_beams=beam_size, max_length=max_length, image_features=feats,
                           length_penalty=length_penalty, add_ner_ffn=True, **kw, **gkw)
        out_dict[step] = entry(batch, gen)
    net.train(was_training)
    return out_dict


# ---- self-critical sequence training (Rennie et al. 2017): loss = sum_c A_c NLL(sample_c) / tokens over captions the model sampled,
# A_c = reward_c - baseline of its group.  The weighted fused LM head (batch key / model(loss_weights=)) is the loss; everything
# here is host-side glue around generate(do_sample=True) and one teacher-forced pass.
def sequences_to_labels(seqs, pad, eos, T=None):
    """[R, L] id rows of generate(do_sample=True) — start token, tokens, eos, then pad — as (decoder_input_ids, labels), both [R, T]
    (T=None: L - 1; the caller passes max_length - 1 so the shape is the same at every step; L > T + 1 is a ValueError).
    labels[r] = seqs[r, 1:] up to and including the FIRST eos behind the start token (the start token may itself be the eos id),
    pad after it and up to T; a row without eos keeps every token.  A pad id that occurs before the eos stays where it is: it does
    not end the caption, and as the loss's ignore index that one position carries no loss.  decoder_input_ids = start token, then
    labels[:, :-1] (shift right).  Runs where `seqs` lives, host or device."""
    if seqs.dim() != 2 or seqs.shape[1] < 2:
        raise ValueError(f"sequences_to_labels: seqs must be [rows, L >= 2], got {tuple(seqs.shape)}")
    R, L = seqs.shape
    T = L - 1 if T is None else int(T)
    if L > T + 1:
        raise ValueError(f"sequences_to_labels: rows of {L} ids do not fit T + 1 = {T + 1} (T = max_length - 1)")
    labels = seqs.new_full((R, T), pad)
    labels[:, :L - 1] = seqs[:, 1:]
    is_eos = labels == eos
    behind = (is_eos.cumsum(1) - is_eos.to(torch.int64)) > 0          # strictly behind the first eos
    labels = torch.where(behind, torch.full_like(labels, pad), labels)
    dec_in = torch.cat([seqs[:, :1], labels[:, :-1]], 1)
    return dec_in.contiguous(), labels.contiguous()


def group_advantages(rewards, n, baseline="mean"):
    """fp32 [len(rewards)] advantages: every run of n consecutive rewards (the n samples of one image, generate()'s row order) minus
    the run's mean ("mean"; sums to 0 per run) or minus the mean of the run's other n - 1 rewards ("leave_one_out").  n = 1 would
    make every advantage 0 (or divide by zero): ValueError."""
    if baseline not in ("mean", "leave_one_out"):
        raise ValueError(f"group_advantages: baseline={baseline!r} is not 'mean' or 'leave_one_out'")
    if not isinstance(n, int) or n < 2:
        raise ValueError(f"group_advantages: n={n!r} samples per group: a baseline needs at least 2")
    r = torch.as_tensor(rewards, dtype=torch.float64).reshape(-1)
    if r.numel() % n != 0:
        raise ValueError(f"group_advantages: {r.numel()} rewards are not groups of n={n}")
    g = r.view(-1, n)
    s = g.sum(1, keepdim=True)
    base = s / n if baseline == "mean" else (s - g) / (n - 1)
    return (g - base).reshape(-1).to(torch.float32)


def overlap_f1_reward(samples, refs, special_ids=()):
    """clipped unigram F1 of token ids, one float per (sample, reference) pair: overlap = sum over ids of min(count in sample, count
    in reference), precision = overlap / len(sample), recall = overlap / len(reference), ids in `special_ids` (pad, eos, start)
    dropped from both first; an empty sample or reference, or no overlap, scores 0.  A stand-in that needs no tokenizer and no
    metric package (caption metrics are outside SURVEY §8): any callable (samples, refs) -> list[float] takes its place."""
    from collections import Counter
    if len(samples) != len(refs):
        raise ValueError(f"overlap_f1_reward: {len(samples)} samples but {len(refs)} references")
    special = set(int(i) for i in special_ids)
    out = []
    for s, r in zip(samples, refs):
        cs, cr = Counter(int(t) for t in s if int(t) not in special), Counter(int(t) for t in r if int(t) not in special)
        ns, nr = sum(cs.values()), sum(cr.values())
        ov = sum(min(c, cr[t]) for t, c in cs.items())
        if ns == 0 or nr == 0 or ov == 0:
            out.append(0.0)
            continue
        p, q = ov / ns, ov / nr
        out.append(2.0 * p * q / (p + q))
    return out


def check_scst_flags(scst_samples, grad_accum_steps=1, world_size=1):
    """the trainers' up-front refusals for --scst_samples N > 0: the self-critical step is one process, one batch per update."""
    if scst_samples < 0 or scst_samples == 1:
        raise ValueError(f"--scst_samples {scst_samples}: 0 (off) or at least 2 samples per image (the baseline is their mean)")
    if scst_samples and grad_accum_steps > 1:
        raise ValueError(f"--scst_samples {scst_samples} with --grad_accum_steps {grad_accum_steps}: the self-critical step does not "
                         "accumulate (DESIGN.md §8)")
    if scst_samples and world_size > 1:
        raise ValueError(f"--scst_samples {scst_samples} with world_size {world_size}: the self-critical step is one process (DESIGN.md §8)")


def self_critical_step(model, optimizer, batch, args: TrainArgs, reward_fn=overlap_f1_reward, n_samples=4, baseline="mean", ce_weight=0.0,
                       seed=None, **gen_kw):
    """One self-critical update: sample n_samples captions per image (generate(do_sample=True, num_return_sequences=n, seed=, **gen_kw)
    in eval mode, under no_grad), ONE device-to-host copy of the ids, rewards on the host (reward_fn(samples, refs) -> list[float],
    refs = the batch's caption repeated per sample; the default is overlap_f1_reward without pad / eos / start ids), advantages per
    group (group_advantages), then one teacher-forced train-mode pass over the B n sampled captions (row b n + j = sample j of image
    b, the encoder-side inputs repeat_interleave'd n times) with loss_weights = advantages, loss_norm="tokens", the text loss only —
    no CoLaM (the guide's states belong to the ground-truth caption) and no SECLA (it does not depend on the caption) — backward,
    optimizer.step with train_step's clip / guard / EMA / statistics, zero_grad.  ce_weight > 0 appends the B ground-truth
    captions as further rows of weight ce_weight: the same pass, the same weighted loss.
    Returns a device fp32 vector {loss, mean reward, mean advantage^2, mean log-prob of the sampled tokens under the train-mode
    pass} without a further sync.  Eager only, one process, one batch per update: a DistributedDataParallel wrapper or an
    optimizer built with accum_steps > 1 is a ValueError.  max_length (in gen_kw; default generate()'s) fixes T = max_length - 1."""
    if isinstance(model, DistributedDataParallel):
        raise ValueError("self_critical_step is one process: pass the bare model, not a DistributedDataParallel wrapper")
    check_scst_flags(n_samples, max(args.grad_accum_steps, getattr(optimizer, "accum_steps", 1)))
    if n_samples < 2:
        raise ValueError(f"self_critical_step: n_samples={n_samples}: at least 2 samples per image (the baseline is their mean)")
    if ce_weight < 0:
        raise ValueError(f"self_critical_step: ce_weight={ce_weight} must be >= 0")
    if args.deterministic and not ops.deterministic():
        with ops.deterministic_mode(True):
            return self_critical_step(model, optimizer, batch, args, reward_fn, n_samples, baseline, ce_weight, seed, **gen_kw)
    if args.skip_nonfinite and not getattr(optimizer, "skip_nonfinite", False):
        raise ValueError("TrainArgs.skip_nonfinite needs an optimizer built with FusedAdamW(..., skip_nonfinite=True)")
    if args.ema_decay and getattr(optimizer, "ema_decay", None) is None:
        raise ValueError("TrainArgs.ema_decay needs an optimizer built with FusedAdamW(..., ema_decay=...)")
    if args.grad_stats_every and not getattr(optimizer, "grad_stats_every", 0):
        raise ValueError("TrainArgs.grad_stats_every needs an optimizer built with FusedAdamW(..., grad_stats_every=N)")
    net, cfg, n = model, model.config, n_samples
    pad, eos, start = cfg.pad_token_id, cfg.eos_token_id, cfg.decoder_start_token_id
    max_length = gen_kw.setdefault("max_length", 20)
    T = max_length - 1
    tgt = batch["caption_ids"]
    B, dev = tgt.shape[0], tgt.device
    # ---- 1. sample, 2. one copy to the host, 3. rewards and advantages there
    net.eval()
    try:
        with torch.no_grad():
            src, src_mask, feats, kw = _model_inputs(net, batch)
            seqs = net.generate(input_ids=src, attention_mask=src_mask, image_features=feats, add_ner_ffn=True, do_sample=True,
                                num_return_sequences=n, seed=seed, **kw, **gen_kw)
    finally:
        net.train()
    seqs_host, refs_host = _ids_to_lists([seqs, tgt])
    refs = [refs_host[r // n] for r in range(B * n)]
    if reward_fn is overlap_f1_reward:
        rewards = overlap_f1_reward(seqs_host, refs, special_ids=(pad, eos, start))
    else:
        rewards = reward_fn(seqs_host, refs)
    adv = group_advantages([float(r) for r in rewards], n, baseline)
    dec_in, labels = sequences_to_labels(seqs, pad, eos, T)
    # ---- 4. / 5. rows: B n samples (b n + j), then with ce_weight > 0 the B ground-truth captions
    weights = adv
    rep = lambda t: t.repeat_interleave(n, dim=0)                                           # noqa: E731
    if ce_weight > 0:
        W = max(T, tgt.shape[1])

        def widen(t):
            return t if t.shape[1] == W else torch.cat([t, t.new_full((t.shape[0], W - t.shape[1]), pad)], 1)
        _, gt_in = K.prep_ids(tgt, pad, start_id=eos, want_mask=False)                      # shift_tokens_right as train_step does it
        dec_in, labels = torch.cat([widen(dec_in), widen(gt_in)]), torch.cat([widen(labels), widen(tgt)])
        weights = torch.cat([adv, torch.full((B,), float(ce_weight))])
        rep = lambda t: torch.cat([t.repeat_interleave(n, dim=0), t])                       # noqa: E731
    host_stats = torch.tensor([sum(rewards) / len(rewards), float((adv.double() ** 2).mean())], dtype=torch.float32)
    weights, host_stats = weights.to(dev, non_blocking=True), host_stats.to(dev, non_blocking=True)
    # ---- 6. the train-mode pass with the weighted text loss, 7. backward and the update
    ops.begin_step()
    out = net(input_ids=rep(src), attention_mask=rep(src_mask), decoder_input_ids=dec_in.contiguous(), image_features=rep(feats),
              labels=labels.contiguous(), output_logits=False, add_ner_ffn=True, output_attentions=False, loss_weights=weights.contiguous(),
              loss_norm="tokens", **{k: rep(v) for k, v in kw.items()})
    loss = out["loss"]
    with torch.autograd.set_multithreading_enabled(False):
        loss.backward(ops.const_one(loss.device))
    ops.flush_wgrads()
    streams.join_all()
    optimizer.step(clip_norm=None if args.no_clip_norm else args.clip_norm)
    optimizer.zero_grad()
    nll = out["token_nll"][:B * n]
    logp = 0.0 - nll.sum() / (labels[:B * n] != pad).sum().clamp(min=1)
    return torch.cat([loss.detach().view(1), host_stats, logp.view(1)])


def _same_loss_weights_key(who, static, batch):
    """a recorded step holds the launches of the weighted OR of the unweighted text loss: the batch must match what was recorded"""
    rec, now = static.get("loss_weights") is not None, batch.get("loss_weights") is not None
    if rec != now:
        raise ValueError(f"{who}: recorded {'with' if rec else 'without'} batch['loss_weights'], called {'with' if now else 'without'} "
                         "it (the weighted text loss is a different launch sequence: record a step of its own)")


class GraphedTrainStep:
    """The whole training step (all streams: compute, guide, weight gradients) captured once into a hipGraph and
    replayed per batch — "HIP graphs instead of a tracing compiler".  A step is ~2400 kernel launches that eager Python
    issues in ~31-37 ms; on this stack a replayed node costs about what an eager launch costs on the GPU side and the
    graph runs its parallel branches less concurrently, so replay is slower than eager multi-stream launches while the GPU
    needs ~74 ms per step: opt-in (`bench.py --graph`), kept working by tests/test_model_gpu.py.

    Capture-safety of the step: no host<->device sync inside it, LR / step counter / dropout counter live in device
    memory (lr_step kernel), every kernel is launched on torch's current stream (the capture stream or a side stream
    forked from it by an event), and all scratch comes from torch's graph-private allocator pool.
    Inputs are copied into static device buffers before each replay (a few hundred KiB of ids + the image batch).
    Not used with world_size > 1 (RCCL collectives stay outside a captured graph in round 1)."""

    def __init__(self, model, guide, optimizer, args: TrainArgs, example_batch, warmup=2):
        self.static = {k: v.clone() for k, v in example_batch.items()}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # eager warm-up on a side stream (allocator + lazy inits)
            for _ in range(warmup):
                train_step(model, guide, optimizer, self.static, args)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out4 = train_step(model, guide, optimizer, self.static, args)

    def __call__(self, batch):
        _same_loss_weights_key("GraphedTrainStep", self.static, batch)
        for k, v in self.static.items():
            v.copy_(batch[k], non_blocking=True)
        self.graph.replay()
        return self.out4


class PlannedTrainStep:
    """The whole training step — frozen towers, forward, losses, backward, AdamW; every stream — as a LAUNCH PLAN: the step's
    C-ABI call sequence (kernel launches AND the fences between streams) is recorded once by the library while one step runs
    eagerly, and every later step is ONE call, vacnic_plan_replay, which re-issues the same launches on the same streams in the
    same order from C++ (include/vacnic_hip.h "launch plans").  The GPU-side schedule is the eager multi-stream one (a hipGraph
    of the step, GraphedTrainStep, runs its branches less concurrently and is slower); the ~1250 Python -> ctypes -> autograd
    round trips per step are gone from the launch path.

    What makes a step replayable: explicit scheduling (streams: no stream synchronisation hidden inside torch), no
    host<->device sync and no ATen kernel inside the step, per-step scalars in device memory (LR, step and dropout counters:
    vacnic_lr_step), and every buffer at its recorded address — the recording runs inside a private allocator pool that is
    kept, inputs are copied into static tensors before each replay.  world_size > 1: on the reducer's native path the bucket
    all-reduces, their events and the waits before each bucket's AdamW range are C-ABI calls and hence plan commands; on the
    torch.distributed fallback they are host actions at marks of the plan (ddp.HOST_HOOK -> self.host), run unrecorded while the
    recording is paused and repeated by the host at the same points of every replay."""

    def __init__(self, model, guide, optimizer, args: TrainArgs, example_batch, warmup=2, towers=None):
        """towers: a FrozenTowerGraphs — the two frozen networks then stay hipGraph replays on their own streams, launched by the
        host before every plan replay (so they overlap the previous step's tail), and the plan is split at two marks where the
        host joins them (before the CoLaM loss) and releases their static outputs (after it)."""
        global _PLAN
        from . import _lib
        from . import ddp as _ddp
        self.towers = towers
        self.static = {k: v.clone() for k, v in example_batch.items()}
        for _ in range(warmup):                              # eager: lazy buffers, kernel loading, allocator warm-up
            train_step(model, guide, optimizer, self.static, args, None, towers)
        torch.cuda.synchronize()
        self.stream = K._stream()
        self.pool = torch.cuda.MemPool()
        self.marks = []
        self._before()                                       # (host-side work of a step: not part of the plan)
        self.handle = int(_lib.lib.vacnic_plan_begin())
        if self.handle < 0:
            _lib.check(1)
        _PLAN = self
        # world > 1: the reducer's host-side work (bucket launches on the comm stream as backward completes them, the waits before
        # each bucket's AdamW range) becomes host actions at marks of the plan — N ranks then run the SAME launch path as one
        _ddp.HOST_HOOK = self.host
        try:
            with torch.cuda.use_mem_pool(self.pool):
                self.out4 = train_step(model, guide, optimizer, self.static, args, None, towers)
        except BaseException:
            # a recording that raised leaves neither a half-recorded plan nor its private pool behind
            _PLAN = None
            _ddp.HOST_HOOK = None
            _lib.lib.vacnic_plan_end(self.handle)
            _lib.lib.vacnic_plan_destroy(self.handle)
            self.handle = None
            self.pool = None
            raise
        _PLAN = None
        _ddp.HOST_HOOK = None
        _lib.check(_lib.lib.vacnic_plan_end(self.handle))
        torch.cuda.synchronize()
        self.commands = int(_lib.lib.vacnic_plan_size(self.handle))

    def mark(self, what):
        """called by _tower_host while recording: the host acts at this point of every replay.  ('launch' is host work AHEAD of
        the plan, not a point in it: _before has done it, and does it before every replay.)"""
        from . import _lib
        if what != "launch":
            self.marks.append((int(_lib.lib.vacnic_plan_mark()), what))
            self._at(what)

    def host(self, fn):
        """recording: register `fn` as a host action at this point of the plan and run it now, unrecorded (whatever it launches
        through the C-ABI is the host's to repeat at every replay, not the plan's)."""
        from . import _lib
        self.marks.append((int(_lib.lib.vacnic_plan_mark()), fn))
        _lib.check(_lib.lib.vacnic_plan_pause(1))
        try:
            fn()
        finally:
            _lib.check(_lib.lib.vacnic_plan_pause(0))

    def _before(self, batch=None, ready=None):
        if self.towers is not None:
            _tower_host("launch", self.towers, batch if batch is not None else self.static, ready, by_plan=True)

    def _at(self, what):
        if callable(what):
            what()
        else:
            _tower_host(what, self.towers, by_plan=True)

    def __call__(self, batch, ready=None):
        """ready: optional event after which `batch` is resident in HBM (the tower graphs then start on it instead of behind the
        previous step on the compute stream, like train_step's `ready`)."""
        from . import _lib
        if K._stream() != self.stream:
            raise RuntimeError("PlannedTrainStep: replay on the stream the plan was recorded on")
        _same_loss_weights_key("PlannedTrainStep", self.static, batch)
        self._before(batch, ready)
        if ready is not None:
            torch.cuda.current_stream().wait_event(ready)
        for k, v in self.static.items():
            if batch[k] is not v:
                v.copy_(batch[k], non_blocking=True)
        pos = 0
        for idx, what in self.marks:
            _lib.call("vacnic_plan_replay", self.handle, pos, idx)
            self._at(what)
            pos = idx
        _lib.call("vacnic_plan_replay", self.handle, pos, self.commands)
        return self.out4

    def close(self):
        from . import _lib
        if self.handle is not None:
            _lib.check(_lib.lib.vacnic_plan_destroy(self.handle))
            self.handle = None


class FrozenTowerGraphs:
    """hipGraph replay for the two frozen, autograd-free, static-shape networks of the step (guide BART forward and
    CLIP ViT forward): ~430 of the step's launches become two graph launches on their side streams, which takes them off
    the Python launch path while the trainable network keeps eager multi-stream launches
    (a single whole-step graph measured slower: hipGraph runs its parallel branches less concurrently than streams do).

    Static buffers: inputs are copied in on the tower's stream right before the replay; the outputs (`gh`, `img_cls`) are
    read by the main chain only during the forward pass, so the next replay waits for the `consumed` event recorded
    after the CoLaM forward (write-after-read); the id masks the student needs are made by the step itself, on the compute stream."""

    def __init__(self, net, guide, example_batch):
        cfg = net.config
        self.net, self.guide = net, guide
        aux, vis = streams.aux_stream(), streams.vit_stream()
        if aux is None:
            raise RuntimeError("FrozenTowerGraphs needs streams.enable(True)")
        torch.cuda.synchronize()
        self.pad, self.start = cfg.pad_token_id, cfg.eos_token_id
        self.src_s = example_batch["article_ids"].clone()
        self.img_s = example_batch["img_tensor"].clone()
        self.mask_s, _ = K.prep_ids(self.src_s, self.pad)
        _, self.tgtin_s = K.prep_ids(example_batch["caption_ids"].clone(), self.pad, start_id=self.start)
        self.consumed = None
        self.ev_vit = None
        self.gh = self.g_guide = None

        def guide_body():
            return guide(input_ids=self.src_s, attention_mask=self.mask_s, decoder_input_ids=self.tgtin_s)["decoder_hidden_states"][-1]

        def vit_body():
            return extract_clip_img_feat(net.clip_model, self.img_s)[image_feature_index(cfg)]

        torch.cuda.synchronize()
        with torch.no_grad():
            with torch.cuda.stream(vis):                     # eager warm-up on the capture streams
                vit_body()
            if guide is not None:
                with torch.cuda.stream(aux):
                    guide_body()
            torch.cuda.synchronize()
            if guide is not None:
                self.g_guide = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.g_guide, stream=aux):
                    self.gh = guide_body()
            self.g_vit = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_vit, stream=vis):
                self.img_cls = vit_body()
        torch.cuda.synchronize()

    def launch(self, batch, ready=None):
        """enqueue both tower replays on their streams; the guide's id inputs are derived there, in place, from the batch."""
        aux, vis = streams.aux_stream(), streams.vit_stream()
        main = torch.cuda.current_stream()
        for s_ in (aux, vis):
            # the towers read the CALLER's batch (resident: `ready`, or ordered on the compute stream), not a plan's static copy,
            # so they need not queue behind the previous step's tail on the compute stream
            if ready is None:
                s_.wait_stream(main)
            else:
                s_.wait_event(ready)
            if self.consumed is not None:
                s_.wait_event(self.consumed)
        with torch.cuda.stream(vis):                 # the student's encoder input needs the image feature: ViT goes first
            self.img_s.copy_(batch["img_tensor"], non_blocking=True)
            self.g_vit.replay()
            self.ev_vit = torch.cuda.Event()
            self.ev_vit.record(vis)                  # (the towers may share one stream: wait for THIS, not for the stream's tail)
        if self.g_guide is not None:
            with torch.cuda.stream(aux):             # the guide's output is needed only by the CoLaM loss
                self.src_s.copy_(batch["article_ids"], non_blocking=True)
                K.prep_ids_into(self.src_s, self.mask_s, None, self.pad)
                K.prep_ids_into(batch["caption_ids"], None, self.tgtin_s, self.pad, self.start)
                self.g_guide.replay()

    def mark_consumed(self):
        self.consumed = torch.cuda.Event()
        self.consumed.record(torch.cuda.current_stream())
