"""What the non-finite gradient guard (vacnic_grad_guard, FusedAdamW(skip_nonfinite=True)) costs, measured on the GPU.

    python tools/bench_grad_guard.py [--parent-lib DIR/libvacnic_hip.so] [--part optimizer|step|all]

optimizer: the optimizer phase alone on an arena of bench config 2's size (the BART-large VACNIC model, ~861.3 M parameters, rounded
as the arena rounds), device events around 10 launches after 3 warm-up launches, the variants alternating row by row in one process:
  1  lr_step + adamw                                  (the present phase)
  2  lr_step + grad_guard + adamw(skip)               (guard on, clipping off)
  3  lr_step + grad_clip_coef + adamw(clip)           (the present clipped phase)
  4  lr_step + grad_guard + adamw(clip, skip)         (guard on, clipping on)
  5  phase 2 with one NaN planted before every step   (a skipped step: norm pass + zeroing of g)
--parent-lib: the library built from the parent commit (no `skip` field in its argument structs), loaded beside this tree's:
phases 1 and 3 through it alternate with the same phases through this tree's library ("off costs nothing": the difference of the
means against the spread of the parent's own rows).
step: the whole training step at bench.py's default shapes (batch 32, 512 article / 64 caption tokens) on one GPU as a launch plan
with the frozen towers as hipGraphs, TrainArgs.skip_nonfinite off and on, alternating pairs of timed windows.
Yardstick for the guard's extra pass: it reads 4 B/param beside AdamW's 30 B/param (+ 4 B/param of gradient zeroing)."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vacnic_amd import _lib
from vacnic_amd import kernels as K

ROWS, WARM, LAUNCHES = 5, 3, 10


def timed(fn, launches=LAUNCHES, warm=WARM):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def stats(r):
    return sum(r) / len(r), max(r) - min(r)


class ParentLib:
    """the parent commit's library through its own argument layout (vacnic_adamw_args without the trailing `skip`)."""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
        self.Args = type("parent_adamw_args", (C.Structure,), {"_fields_": [
            ("p", vp), ("g", vp), ("m", vp), ("v", vp), ("p_bf16", vp), ("hyper", vp), ("n", i64), ("beta1", f32), ("beta2", f32),
            ("eps", f32), ("weight_decay", f32), ("grad_scale", f32), ("zero_grad", i32), ("clip_coef", vp)]})
        self.lib.vacnic_adamw.argtypes = [C.POINTER(self.Args), vp]
        self.lib.vacnic_lr_step.argtypes = [vp, f32, f32, f32, vp, vp]
        self.lib.vacnic_grad_clip_coef.argtypes = [vp, i64, f32, f32, vp, vp, vp]

    def phase(self, p, g, m, v, p16, hyper, n, clip, scratch, out):
        s = K._stream()
        rc = self.lib.vacnic_lr_step(hyper.data_ptr(), 3e-5, 0.0, 1e9, None, s)
        if clip:
            rc |= self.lib.vacnic_grad_clip_coef(g.data_ptr(), n, 1.0, 0.1, scratch.data_ptr(), out.data_ptr(), s)
        a = self.Args(p=p.data_ptr(), g=g.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), p_bf16=p16.data_ptr(), hyper=hyper.data_ptr(), n=n,
                      beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0, zero_grad=1,
                      clip_coef=out.data_ptr() if clip else None)
        rc |= self.lib.vacnic_adamw(C.byref(a), s)
        if rc != 0:
            raise RuntimeError("parent library call failed")


def arena_size():
    from vacnic_amd.config import bart_large_vit_l14
    from vacnic_amd.models.mmbart import BartForMultiModalGeneration
    cfg, _ = bart_large_vit_l14()
    with torch.device("meta"):                 # layout only
        net = BartForMultiModalGeneration(cfg, enc_fusion_layer=cfg.enc_fusion_layer, dim_common=cfg.dim_common, prompt_size=cfg.prompt_size)
    net.finalize("meta")
    return net.arena.n


def optimizer_part(parent_path):
    n = arena_size()
    print(f"== optimizer phase alone, arena of {n} elements ({n / 1e6:.1f} M), {ROWS} rows x {LAUNCHES} launches after {WARM} warm-up launches, "
          f"variants alternating row by row")
    p = torch.randn(n, device="cuda"); g = torch.randn(n, device="cuda") * 1e-3
    m = torch.zeros(n, device="cuda"); v = torch.zeros(n, device="cuda"); p16 = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    hyper = torch.tensor([3e-5, 1.0], device="cuda")
    out = torch.zeros(2, device="cuda"); scratch = torch.empty(1024, device="cuda"); idx = torch.empty(1024, device="cuda", dtype=torch.int64)
    state = K.guard_state("cuda")
    nan = torch.full((1,), float("nan"), device="cuda")
    where = n // 3

    def phase(guard, clip, poison=False):
        def fn():
            if poison:
                g[where:where + 1].copy_(nan)                  # (one 4-byte copy kernel inside the timed window)
            K.lr_step(hyper, 3e-5, 0.0, 1e9)
            c = None
            if guard:
                K.grad_guard(g, n, hyper, state, 0.1 if clip else 0.0, None, 1.0, scratch, idx, out)
                c = out if clip else None
            elif clip:
                c = K.grad_clip_coef(g, n, 0.1, 1.0, scratch, out)
            K.adamw(p, g, m, v, p16, hyper, n, zero_grad=True, clip_coef=c, skip=state if guard else None)
        return fn

    variants = [("1 lr_step + adamw", phase(False, False)),
                ("2 lr_step + grad_guard + adamw(skip)", phase(True, False)),
                ("3 lr_step + grad_clip_coef + adamw(clip)", phase(False, True)),
                ("4 lr_step + grad_guard + adamw(clip, skip)", phase(True, True)),
                ("5 skipped step (one NaN planted): lr_step + grad_guard + adamw(skip)", phase(True, False, poison=True)),
                ("  grad_guard alone", lambda: K.grad_guard(g, n, hyper, state, 0.1, None, 1.0, scratch, idx, out)),
                ("  grad_clip_coef alone", lambda: K.grad_clip_coef(g, n, 0.1, 1.0, scratch, out))]
    if parent_path:
        par = ParentLib(parent_path)
        variants += [("P1 parent library: lr_step + adamw", lambda: par.phase(p, g, m, v, p16, hyper, n, False, scratch, out)),
                     ("P3 parent library: lr_step + grad_clip_coef + adamw(clip)", lambda: par.phase(p, g, m, v, p16, hyper, n, True, scratch, out))]
    rows = {name: [] for name, _ in variants}
    for rep in range(ROWS):
        for name, fn in variants:
            state.copy_(torch.tensor([0, 0, 0, -1]))
            rows[name].append(timed(fn))
            if name.startswith("5"):
                assert state[1].item() == WARM + LAUNCHES, "every step of the poisoned variant was skipped"
                assert torch.isfinite(p[where]).item()
            elif name[0] in "24":
                assert state[1].item() == 0
        print(f"row {rep}: " + "  ".join(f"{name.split()[0]}={rows[name][-1]:.3f}" for name, _ in variants if name.strip()[0] != "g") + " ms")
    print()
    for name, _ in variants:
        mean, spread = stats(rows[name])
        print(f"{name}: mean {mean:.3f} ms, spread {spread:.3f} ms (rows {', '.join(f'{x:.3f}' for x in rows[name])})")
    names = [nm for nm, _ in variants]
    mean = lambda k: stats(rows[names[k]])[0]
    derived = n * 4 / 6.2e12 * 1e3
    print(f"\nguard on, clipping off:  phase 2 - phase 1 = {mean(1) - mean(0):+.3f} ms  (derived from bytes: 4 B/param at the 6.2 TB/s of "
          f"profiles/r1_adamw_microbench.txt = {derived:.3f} ms; the pass alone: {mean(5):.3f} ms = {n * 4 / mean(5) / 1e9:.2f} TB/s)")
    print(f"guard on, clipping on:   phase 4 - phase 3 = {mean(3) - mean(2):+.3f} ms  (the guard's norm pass replaces the clip's: "
          f"alone {mean(5):.3f} ms against {mean(6):.3f} ms)")
    print(f"a skipped step:          phase 5 = {mean(4):.3f} ms  (reads 4 B/param, writes 4 B/param of zeros)")
    if parent_path:
        for new, old, what in ((0, 7, "lr_step + adamw, skip = NULL"), (2, 8, "clipped phase, skip = NULL")):
            (mn, sn), (mo, so) = stats(rows[names[new]]), stats(rows[names[old]])
            print(f"off costs nothing? {what}: this tree {mn:.3f} ms (spread {sn:.3f}) against the parent library {mo:.3f} ms (spread of the "
                  f"parent's own rows {so:.3f}): difference {mn - mo:+.3f} ms -> {'within' if abs(mn - mo) <= so else 'OUTSIDE'} the parent's spread")


def step_part(pairs, steps):
    from vacnic_amd import streams, synthetic
    from vacnic_amd.config import bart_large_vit_l14
    from vacnic_amd.training import FrozenTowerGraphs, FusedAdamW, PlannedTrainStep, TrainArgs, build_models, to_device
    streams.enable(True)
    cfg, vcfg = bart_large_vit_l14()
    B, S, T = 32, 512, 64
    with torch.device("cuda"):
        model, guide, _ = build_models(cfg, vcfg, device="cuda", seed=1234, init="device")
    torch.cuda.empty_cache()
    batches = [to_device(synthetic.make_batch(cfg, B, S=S, T=T, seed=42, step=i, full_length=True), "cuda") for i in range(4)]
    torch.cuda.synchronize()
    ready = torch.cuda.Event(); ready.record()
    towers = FrozenTowerGraphs(model, guide, batches[0])
    plans, opts = {}, {}
    # two optimizers over the one arena, both built before anything is recorded: the second constructor replaces the arena's
    # moments, and a plan replays the addresses it recorded — they share the moments, each has its own step count
    for on in (False, True):
        args = TrainArgs(num_training_steps=100000, skip_nonfinite=on)
        opts[on] = (FusedAdamW(model.arena, lr=args.lr_bart, weight_decay=args.weight_decay,
                               num_warmup_steps=args.warmup_rate * args.num_training_steps,
                               num_training_steps=args.num_training_steps, skip_nonfinite=on), args)
    for on in (False, True):
        opt, args = opts[on]
        plans[on] = (PlannedTrainStep(model, guide, opt, args, batches[0], warmup=2, towers=towers), opt)
        out4 = plans[on][0](batches[1], ready)
        torch.cuda.synchronize()
        assert torch.isfinite(out4).all().item(), out4.tolist()
    print(f"\n== whole training step, one GPU, batch {B}, {S} article / {T} caption tokens, launch plan + tower graphs ({plans[True][0].commands} "
          f"commands with the guard, {plans[False][0].commands} without); {pairs} alternating pairs of windows of {steps} steps (device events)")
    rows = {False: [], True: []}
    i = 0
    for pair in range(pairs):
        for on in (False, True):
            step = plans[on][0]
            for _ in range(2):
                step(batches[i % 4], ready); i += 1
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                out4 = step(batches[i % 4], ready); i += 1
            e1.record(); torch.cuda.synchronize()
            rows[on].append(e0.elapsed_time(e1) / steps)
        print(f"pair {pair}: skip_nonfinite off {rows[False][-1]:.3f} ms/step, on {rows[True][-1]:.3f} ms/step")
    rep = plans[True][1].guard_report(model.named_parameters())
    assert rep["skipped"] == 0 and torch.isfinite(out4).all().item(), (rep, out4.tolist())
    (m0, s0), (m1, s1) = stats(rows[False]), stats(rows[True])
    print(f"skip_nonfinite off: mean {m0:.3f} ms/step (spread {s0:.3f});  on: mean {m1:.3f} ms/step (spread {s1:.3f});  difference {m1 - m0:+.3f} ms "
          f"= {100 * (m1 - m0) / m0:+.2f} %;  no step was skipped, grad norm of the last step {plans[True][1].clip[1].item():.4g}")
    print("multi-GPU cost (the bucket-wise AdamW overlap is not used while the guard is on): NOT measured, this is a one-GPU run")
    for on in plans:
        plans[on][0].close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="libvacnic_hip.so built from the parent commit")
    ap.add_argument("--part", choices=("optimizer", "step", "all"), default="all")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_guard.py measures on the GPU: no device found")
    print(f"tools/bench_grad_guard.py on {torch.cuda.get_device_name(0)}, library version {_lib.lib.vacnic_version()}")
    if a.part in ("optimizer", "all"):
        optimizer_part(a.parent_lib)
        torch.cuda.empty_cache()
    if a.part in ("step", "all"):
        step_part(a.pairs, a.steps)
