"""What the per-parameter statistics (vacnic_param_stats, FusedAdamW(grad_stats_every=N)) cost, measured on the GPU.

    python tools/bench_param_stats.py [--part kernel|step|all] [--out profiles/param_stats.txt]

kernel: on an arena of bench config 2's size and layout (the BART-large VACNIC model, ~861 M parameters; the slot / unit table is
the one the optimizer would build for it), device events around 10 launches after 3 warm-up launches, the variants alternating row
by row in one process:
  a  grad_clip_coef                     the yardstick: the existing norm pass, 4 B per element read
  b  param_stats gated off              two launches whose workgroups read the gate and leave
  c  param_stats firing                 8 B per element read (g and p) + the unit table (12 B per 4096 elements)
  d  param_stats firing, p = NULL       4 B per element: the same bytes as (a), through the segmented shape
Target: c <= 2.5 x a (2 x for the bytes, 25 % for the table reads and the unaligned slot edges).
step: the whole training step at bench.py's default shapes (batch 32, 512 article / 64 caption tokens) on one GPU as a launch plan
with the frozen towers as hipGraphs, grad_stats_every 0 / 50 / 1, alternating windows of 50 steps (so that every window of the
middle variant holds exactly one firing step)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vacnic_amd import _lib
from vacnic_amd import kernels as K

ROWS, WARM, LAUNCHES = 5, 3, 10
OUT = None


def say(line=""):
    print(line, flush=True)
    if OUT is not None:
        OUT.write(line + "\n"); OUT.flush()


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


def bench_arena():
    """layout only: the bench model's arena on the meta device"""
    from vacnic_amd.config import bart_large_vit_l14
    from vacnic_amd.models.mmbart import BartForMultiModalGeneration
    cfg, _ = bart_large_vit_l14()
    with torch.device("meta"):
        net = BartForMultiModalGeneration(cfg, enc_fusion_layer=cfg.enc_fusion_layer, dim_common=cfg.dim_common, prompt_size=cfg.prompt_size)
    net.finalize("meta")
    return net.arena


def kernel_part():
    from vacnic_amd.arena import stats_table
    arena = bench_arena()
    n = arena.n
    tab = stats_table(arena).to("cuda")
    inside = sum(m for _, m in tab.slots)
    say(f"== the kernel alone: arena of {n} elements ({n / 1e6:.1f} M), {tab.nslot} slots holding {inside} of them, {tab.nunit} units; "
        f"{ROWS} rows x {LAUNCHES} launches after {WARM} warm-up launches, variants alternating row by row")
    g = torch.randn(n, device="cuda") * 1e-3
    p = torch.randn(n, device="cuda")
    out = torch.zeros(2, device="cuda"); scratch = torch.empty(1024, device="cuda")
    work = K.param_stats_workspace(tab, "cuda")
    out_f = torch.zeros(tab.nslot, 4, device="cuda"); out_i = torch.zeros(tab.nslot, 2, device="cuda", dtype=torch.int64)
    stamp = torch.zeros(4, device="cuda", dtype=torch.int64)
    hyper = torch.tensor([3e-5, 1.0], device="cuda")             # count 1: not a multiple of 1000000

    def ps(pp, hy, every):
        return lambda: K.param_stats(g, pp, n, tab, hy, every, None, 1.0, work, out_f, out_i, stamp)

    variants = [("a grad_clip_coef", lambda: K.grad_clip_coef(g, n, 0.1, 1.0, scratch, out), 4 * n),
                ("b param_stats gated off", ps(p, hyper, 1000000), 0),
                ("c param_stats firing", ps(p, None, 1), 8 * inside + 12 * tab.nunit),
                ("d param_stats firing, p = NULL", ps(None, None, 1), 4 * inside + 12 * tab.nunit)]
    rows = {name: [] for name, _, _ in variants}
    for rep in range(ROWS):
        for name, fn, _ in variants:
            fires = int(stamp[0].item())
            rows[name].append(timed(fn))
            fired = int(stamp[0].item()) - fires
            assert fired == (0 if name[0] in "ab" else WARM + LAUNCHES), (name, fired)
        say(f"row {rep}: " + "  ".join(f"{name[0]}={rows[name][-1]:.3f}" for name, _, _ in variants) + " ms")
    say()
    mean = {}
    for name, _, nbytes in variants:
        mean[name[0]], spread = stats(rows[name])
        rate = f", {nbytes / mean[name[0]] / 1e9:.2f} TB/s over {nbytes / 1e9:.2f} GB" if nbytes else ""
        say(f"{name}: mean {mean[name[0]]:.3f} ms, spread {spread:.3f} ms{rate}")
    total = float(out_f[:, 0].double().sum().sqrt())
    say(f"total gradient norm from the slot sums {total:.6g}, from grad_clip_coef {out[1].item():.6g} (the arena outside the slots holds "
        f"{n - inside} random elements the clip pass also reads)")
    ratio = mean["c"] / mean["a"]
    say(f"\nfiring against the clip pass: c / a = {ratio:.2f} (target <= 2.5): {'met' if ratio <= 2.5 else 'MISSED'};  "
        f"d / a = {mean['d'] / mean['a']:.2f} at the same bytes;  gated off: b = {mean['b'] * 1e3:.1f} us per step")
    return ratio


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
    every = (0, 50, 1)
    plans, opts = {}, {}
    # the optimizers share the arena and its moments (the last constructor's), each has its own step count; all are built before
    # anything is recorded, because a plan replays the addresses it recorded
    for ev in every:
        args = TrainArgs(num_training_steps=100000, grad_stats_every=ev)
        opts[ev] = (FusedAdamW(model.arena, lr=args.lr_bart, weight_decay=args.weight_decay,
                               num_warmup_steps=args.warmup_rate * args.num_training_steps,
                               num_training_steps=args.num_training_steps, grad_stats_every=ev), args)
    for ev in every:
        opt, args = opts[ev]
        plans[ev] = PlannedTrainStep(model, guide, opt, args, batches[0], warmup=2, towers=towers)
        out4 = plans[ev](batches[1], ready)
        torch.cuda.synchronize()
        assert torch.isfinite(out4).all().item(), out4.tolist()
    say(f"\n== whole training step, one GPU, batch {B}, {S} article / {T} caption tokens, launch plan + tower graphs (commands per plan: "
        + ", ".join(f"every {ev}: {plans[ev].commands}" for ev in every) + f"); {pairs} alternating rounds of windows of {steps} steps (device events)")
    rows = {ev: [] for ev in every}
    i = 0
    for pair in range(pairs):
        for ev in every:
            step = plans[ev]
            for _ in range(2):
                step(batches[i % 4], ready); i += 1
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                out4 = step(batches[i % 4], ready); i += 1
            e1.record(); torch.cuda.synchronize()
            rows[ev].append(e0.elapsed_time(e1) / steps)
        say(f"round {pair}: " + "  ".join(f"every {ev}: {rows[ev][-1]:.3f} ms/step" for ev in every))
    assert torch.isfinite(out4).all().item(), out4.tolist()
    base, base_spread = stats(rows[0])
    for ev in every:
        m, s = stats(rows[ev])
        fires = opts[ev][0].grad_stats(model.named_parameters())["fires"] if ev else 0
        say(f"grad_stats_every {ev}: mean {m:.3f} ms/step (spread {s:.3f}), {m - base:+.3f} ms = {100 * (m - base) / base:+.2f} % against off "
            f"(spread of the off rows {base_spread:.3f} ms); records taken {fires}")
    rep = opts[50][0].grad_stats(model.named_parameters())
    worst = max(rep["params"].items(), key=lambda kv: kv[1]["grad_norm"])
    say(f"last record of every 50: step {rep['step']}, total gradient norm {rep['total_grad_norm']:.4g}, {len(rep['params'])} parameters, "
        f"largest gradient norm in {worst[0]} ({worst[1]['grad_norm']:.4g})")
    say("multi-GPU cost (the bucket-wise AdamW overlap is not used while the option is on): NOT measured, this is a one-GPU run")
    for ev in plans:
        plans[ev].close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernel", "step", "all"), default="all")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default="", help="also append the report to this file (profiles/param_stats.txt)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_param_stats.py measures on the GPU: no device found")
    if a.out:
        OUT = open(a.out, "a")
    say(f"tools/bench_param_stats.py on {torch.cuda.get_device_name(0)}, library version {_lib.lib.vacnic_version()}")
    if a.part in ("kernel", "all"):
        kernel_part()
        torch.cuda.empty_cache()
    if a.part in ("step", "all"):
        step_part(a.pairs, a.steps)
