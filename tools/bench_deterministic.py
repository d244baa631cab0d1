"""What the deterministic mode (ops.set_deterministic, TrainArgs.deterministic) costs, measured on the GPU.

    python tools/bench_deterministic.py [--part kernels|step|all] [--pairs N] [--steps N]

kernels: the new fixed-order kernels beside the ones they replace, at bench.py's default shapes (batch 32, 512 article / 64 caption
tokens, BART-large widths), device events around 10 launches after 3 warm-up launches, the variants alternating row by row:
  embedding backward (R = 16384 and R = 2048 rows of d = 1024, ids of the synthetic batch): atomic kernel | ordered kernel + scatter + fold
  LayerNorm backward (R = 16384, d = 1024):                                                in-call atomic fold | ordered fold
  weight gradient with bias (M = 16384 rows, 4096 x 1024 and 1024 x 1024 outputs):         GEMM with xsum | GEMM without + bias_grad_ordered
Derived beforehand from the extra traffic: the bias pass reads dY once more (M N 2 bytes), the ordered embedding backward writes and
reads R D 4 bytes of dh scratch (2 R D 4 bytes); both at the 4 TB/s these streaming kernels reach.  The ratio measured / derived is
printed beside every pair.
step: the whole training step at the same shapes on one GPU as a launch plan with the frozen towers as hipGraphs,
TrainArgs.deterministic off and on, alternating pairs of timed windows."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vacnic_amd import _lib
from vacnic_amd import kernels as K

ROWS, WARM, LAUNCHES = 5, 3, 10
HBM = 4.0e12            # bytes/s a streaming kernel of this family reaches (profiles/r2_add_ln_16384x1024.txt)
BF16 = torch.bfloat16


def timed(fn, launches=LAUNCHES, warm=WARM):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3          # us


def stats(r):
    return sum(r) / len(r), max(r) - min(r)


def in_mode(flag, fn):
    def run():
        K.DETERMINISTIC = flag
        try:
            fn()
        finally:
            K.DETERMINISTIC = False
    return run


def pair(what, off, on, extra_bytes):
    rows = {False: [], True: []}
    for _ in range(ROWS):
        rows[False].append(timed(in_mode(False, off)))
        rows[True].append(timed(in_mode(True, on)))
    (m0, s0), (m1, s1) = stats(rows[False]), stats(rows[True])
    line = f"{what}: default {m0:.1f} us (spread {s0:.1f}), deterministic {m1:.1f} us (spread {s1:.1f}), difference {m1 - m0:+.1f} us; "
    if extra_bytes:
        derived = extra_bytes / HBM * 1e6
        line += f"derived from {extra_bytes / 1e6:.1f} MB of extra traffic: {derived:.1f} us -> measured / derived = {(m1 - m0) / derived:.2f}"
    else:
        line += "no extra traffic (the same partials are read: the difference is the fold's 4 strands of a column against 32)"
    print(line)


def kernels_part():
    from vacnic_amd import synthetic
    from vacnic_amd.config import bart_large_vit_l14
    cfg, _ = bart_large_vit_l14()
    D, V = cfg.d_model, cfg.vocab_size
    print(f"== kernels, d = {D}, V = {V}; {ROWS} rows x {LAUNCHES} launches after {WARM} warm-up launches, default and deterministic alternating")
    batch = synthetic.make_batch(cfg, 32, S=512, T=64, seed=42, full_length=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    emb, gamma, beta = (rn(V, D) * 0.5).to(BF16), rn(D) * 0.3 + 1.0, rn(D) * 0.5
    demb, dg, db = torch.zeros(V, D, device="cuda"), torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    for name, key in (("encoder", "article_ids"), ("decoder", "caption_ids" if "caption_ids" in batch else "article_ids")):
        ids = batch[key].cuda()
        if name == "decoder" and key == "article_ids":
            ids = ids[:, :64].contiguous()
        B, T = ids.shape
        R = B * T
        pos = (rn(T + 2, D) * 0.5).to(BF16)
        dpos = torch.zeros(T + 2, D, device="cuda")
        dout = rn(B, T, D).to(BF16)
        _, mean, rstd = K.embed_ln_fwd(ids, emb, pos, gamma, beta, embed_scale=32.0)
        f = lambda: K.embed_ln_bwd(ids, emb, pos, dout, gamma, mean, rstd, demb, dpos, dg, db, embed_scale=32.0)
        pair(f"embedding backward, {name} (R = {R}, {ids.unique().numel()} distinct ids)", f, f, 2 * R * D * 4)
    R = 16384
    x, res, dout = rn(R, D).to(BF16), rn(R, D).to(BF16), rn(R, D).to(BF16)
    _, mean, rstd = K.add_ln_fwd(x, res, gamma, beta)
    f = lambda: K.add_ln_bwd(dout, x, res, gamma, mean, rstd, dg, db)
    pair(f"LayerNorm backward (R = {R}), fold in the call", f, f, 0)
    for N, Kd in ((4096, 1024), (1024, 1024)):
        M = 16384
        dy, xx = rn(M, N).to(BF16), rn(M, Kd).to(BF16)
        dw, dbias = torch.zeros(N, Kd, device="cuda"), torch.zeros(N, device="cuda")
        hint, split = (128, 8) if N * Kd <= (1 << 20) else (256, 4)
        gemm = lambda xs: K.gemm(dy, xx, N, Kd, M, out=dw, ldx=N, ldw=Kd, ldo=Kd, x_kstrided=True, w_kstrided=True, out_mode=2, split_k=split,
                                 xsum=xs, fixup=True, tile_hint=hint)
        pair(f"weight gradient {N} x {Kd} with bias (M = {M})", lambda: gemm(dbias), lambda: (gemm(None), K.bias_grad_ordered(dy, dbias, M, N)),
             M * N * 2)


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
    plans = {}
    args0 = TrainArgs(num_training_steps=100000)
    opt = FusedAdamW(model.arena, lr=args0.lr_bart, weight_decay=args0.weight_decay, num_warmup_steps=args0.warmup_rate * args0.num_training_steps,
                     num_training_steps=args0.num_training_steps)
    for on in (False, True):
        args = TrainArgs(num_training_steps=100000, deterministic=on)
        plans[on] = PlannedTrainStep(model, guide, opt, args, batches[0], warmup=2, towers=towers)
        out4 = plans[on](batches[1], ready)
        torch.cuda.synchronize()
        assert torch.isfinite(out4).all().item(), out4.tolist()
    print(f"\n== whole training step, one GPU, batch {B}, {S} article / {T} caption tokens, launch plan + tower graphs ({plans[True].commands} "
          f"commands deterministic, {plans[False].commands} default); {pairs} alternating pairs of windows of {steps} steps (device events)")
    rows = {False: [], True: []}
    i = 0
    for p in range(pairs):
        for on in (False, True):
            step = plans[on]
            for _ in range(2):
                step(batches[i % 4], ready); i += 1
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                out4 = step(batches[i % 4], ready); i += 1
            e1.record(); torch.cuda.synchronize()
            rows[on].append(e0.elapsed_time(e1) / steps)
        print(f"pair {p}: deterministic off {rows[False][-1]:.3f} ms/step, on {rows[True][-1]:.3f} ms/step")
    assert torch.isfinite(out4).all().item(), out4.tolist()
    (m0, s0), (m1, s1) = stats(rows[False]), stats(rows[True])
    print(f"deterministic off: mean {m0:.3f} ms/step (spread {s0:.3f});  on: mean {m1:.3f} ms/step (spread {s1:.3f});  difference {m1 - m0:+.3f} ms "
          f"= {100 * (m1 - m0) / m0:+.2f} %")
    for on in plans:
        plans[on].close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernels", "step", "all"), default="all")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deterministic.py measures on the GPU: no device found")
    print(f"tools/bench_deterministic.py on {torch.cuda.get_device_name(0)}, library version {_lib.lib.vacnic_version()}")
    if a.part in ("kernels", "all"):
        kernels_part()
        torch.cuda.empty_cache()
    if a.part in ("step", "all"):
        step_part(a.pairs, a.steps)
