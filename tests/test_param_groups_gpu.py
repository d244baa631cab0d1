"""AdamW parameter groups on the MI355X: the grouped update and clip-norm kernels against torch.optim.AdamW(param_groups) +
LambdaLR and against the ungrouped kernels (bit for bit where the groups say the same), range-wise steps, and the optimizer,
launch plan and checkpoint at model level.  Tolerances against torch are those of test_adamw_and_schedule for the same comparison:
rtol 1e-5 / atol 1e-7 on fp32 parameters after 8 steps, 4e-3 / 1e-6 for the bf16 shadow."""
import io
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 4104
# a 1-element segment, three segments inside one 4-vector, boundaries off the vector grid, boundaries on the 1024-element
# workgroup tile, a short tail
BOUNDS = [0, 1, 3, 4, 6, 1024, 1027, 2048, 4100, 4104]
GROUPS = [(1.0, 0.01, False), (10.0, 0.0, False), (1.0, 0.0, True), (0.1, 0.1, False)]        # (lr_scale, weight_decay, frozen)
LR, WARM, TOTAL = 3e-5, 5.0, 100.0


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


def rnd(*shape, scale=1.0, dtype=torch.bfloat16, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to("cuda").to(dtype)


def close(a, b, rtol, atol, what=""):
    a = a.float(); b = b.float()
    err = (a - b).abs()
    bound = atol + rtol * b.abs()
    bad = (err > bound).sum().item()
    assert bad == 0, f"{what}: {bad}/{a.numel()} off; max err {err.max().item():.4g} (ref max {b.abs().max().item():.4g})"


def small_cfg(**kw):
    from vacnic_amd.config import VacnicConfig
    base = dict(d_model=768, encoder_layers=1, decoder_layers=1, encoder_attention_heads=12, decoder_attention_heads=12,
                encoder_ffn_dim=3072, decoder_ffn_dim=3072, enc_fusion_layer=[0], dim_common=768, clip_width=768, dropout=0.0)
    base.update(kw)
    return VacnicConfig(**base)


def _vcfg():
    from vacnic_amd.config import ClipVisionConfig
    return ClipVisionConfig(width=768, layers=1, patch_size=16, image_size=32, output_dim=64)


def segments(bounds=BOUNDS, thaw=False):
    """[(start, end, lr_scale, wd, frozen)] cycling through GROUPS; thaw: the frozen group trains instead (at {1, 0})."""
    return [(bounds[i], bounds[i + 1], *GROUPS[i % 4][:2], GROUPS[i % 4][2] and not thaw) for i in range(len(bounds) - 1)]


def table(segs, n):
    from vacnic_amd.arena import table_from_segments
    t = table_from_segments(n, [(s, lr, wd, fr) for s, _, lr, wd, fr in segs]).to("cuda")
    assert t.nseg == len(segs), "adjacent test segments differ, nothing merges"
    return t


def state(n=N, marks=True):
    """p, g, m, v, shadow, hyper; marks: the moments of frozen segments and the whole shadow start from values no update produces."""
    p = rnd(n, dtype=torch.float32, seed=1); g = rnd(n, dtype=torch.float32, seed=2)
    m = torch.zeros(n, device="cuda"); v = torch.zeros(n, device="cuda")
    p16 = torch.full((n,), 7.0 if marks else 0.0, device="cuda", dtype=torch.bfloat16)
    if marks:
        for s, e, _, _, fr in segments():
            if fr:
                m[s:e] = 0.25; v[s:e] = 0.5
    return p, g, m, v, p16, torch.zeros(2, device="cuda")


# ------------------------------------------------------------------------------------------------------ 1: against torch
def test_grouped_adamw_matches_torch_param_groups(K):
    segs = segments()
    tab = table(segs, N)
    p, g, m, v, p16, hyper = state()
    p0, m0, v0, s0 = p.clone(), m.clone(), v.clone(), p16.clone()
    live = [(s, e, lr, wd) for s, e, lr, wd, fr in segs if not fr]
    ref = [torch.nn.Parameter(p[s:e].clone()) for s, e, _, _ in live]
    opt = torch.optim.AdamW([{"params": [q], "lr": LR * lr, "weight_decay": wd} for q, (_, _, lr, wd) in zip(ref, live)],
                            lr=LR, betas=(0.9, 0.999), eps=1e-8)
    lam = lambda k: k / max(1.0, WARM) if k < WARM else max(0.0, (TOTAL - k) / max(1.0, TOTAL - WARM))
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    for step in range(8):
        gg = g * (1.0 + 0.1 * step)
        for q, (s, e, _, _) in zip(ref, live):
            q.grad = gg[s:e].clone()
        opt.step(); sched.step()
        gbuf = gg.clone()
        K.lr_step(hyper, LR, WARM, TOTAL)
        K.adamw_groups(p, gbuf, m, v, p16, hyper, N, tab)
        assert (gbuf == 0).all(), "g is zeroed everywhere, frozen segments included"
    for q, (s, e, lr, wd) in zip(ref, live):
        close(p[s:e], q.data, 1e-5, 1e-7, f"params of segment [{s}, {e}) lr_scale {lr} wd {wd} after 8 steps")
        close(p16[s:e], p[s:e], 4e-3, 1e-6, f"bf16 shadow of segment [{s}, {e})")
        assert (m[s:e] != 0).all() and (v[s:e] != 0).all()
    moved = 0
    for s, e, _, _, fr in segs:
        if fr:
            for got, want, what in ((p, p0, "p"), (m, m0, "m"), (v, v0, "v"), (p16, s0, "shadow")):
                assert torch.equal(got[s:e], want[s:e]), f"frozen [{s}, {e}): {what} was written"
        else:
            moved += int((p[s:e] != p0[s:e]).sum())
    assert moved > 0.99 * sum(e - s for s, e, _, _ in live)
    assert hyper[1].item() == 8.0


# ------------------------------------------------------------------------------- 2: bit-identity with the existing kernel
def _same(a, b, what):
    for x, y, nm in zip(a, b, ("p", "m", "v", "shadow", "g")):
        assert torch.equal(x, y), f"{what}: {nm} differs from the ungrouped kernel in {(x != y).sum().item()} elements"


def test_one_segment_is_the_ungrouped_kernel_bit_for_bit(K):
    wd = 0.01
    tab = table([(0, N, 1.0, wd, False)], N)
    A, B = state(marks=False), state(marks=False)
    for step in range(3):
        for (p, g, m, v, p16, hyper), grouped in ((A, False), (B, True)):
            g.copy_(rnd(N, dtype=torch.float32, seed=2) * (1.0 + 0.1 * step))
            K.lr_step(hyper, LR, WARM, TOTAL)
            if grouped:
                K.adamw_groups(p, g, m, v, p16, hyper, N, tab)
            else:
                K.adamw(p, g, m, v, p16, hyper, N, weight_decay=wd)
        _same([A[i] for i in (0, 2, 3, 4, 1)], [B[i] for i in (0, 2, 3, 4, 1)], f"step {step}")
    assert (A[0] != rnd(N, dtype=torch.float32, seed=1)).any()


def _two_segment_case(K, n, split, steps):
    tab = table([(0, split, 1.0, 0.01, False), (split, n, 1.0, 0.0, False)], n)
    gen = torch.Generator(device="cuda").manual_seed(11)
    p = torch.randn(n, device="cuda", generator=gen); g0 = torch.randn(n, device="cuda", generator=gen)
    A = [p, g0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda", dtype=torch.bfloat16)]
    B = [t.clone() for t in A]
    hyper = torch.zeros(2, device="cuda")
    for step in range(steps):
        K.lr_step(hyper, LR, 0.0, TOTAL)
        if step:
            A[1].copy_(g0); B[1].copy_(g0)
        for lo, hi, wd in ((0, split, 0.01), (split, n, 0.0)):
            K.adamw(A[0][lo:hi], A[1][lo:hi], A[2][lo:hi], A[3][lo:hi], A[4][lo:hi], hyper, hi - lo, weight_decay=wd)
        K.adamw_groups(*B, hyper, n, tab)
        _same([A[i] for i in (0, 2, 3, 4, 1)], [B[i] for i in (0, 2, 3, 4, 1)], f"n={n} step {step}")
    assert (B[0][split:] != 0).all() and (B[1] == 0).all()
    return A, B


def test_two_segments_are_two_ungrouped_calls_bit_for_bit(K):
    _two_segment_case(K, N, 2052, steps=3)


def test_two_segments_beyond_2_pow_26_elements(K):
    """the grid-stride path (more 4-vectors than the 65536 x 256 threads of the launch) and 64-bit element offsets."""
    n = 65536 * 1024 + 4104
    split = (1 << 26) + 2052
    assert n // 4 > 65536 * 256 and split < n
    _two_segment_case(K, n, split, steps=1)
    torch.cuda.empty_cache()


# -------------------------------------------------------------------------------------------------------- 3: range steps
def test_range_steps_equal_one_whole_arena_step(K):
    """FusedAdamW.step_range as the data-parallel reducer calls it: slices of the arena with elem_base = the slice's offset.  The
    first two ranges end inside a segment."""
    tab = table(segments(), N)
    whole, parts = state(), state()
    for hyper in (whole[5], parts[5]):
        K.lr_step(hyper, LR, 0.0, TOTAL); K.lr_step(hyper, LR, 0.0, TOTAL)
    p, g, m, v, p16, hyper = whole
    K.adamw_groups(p, g, m, v, p16, hyper, N, tab)
    p, g, m, v, p16, hyper = parts
    for lo, hi in ((2052, 4104), (0, 1028), (1028, 2052)):               # (any order: the reducer steps buckets as they arrive)
        K.adamw_groups(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], p16[lo:hi], hyper, hi - lo, tab, elem_base=lo)
    _same([whole[i] for i in (0, 2, 3, 4, 1)], [parts[i] for i in (0, 2, 3, 4, 1)], "range-wise")
    assert (whole[0] != rnd(N, dtype=torch.float32, seed=1)).sum() > 3000


# ---------------------------------------------------------------------------------------------------- 4: grouped clip-norm
N_CLIP = 1024 * 1100 + 4104                                                # more 4-vectors than the norm pass has threads
BOUNDS_CLIP = BOUNDS[:-1] + [500001, N_CLIP]


@pytest.mark.parametrize("max_norm,world", [(0.1, 1), (1e4, 1), (0.1, 4), (1e4, 4)])
def test_grouped_clip_norm_matches_torch_over_the_trained_segments(K, max_norm, world):
    segs = segments(BOUNDS_CLIP)
    assert N_CLIP // 4 > 1024 * 256 and sum(fr for *_, fr in segs) == 2
    tab = table(segs, N_CLIP)
    g = rnd(N_CLIP, dtype=torch.float32, seed=2) * 3.0
    for s, e, _, _, fr in segs:
        if fr:
            g[s:e] *= 100.0                                                 # a frozen gradient that would dominate the norm
    g0 = g.clone()
    ref = [torch.nn.Parameter(torch.zeros(e - s, device="cuda")) for s, e, _, _, fr in segs if not fr]
    for q, (s, e) in zip(ref, [(s, e) for s, e, _, _, fr in segs if not fr]):
        q.grad = g[s:e].clone() / world
    ref_norm = torch.nn.utils.clip_grad_norm_(ref, max_norm).item()
    out = K.grad_clip_coef_groups(g, N_CLIP, max_norm, tab, grad_scale=1.0 / world)
    out2 = K.grad_clip_coef_groups(g, N_CLIP, max_norm, tab, grad_scale=1.0 / world)
    assert torch.equal(out, out2), "the norm must be bit-reproducible"
    assert torch.equal(g, g0), "the gradient arena is not rewritten by the norm pass"
    everything = (g0 / world).double().norm().item()
    print(f"norm {out[1].item():.6f} torch {ref_norm:.6f} (frozen included: {everything:.3f}) coef {out[0].item():.6g}")
    assert everything > 2 * ref_norm
    assert abs(out[1].item() - ref_norm) <= 1e-5 * ref_norm
    want = min(1.0, max_norm / (ref_norm + 1e-6))
    assert abs(out[0].item() - want) <= 1e-5 * want
    # nothing frozen: the ungrouped entry, bit for bit
    thawed = table(segments(BOUNDS_CLIP, thaw=True), N_CLIP)
    assert torch.equal(K.grad_clip_coef_groups(g, N_CLIP, max_norm, thawed, grad_scale=1.0 / world),
                       K.grad_clip_coef(g, N_CLIP, max_norm, grad_scale=1.0 / world))


def test_clip_coefficient_feeds_the_grouped_update(K):
    """clip_grad_norm_ + AdamW(param_groups) in torch against coefficient-on-device + grouped update, one step."""
    segs = segments()
    tab = table(segs, N)
    p, g, m, v, p16, hyper = state()
    g *= 3.0
    live = [(s, e, lr, wd) for s, e, lr, wd, fr in segs if not fr]
    ref = [torch.nn.Parameter(p[s:e].clone()) for s, e, _, _ in live]
    opt = torch.optim.AdamW([{"params": [q], "lr": LR * lr, "weight_decay": wd} for q, (_, _, lr, wd) in zip(ref, live)],
                            lr=LR, betas=(0.9, 0.999), eps=1e-8)
    for q, (s, e, _, _) in zip(ref, live):
        q.grad = g[s:e].clone()
    torch.nn.utils.clip_grad_norm_(ref, 0.1)
    opt.step()
    K.lr_step(hyper, LR, 0.0, 1e9)
    out = K.grad_clip_coef_groups(g, N, 0.1, tab)
    assert out[0].item() < 0.01
    K.adamw_groups(p, g, m, v, p16, hyper, N, tab, clip_coef=out)
    for q, (s, e, _, _) in zip(ref, live):
        close(p[s:e], q.data, 1e-5, 1e-7, f"clipped grouped update of [{s}, {e})")
        # m = 0.1 * coef * g: the coefficient's own 1e-5 bound plus fp32 rounding
        close(m[s:e], opt.state[q]["exp_avg"], 2e-5, 0.0, f"first moment of [{s}, {e})")


# ------------------------------------------------------------------------------------------------------- 5: model level
def model_spec(model):
    from vacnic_amd.arena import no_decay_spec
    return [{"match": r"^model\.shared\.", "frozen": True}, {"match": "prompt_mlp|visual_map", "lr_scale": 10.0}] + no_decay_spec(model)


def _grouped_opt(model, args, **kw):
    from vacnic_amd.training import FusedAdamW
    return FusedAdamW(model.arena, lr=args.lr_bart, weight_decay=args.weight_decay, param_groups=model_spec(model),
                      named_parameters=model.named_parameters(), **kw)


def test_model_step_matches_torch_param_groups():
    from vacnic_amd import ops, streams, synthetic
    from vacnic_amd.arena import resolve_spec
    from vacnic_amd.training import TrainArgs, build_models, forward_losses, to_device
    cfg = small_cfg()
    args = TrainArgs(num_training_steps=20, lr_bart=1e-4)
    streams.enable(False)
    ops.Rng.manual_seed(3); ops.Rng.device_counter().zero_()
    model, guide, _ = build_models(cfg, _vcfg(), init="synthetic", seed=0)
    model.train()
    a = model.arena
    opt = _grouped_opt(model, args, num_warmup_steps=0, num_training_steps=20)        # no warm-up: the first step's lr is lr_bart
    batch = to_device(synthetic.make_batch(cfg, 3, S=32, T=12, F=3, seed=40, image_size=32), "cuda")
    ops.begin_step()
    total, _, _ = forward_losses(model, guide, batch, args)
    with torch.autograd.set_multithreading_enabled(False):
        total.backward(ops.const_one(total.device))
    ops.flush_wgrads()
    streams.join_all()
    torch.cuda.synchronize()
    grad = a.grad.clone()
    snap = [t.clone() for t in (a.flat32, a.exp_avg, a.exp_avg_sq, a.flat16, opt.hyper)]

    def restore():
        for t, s_ in zip((a.flat32, a.exp_avg, a.exp_avg_sq, a.flat16, opt.hyper), snap):
            t.copy_(s_)
        a.grad.copy_(grad)

    named = [(nm, p) for nm, p in model.named_parameters() if id(p) in a.slots]
    vals = resolve_spec([nm for nm, _ in named], opt.param_groups, args.weight_decay)
    assert vals["model.shared.weight"] == (1.0, 0.01, True)
    assert sorted({v for v in vals.values()}) == [(1.0, 0.0, False), (1.0, 0.01, False), (1.0, 0.01, True), (10.0, 0.0, False), (10.0, 0.01, False)]
    ref, where = [], []
    for nm, p in named:
        lr, wd, fr = vals[nm]
        if not fr:
            o, n, _ = a.slots[id(p)]
            q = torch.nn.Parameter(snap[0][o:o + n].clone())
            q.grad = grad[o:o + n].clone()
            ref.append({"params": [q], "lr": args.lr_bart * lr, "weight_decay": wd}); where.append((o, n))
    topt = torch.optim.AdamW(ref, lr=args.lr_bart, betas=(0.9, 0.999), eps=1e-8)
    topt.step()
    want = snap[0].clone()
    for grp, (o, n) in zip(ref, where):
        want[o:o + n] = grp["params"][0].data

    opt.step()
    torch.cuda.synchronize()
    close(a.flat32, want, 1e-5, 1e-7, "every parameter after one grouped step")
    close(a.flat16, a.flat32, 4e-3, 1e-6, "bf16 shadow")
    assert (a.grad == 0).all(), "the gradient arena is zeroed, the frozen embedding's included"
    emb = model.model.shared.weight
    o, n, cap = a.slots[id(emb)]
    assert grad[o:o + n].abs().max() > 0, "backward still computes the frozen embedding's gradient"
    for got, was, what in zip((a.flat32, a.exp_avg, a.exp_avg_sq, a.flat16), snap, ("p", "m", "v", "shadow")):
        assert torch.equal(got[o:o + cap], was[o:o + cap]), f"frozen embedding: {what} was written"
    covered = torch.zeros(a.n, dtype=torch.bool, device="cuda")
    for so, sn, _ in a.slots.values():
        covered[so:so + sn] = True
    assert cap > n and not covered[o + n:o + cap].any()
    for t, what in ((a.flat32, "p"), (a.exp_avg, "m"), (a.exp_avg_sq, "v"), (a.flat16, "shadow")):
        assert (t[~covered] == 0).all(), f"padding rows and alignment gaps must stay exactly zero: {what}"
    moved = (a.flat32 != snap[0])[covered].float().mean().item()
    expect = 1.0 - n / covered.sum().item()              # the embedding stays, everything else moves
    assert 0.05 < n / covered.sum().item() < 0.95 and abs(moved - expect) < 0.01, (moved, expect)
    stepped = [t.clone() for t in (a.flat32, a.exp_avg, a.exp_avg_sq, a.flat16)]

    # the data-parallel reducer's pipelined branch: begin_step + step_range per bucket (reverse layout order) == step()
    restore()
    opt.begin_step()
    buckets = a.bucket_slices(8 << 20)
    assert len(buckets) > 8
    for s, e in buckets:
        opt.step_range(s, e)
    torch.cuda.synchronize()
    for got, w_, what in zip((a.flat32, a.exp_avg, a.exp_avg_sq, a.flat16), stepped, ("p", "m", "v", "shadow")):
        assert torch.equal(got, w_), f"bucket-wise step: {what}"
    assert (a.grad == 0).all()

    # its clip branch: optimizer.step(clip_norm) — the norm leaves the frozen embedding out
    restore()
    opt.step(clip_norm=0.1)
    torch.cuda.synchronize()
    live = grad.clone(); live[o:o + cap] = 0
    ref_norm = live.double().norm().item()
    # the check must be able to tell: the frozen gradient moves the norm by at least 10x the tolerance below
    assert grad.double().norm().item() > ref_norm * (1 + 1e-4), "the frozen gradient would show in the norm"
    assert abs(opt.clip[1].item() - ref_norm) <= 1e-5 * ref_norm, (opt.clip[1].item(), ref_norm)
    assert torch.equal(a.flat32[o:o + cap], snap[0][o:o + cap]) and (a.grad == 0).all()


def test_planned_steps_with_param_groups_replay_like_eager():
    """three planned steps against three eager steps with the same spec: the bounds of test_planned_step_replays_like_eager."""
    from vacnic_amd import ops, streams, synthetic
    from vacnic_amd.training import PlannedTrainStep, TrainArgs, build_models, to_device, train_step
    cfg = small_cfg()
    args = TrainArgs(num_training_steps=20, warmup_rate=0.1, lr_bart=1e-4)
    batches = [to_device(synthetic.make_batch(cfg, 3, S=32, T=12, F=3, seed=40 + i, image_size=32), "cuda") for i in range(3)]
    streams.enable(True)
    try:
        runs, weights = [], []
        for planned in (False, True):
            ops.Rng.manual_seed(3); ops.Rng.device_counter().zero_()
            model, guide, _ = build_models(cfg, _vcfg(), init="synthetic", seed=0)
            emb0 = model.model.shared.weight.detach().clone()
            opt = _grouped_opt(model, args, num_warmup_steps=2, num_training_steps=20)
            if planned:
                step = PlannedTrainStep(model, guide, opt, args, batches[0], warmup=2)
                losses = [step(b).tolist() for b in batches[1:] + batches[:1]]
                step.close()
            else:
                for _ in range(3):
                    train_step(model, guide, opt, batches[0], args)
                losses = [train_step(model, guide, opt, b, args).tolist() for b in batches[1:] + batches[:1]]
            torch.cuda.synchronize()
            assert torch.equal(model.model.shared.weight, emb0), "the frozen embedding stays through six steps"
            assert opt.hyper[1].item() == 6.0
            runs.append(np.array(losses))
            weights.append(model.arena.flat32.clone())
        assert np.isfinite(runs[1]).all()
        np.testing.assert_allclose(runs[1], runs[0], rtol=2e-3, atol=1e-4)
        rel = ((weights[1] - weights[0]).norm() / weights[0].norm()).item()
        assert rel < 1e-4, rel
    finally:
        streams.enable(False)


def test_checkpoint_resume_with_param_groups():
    """save after step 1, restore into a differently initialised model with the same spec: step 2 matches (the first-step bound of
    test_checkpoint_resume: fp32 atomics-order noise)."""
    from vacnic_amd import checkpoint, ops, streams, synthetic
    from vacnic_amd.training import FusedAdamW, TrainArgs, build_models, to_device, train_step
    cfg = small_cfg()
    args = TrainArgs(num_training_steps=20, warmup_rate=0.1, lr_bart=1e-4)
    batches = [to_device(synthetic.make_batch(cfg, 3, S=32, T=12, F=3, seed=20 + i, image_size=32), "cuda") for i in range(2)]
    streams.enable(False)
    ops.Rng.manual_seed(7); ops.Rng.device_counter().zero_()
    model, guide, _ = build_models(cfg, _vcfg(), init="synthetic", seed=0)
    opt = _grouped_opt(model, args, num_warmup_steps=0, num_training_steps=20)
    train_step(model, guide, opt, batches[0], args)
    buf = io.BytesIO()
    ck = checkpoint.save_checkpoint(buf, model, opt, step=1)
    assert ck["schedule"]["param_groups"] == opt.param_groups
    want = train_step(model, guide, opt, batches[1], args).tolist()
    model2, _, _ = build_models(cfg, _vcfg(), init="synthetic", seed=5)
    model2.clip_model = model.clip_model
    opt2 = _grouped_opt(model2, args, num_warmup_steps=0, num_training_steps=20)
    buf.seek(0)
    assert checkpoint.load_checkpoint(buf, model2, opt2)["step"] == 1 and opt2.hyper[1].item() == 1.0
    got = train_step(model2, guide, opt2, batches[1], args).tolist()
    np.testing.assert_allclose(np.array(got), np.array(want), rtol=2e-5, atol=1e-5)
    torch.cuda.synchronize()
    assert torch.equal(model2.model.shared.weight, model.model.shared.weight)
    rel = ((model2.arena.flat32 - model.arena.flat32).norm() / model.arena.flat32.norm()).item()
    assert rel < 1e-4, rel
    plain = FusedAdamW(model2.arena, lr=args.lr_bart, weight_decay=args.weight_decay, num_warmup_steps=0, num_training_steps=20)
    with pytest.raises(ValueError, match="param_groups=None"):
        checkpoint.load_checkpoint(ck, model2, plain)
