"""Moving average of the weights on the MI355X (vacnic_adamw_ema, vacnic_ema_swap, FusedAdamW(ema_decay=...)): the fused kernel
leaves AdamW bit for bit what the two existing entry points compute, the average against float64, frozen segments, straddling
vectors, dropped steps and range-wise steps, the swap, and the optimizer, launch plan, guard and checkpoint at model level, and the trainer entry point through to the stand-alone caption generator.

Bound of the average (per element, none left out): the kernel computes fma(d, ema, fl((1 - d) * p)) — two roundings, each within
2^-24 of a value no larger than max(|ema|, |p|) — so |got - want| <= 2^-23 max(|ema|, |p|); the tests allow 2^-22."""
import io
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 4104                     # a multiple of 4, five 1024-element table blocks
# three segments, both boundaries inside a 4-vector (1030 = 4 * 257 + 2, 2051 = 4 * 512 + 3), the middle one frozen
SEGS = [(0, 1030, 1.0, 0.01, False), (1030, 2051, 1.0, 0.0, True), (2051, N, 10.0, 0.1, False)]
LR = 3e-5


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


def rnd(n, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(n, generator=g) * scale).to("cuda")


def table(segs=SEGS, n=N):
    from vacnic_amd.arena import table_from_segments
    t = table_from_segments(n, [(s, lr, wd, fr) for s, _, lr, wd, fr in segs]).to("cuda")
    assert t.nseg == len(segs)
    return t


def state(t=3.0, n=N):
    """p, g, m, v, shadow, ema, hyper = {LR, t}: moments as after some steps, the shadow and the average from values no update gives"""
    p, g = rnd(n, 1), rnd(n, 2)
    m, v = rnd(n, 3, 0.1), rnd(n, 4).abs() * 0.01
    p16 = torch.full((n,), 7.0, device="cuda", dtype=torch.bfloat16)
    ema = rnd(n, 5)
    return [p, g, m, v, p16, ema, torch.tensor([LR, float(t)], device="cuda")]


def same(a, b, what, names=("p", "g", "m", "v", "shadow")):
    for x, y, nm in zip(a, b, names):
        assert torch.equal(x, y), f"{what}: {nm} differs in {(x != y).sum().item()} of {x.numel()} elements"


def decay_at(decay, warmup, t):
    """this step's d and 1 - d as the kernel computes them: in float32"""
    f = np.float32
    d = f(decay)
    if warmup:
        d = min(d, (f(1) + f(t)) / (f(10) + f(t)))
    return f(d), f(1) - f(d)


def check_average(ema_new, ema_old, p_new, decay, warmup, t, where=slice(None), what=""):
    d, omd = decay_at(decay, warmup, t)
    e0, pn = ema_old[where].double(), p_new[where].double()
    want = float(d) * e0 + float(omd) * pn
    err = (ema_new[where].double() - want).abs()
    bound = 2.0 ** -22 * torch.maximum(e0.abs(), pn.abs())
    bad = int((err > bound).sum())
    print(f"{what} d={float(d):.8f} t={t}: max err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f} over {err.numel()} elements")
    assert bad == 0, f"{what}: {bad}/{err.numel()} elements of the average beyond 2^-22 max(|ema|, |p|); max err {err.max().item():.3g}"
    assert (ema_new[where] != ema_old[where]).float().mean() > 0.99, f"{what}: the average moved"


# ------------------------------------------------------------------------------------------------ 1, 2: AdamW is unchanged
@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("with_clip", [False, True])
def test_ungrouped_adamw_is_bitwise_the_existing_kernel(K, with_clip, grad_scale, zero_grad):
    clip = torch.tensor([0.37, 5.0], device="cuda") if with_clip else None
    A, B = state(), state()
    K.adamw(*A[:5], A[6], N, weight_decay=0.01, grad_scale=grad_scale, zero_grad=bool(zero_grad), clip_coef=clip)
    K.adamw_ema(*B[:5], B[6], N, B[5], 0.999, True, weight_decay=0.01, grad_scale=grad_scale, zero_grad=bool(zero_grad), clip_coef=clip)
    same(A[:5], B[:5], f"clip {with_clip} grad_scale {grad_scale} zero_grad {zero_grad}")
    assert (A[0] != state()[0]).float().mean() > 0.99 and bool((A[1] == 0).all()) == bool(zero_grad)
    assert torch.equal(A[5], state()[5]) and (B[5] != A[5]).float().mean() > 0.99, "only the new entry point writes an average"


@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
@pytest.mark.parametrize("with_clip", [False, True])
def test_grouped_adamw_is_bitwise_the_existing_kernel(K, with_clip, grad_scale, zero_grad):
    clip = torch.tensor([0.37, 5.0], device="cuda") if with_clip else None
    tab = table()
    A, B = state(), state()
    K.adamw_groups(*A[:5], A[6], N, tab, grad_scale=grad_scale, zero_grad=bool(zero_grad), clip_coef=clip)
    K.adamw_ema(*B[:5], B[6], N, B[5], 0.999, True, table=tab, weight_decay=123.0, grad_scale=grad_scale, zero_grad=bool(zero_grad),
                clip_coef=clip)                                    # (with a table the struct's own weight decay is not read)
    same(A[:5], B[:5], f"clip {with_clip} grad_scale {grad_scale} zero_grad {zero_grad}")
    p0 = state()[0]
    assert torch.equal(A[0][1030:2051], p0[1030:2051])
    assert (A[0][:1030] != p0[:1030]).float().mean() > 0.99 and (A[0][2051:] != p0[2051:]).float().mean() > 0.99


# ----------------------------------------------------------------------------------------------- 3: the average in float64
@pytest.mark.parametrize("warmup,t", [(True, 1), (True, 5), (True, 1000), (False, 5)])
@pytest.mark.parametrize("decay", [0.9, 0.9999])
def test_average_against_float64(K, decay, warmup, t):
    S = state(t)
    ema0 = S[5].clone()
    K.adamw_ema(*S[:5], S[6], N, S[5], decay, warmup, weight_decay=0.01)
    if warmup and t == 1:
        assert float(decay_at(decay, warmup, t)[0]) == float(np.float32(2) / np.float32(11)), "the warm-up holds the decay down early on"
    check_average(S[5], ema0, S[0], decay, warmup, t, what=f"decay {decay} warm-up {warmup}")
    assert S[6].tolist() == [pytest.approx(LR), float(t)], "hyper is read, not written"


# ------------------------------------------------------------------------------------ 4: frozen and straddling elements
def test_frozen_segment_keeps_its_average_also_inside_shared_vectors(K):
    tab = table()
    S = state(5)
    ema0 = S[5].clone()
    K.adamw_ema(*S[:5], S[6], N, S[5], 0.9, False, table=tab)
    assert torch.equal(S[5][1030:2051], ema0[1030:2051]), "the frozen segment's average was written"
    # 1028..1031 and 2048..2051 are the two vectors a boundary cuts: 1030, 1031 and 2048..2050 frozen, their neighbours trained
    for lo, hi in ((0, 1030), (2051, N), (1028, 1030), (2051, 2052)):
        check_average(S[5], ema0, S[0], 0.9, False, 5, slice(lo, hi), what=f"trained [{lo}, {hi})")


# ------------------------------------------------------------------------------------------------------------- 5: skip
@pytest.mark.parametrize("grouped", [False, True])
def test_skipped_step_leaves_everything_but_the_gradient(K, grouped):
    tab = table() if grouped else None
    S, S0 = state(), state()
    skip = torch.tensor([1, 0, 0, -1], device="cuda", dtype=torch.int64)
    K.adamw_ema(*S[:5], S[6], N, S[5], 0.9, True, table=tab, skip=skip)
    same([S[i] for i in (0, 2, 3, 4, 5)], [S0[i] for i in (0, 2, 3, 4, 5)], "skipped step", ("p", "m", "v", "shadow", "ema"))
    assert (S[1] == 0).all(), "the gradient is still cleared"
    A, B = state(), state()
    skip[0] = 0
    K.adamw_ema(*A[:5], A[6], N, A[5], 0.9, True, table=tab, skip=skip)
    K.adamw_ema(*B[:5], B[6], N, B[5], 0.9, True, table=tab, skip=None)
    same(A[:6], B[:6], "skip flag 0 against no flag", ("p", "g", "m", "v", "shadow", "ema"))
    assert (A[5] != S0[5]).any()


# ----------------------------------------------------------------------------------------------------- 6, 10: optimizer
class _Arena:
    """the fields FusedAdamW uses of a ParamArena; group_table hands out the test's table"""

    def __init__(self, S):
        self.flat32, self.grad, self.flat16 = S[0], S[1], S[4]
        self.n, self.device = S[0].numel(), S[0].device
        self.exp_avg = self.exp_avg_sq = self.ema = None
        self.refresh_hooks = []
        self._ema0 = S[5]

    def init_optimizer_state(self):
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.flat32), torch.zeros_like(self.flat32)

    def init_ema(self):
        self.ema = self._ema0.clone()                               # (an average that differs from the weights from the start)

    def group_table(self, named, spec, wd):
        return table().to("cpu")


def _opt(grouped=True, **kw):
    from vacnic_amd.training import FusedAdamW
    a = _Arena(state())
    groups = dict(param_groups=[{"match": "middle", "frozen": True}], named_parameters=[]) if grouped else {}
    return a, FusedAdamW(a, lr=LR, weight_decay=0.01, num_warmup_steps=0, num_training_steps=100, ema_decay=0.9, **groups, **kw)


def test_two_range_steps_equal_one_whole_arena_step():
    whole, ow = _opt()
    parts, op = _opt()
    ow.step()
    op.begin_step()
    op.step_range(2052, N)                                          # (the reducer steps buckets in reverse layout order)
    op.step_range(0, 2052)
    torch.cuda.synchronize()
    names = ("p", "g", "m", "v", "shadow", "ema")
    same([getattr(whole, f) for f in ("flat32", "grad", "exp_avg", "exp_avg_sq", "flat16", "ema")],
         [getattr(parts, f) for f in ("flat32", "grad", "exp_avg", "exp_avg_sq", "flat16", "ema")], "range-wise", names)
    assert torch.equal(whole.ema[1030:2051], whole._ema0[1030:2051]) and (whole.ema[:1030] != whole._ema0[:1030]).float().mean() > 0.99
    assert ow.hyper[1].item() == op.hyper[1].item() == 1.0


def test_guard_drops_the_average_update_with_the_step():
    """a NaN in the gradient arena: the average stays bitwise; the next clean step updates it with the t the dropped step did not
    consume (visible in the warm-up's decay: t = 2 gives 3/12, t = 3 would give 4/13)."""
    a, opt = _opt(grouped=False, skip_nonfinite=True)
    g = state()[1]
    opt.step()                                                      # t = 1
    torch.cuda.synchronize()
    before = [t.clone() for t in (a.flat32, a.exp_avg, a.exp_avg_sq, a.flat16, a.ema)]
    a.grad.copy_(g); a.grad[1234] = float("nan")
    opt.step()                                                      # dropped
    torch.cuda.synchronize()
    same([a.flat32, a.exp_avg, a.exp_avg_sq, a.flat16, a.ema], before, "dropped step", ("p", "m", "v", "shadow", "ema"))
    assert (a.grad == 0).all() and opt.hyper[1].item() == 1.0 and opt.guard_report()["skipped"] == 1
    a.grad.copy_(g)
    opt.step()                                                      # t = 2
    torch.cuda.synchronize()
    assert opt.hyper[1].item() == 2.0
    check_average(a.ema, before[4], a.flat32, 0.9, True, 2, what="the clean step after the dropped one")
    assert float(decay_at(0.9, True, 2)[0]) == 0.25


# ------------------------------------------------------------------------------------------------------------- 7: swap
@pytest.mark.parametrize("n", [N, 4])
def test_swap_exchanges_contents_and_a_second_swap_restores(K, n):
    p, ema = rnd(n, 1), rnd(n, 5)
    p16 = K.cast_f32_bf16(p)
    p0, e0, s0 = p.clone(), ema.clone(), p16.clone()
    ptrs = (p.data_ptr(), ema.data_ptr(), p16.data_ptr())
    K.ema_swap(p, ema, p16)
    assert torch.equal(p, e0) and torch.equal(ema, p0), "contents are exchanged"
    assert torch.equal(p16, K.cast_f32_bf16(e0)) and not torch.equal(p16, s0), "the shadow is the cast of the new weights"
    K.ema_swap(p, ema, p16)
    assert torch.equal(p, p0) and torch.equal(ema, e0) and torch.equal(p16, s0), "a second swap restores all three"
    assert ptrs == (p.data_ptr(), ema.data_ptr(), p16.data_ptr())


# ------------------------------------------------------------------------------------------------------ 8-11: model level
def small_cfg(**kw):
    from vacnic_amd.config import VacnicConfig
    base = dict(d_model=768, encoder_layers=1, decoder_layers=1, encoder_attention_heads=12, decoder_attention_heads=12,
                encoder_ffn_dim=3072, decoder_ffn_dim=3072, enc_fusion_layer=[0], dim_common=768, clip_width=768, dropout=0.0)
    base.update(kw)
    return VacnicConfig(**base)


def _vcfg():
    from vacnic_amd.config import ClipVisionConfig
    return ClipVisionConfig(width=768, layers=1, patch_size=16, image_size=32, output_dim=64)


def close(a, b, rtol, atol, what=""):
    a = a.float(); b = b.float()
    err = (a - b).abs()
    bound = atol + rtol * b.abs()
    bad = (err > bound).sum().item()
    assert bad == 0, f"{what}: {bad}/{a.numel()} off; max err {err.max().item():.4g} (ref max {b.abs().max().item():.4g})"


def model_spec(model):
    from vacnic_amd.arena import no_decay_spec
    return [{"match": r"^model\.shared\.", "frozen": True}, {"match": "prompt_mlp|visual_map", "lr_scale": 10.0}] + no_decay_spec(model)


def _grouped_opt(model, args, **kw):
    from vacnic_amd.training import FusedAdamW
    return FusedAdamW(model.arena, lr=args.lr_bart, weight_decay=args.weight_decay, param_groups=model_spec(model),
                      named_parameters=model.named_parameters(), **kw)


def test_model_average_matches_torch_adamw_with_a_float64_average():
    """five eager steps, ema_decay 0.9 without warm-up, against torch.optim.AdamW fed the same gradients and an average kept in
    float64.  The average is a convex combination of the initial weights and the weights after each step, so it deviates by no more
    than the weights do: the weight tolerance of test_model_step_matches_torch_param_groups (1e-5 / 1e-7) serves for both."""
    from vacnic_amd import ops, streams, synthetic
    from vacnic_amd.training import (FusedAdamW, TrainArgs, build_models, eval_epoch, forward_losses, gen_caption_from_loader_bart,
                                     to_device)
    cfg = small_cfg()
    args = TrainArgs(num_training_steps=20, lr_bart=1e-4)
    streams.enable(False)
    ops.Rng.manual_seed(3); ops.Rng.device_counter().zero_()
    model, guide, _ = build_models(cfg, _vcfg(), init="synthetic", seed=0)
    model.train()
    a = model.arena
    opt = FusedAdamW(a, lr=args.lr_bart, weight_decay=args.weight_decay, num_warmup_steps=0, num_training_steps=1e9,
                     ema_decay=0.9, ema_warmup=False)
    assert torch.equal(a.ema, a.flat32) and a.ema.data_ptr() != a.flat32.data_ptr() and "ema" in opt.state_dict()
    batch = to_device(synthetic.make_batch(cfg, 3, S=32, T=12, F=3, seed=40, image_size=32), "cuda")
    ref = torch.nn.Parameter(a.flat32.clone())
    topt = torch.optim.AdamW([ref], lr=args.lr_bart, betas=(0.9, 0.999), eps=1e-8, weight_decay=args.weight_decay)
    avg = ref.data.double().clone()
    for _ in range(5):
        ops.begin_step()
        total, _, _ = forward_losses(model, guide, batch, args)
        with torch.autograd.set_multithreading_enabled(False):
            total.backward(ops.const_one(total.device))
        ops.flush_wgrads()
        streams.join_all()
        ref.grad = a.grad.clone()
        topt.step()
        avg = 0.9 * avg + 0.1 * ref.data.double()
        opt.step()
    torch.cuda.synchronize()
    close(a.flat32, ref.data, 1e-5, 1e-7, "weights after five steps")
    close(a.ema, avg, 1e-5, 1e-7, "average after five steps")
    assert (a.ema != a.flat32).float().mean() > 0.5 and opt.hyper[1].item() == 5.0

    # inside ema_weights() the model evaluates with the average, through the shadow and the fp32 views alike
    w0, s0, e0 = a.flat32.clone(), a.flat16.clone(), a.ema.clone()
    model2, _, _ = build_models(cfg, _vcfg(), init="synthetic", seed=5)
    model2.clip_model = model.clip_model
    model2.arena.flat32.copy_(e0); model2.arena.refresh_shadow()
    want, _ = eval_epoch(model2, [batch])
    plain, _ = eval_epoch(model, [batch])
    # generate: greedy, eight positions.  The first call, with the weights themselves, builds the model's cached decode session;
    # the call inside the context then runs on that session and must still see the average (the session holds addresses)
    gen = lambda m: gen_caption_from_loader_bart(m, [batch], 1, 8, pipeline=False)[0]["gen"]      # noqa: E731
    want_gen, plain_gen = gen(model2), gen(model)
    with opt.ema_weights():
        got_gen = gen(model)
        assert got_gen == want_gen, ("generate inside ema_weights()", got_gen, want_gen)
        assert opt.ema_swapped and torch.equal(a.flat32, e0) and torch.equal(a.flat16, model2.arena.flat16) and torch.equal(a.ema, w0)
        assert torch.equal(model.model.shared.weight.data.reshape(-1), model2.model.shared.weight.data.reshape(-1))
        got, _ = eval_epoch(model, [batch])
        with pytest.raises(RuntimeError, match="swapped in"):
            opt.step()
    print(f"eval loss with the average {got:.6f}, a model loaded with it {want:.6f}, with the weights {plain:.6f}")
    print(f"greedy ids with the average {got_gen[0]}, with the weights {plain_gen[0]}")
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-5)     # (the loss bound of test_checkpoint_resume_with_param_groups)
    assert abs(plain - want) > 1e-5 + 2e-5 * abs(want), "the check can tell the average from the weights"
    assert not opt.ema_swapped and torch.equal(a.flat32, w0) and torch.equal(a.flat16, s0) and torch.equal(a.ema, e0)
    with pytest.raises(ZeroDivisionError):
        with opt.ema_weights():
            1 / 0
    assert not opt.ema_swapped and torch.equal(a.flat32, w0) and torch.equal(a.flat16, s0) and torch.equal(a.ema, e0), \
        "an exception inside the context swaps back too"
    assert model.training


def test_planned_steps_with_the_average_replay_like_eager():
    """three planned steps against three eager steps, parameter groups and the average on: the bounds of
    test_planned_steps_with_param_groups_replay_like_eager, for the weights and for the average."""
    from vacnic_amd import ops, streams, synthetic
    from vacnic_amd.training import PlannedTrainStep, TrainArgs, build_models, to_device, train_step
    cfg = small_cfg()
    args = TrainArgs(num_training_steps=20, warmup_rate=0.1, lr_bart=1e-4, ema_decay=0.9)
    batches = [to_device(synthetic.make_batch(cfg, 3, S=32, T=12, F=3, seed=40 + i, image_size=32), "cuda") for i in range(3)]
    streams.enable(True)
    try:
        runs, weights, averages = [], [], []
        for planned in (False, True):
            ops.Rng.manual_seed(3); ops.Rng.device_counter().zero_()
            model, guide, _ = build_models(cfg, _vcfg(), init="synthetic", seed=0)
            emb0 = model.model.shared.weight.detach().clone()
            start = model.arena.flat32.clone()
            opt = _grouped_opt(model, args, num_warmup_steps=2, num_training_steps=20, ema_decay=0.9)
            if planned:
                step = PlannedTrainStep(model, guide, opt, args, batches[0], warmup=2)
                losses = [step(b).tolist() for b in batches[1:] + batches[:1]]
                step.close()
            else:
                for _ in range(3):
                    train_step(model, guide, opt, batches[0], args)
                losses = [train_step(model, guide, opt, b, args).tolist() for b in batches[1:] + batches[:1]]
            torch.cuda.synchronize()
            a = model.arena
            o, n, cap = a.slots[id(model.model.shared.weight)]
            assert torch.equal(model.model.shared.weight, emb0) and torch.equal(a.ema[o:o + cap], start[o:o + cap]), \
                "the frozen embedding and its average stay through six steps"
            assert opt.hyper[1].item() == 6.0
            live = torch.ones(a.n, dtype=torch.bool, device="cuda")
            live[o:o + cap] = False                                 # (the frozen embedding is most of this small model's arena)
            assert (a.ema != start)[live].float().mean() > 0.9 and (a.ema != a.flat32)[live].float().mean() > 0.9
            runs.append(np.array(losses)); weights.append(a.flat32.clone()); averages.append(a.ema.clone())
        assert np.isfinite(runs[1]).all()
        np.testing.assert_allclose(runs[1], runs[0], rtol=2e-3, atol=1e-4)
        for pair, what in ((weights, "weights"), (averages, "average")):
            rel = ((pair[1] - pair[0]).norm() / pair[0].norm()).item()
            assert rel < 1e-4, (what, rel)
    finally:
        streams.enable(False)


def test_checkpoint_resume_with_the_average():
    """save after step 1, restore into a differently initialised model, step 2: the average matches the uninterrupted run's (the
    bound of test_checkpoint_resume_with_param_groups); weights="ema" loads the stored average as the weights, bit for bit."""
    from vacnic_amd import checkpoint, ops, streams, synthetic
    from vacnic_amd.training import TrainArgs, build_models, to_device, train_step
    cfg = small_cfg()
    args = TrainArgs(num_training_steps=20, warmup_rate=0.1, lr_bart=1e-4, ema_decay=0.9)
    batches = [to_device(synthetic.make_batch(cfg, 3, S=32, T=12, F=3, seed=20 + i, image_size=32), "cuda") for i in range(2)]
    streams.enable(False)
    ops.Rng.manual_seed(7); ops.Rng.device_counter().zero_()
    model, guide, _ = build_models(cfg, _vcfg(), init="synthetic", seed=0)
    opt = _grouped_opt(model, args, num_warmup_steps=0, num_training_steps=20, ema_decay=0.9)
    train_step(model, guide, opt, batches[0], args)
    torch.cuda.synchronize()
    saved = model.arena.ema.clone()
    assert (saved != model.arena.flat32).float().mean() > 0.04     # (everything but the frozen embedding, which is most of the arena)
    buf = io.BytesIO()
    ck = checkpoint.save_checkpoint(buf, model, opt, step=1)
    assert ck["schedule"]["ema_decay"] == 0.9 and ck["schedule"]["ema_warmup"] is True
    assert sorted(ck["optimizer"]["ema"]) == sorted(ck["optimizer"]["exp_avg"])
    with opt.ema_weights():
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            checkpoint.save_checkpoint(io.BytesIO(), model, opt, step=1)
    want = train_step(model, guide, opt, batches[1], args).tolist()
    model2, _, _ = build_models(cfg, _vcfg(), init="synthetic", seed=5)
    model2.clip_model = model.clip_model
    opt2 = _grouped_opt(model2, args, num_warmup_steps=0, num_training_steps=20, ema_decay=0.9)
    buf.seek(0)
    assert checkpoint.load_checkpoint(buf, model2, opt2)["step"] == 1 and opt2.hyper[1].item() == 1.0
    assert torch.equal(model2.arena.ema, saved), "the stored average is restored exactly"
    got = train_step(model2, guide, opt2, batches[1], args).tolist()
    np.testing.assert_allclose(np.array(got), np.array(want), rtol=2e-5, atol=1e-5)
    torch.cuda.synchronize()
    for x, y, what in ((model2.arena.flat32, model.arena.flat32, "weights"), (model2.arena.ema, model.arena.ema, "average")):
        rel = ((x - y).norm() / y.norm()).item()
        assert rel < 1e-4, (what, rel)
    assert (model2.arena.ema != saved).any()
    buf.seek(0)
    checkpoint.load_checkpoint(buf, model2, weights="ema")          # (no optimizer: inference from a training checkpoint)
    assert torch.equal(model2.arena.flat32, saved), "weights='ema': the model's weights are the stored average"
    assert torch.equal(model2.arena.flat16, saved.to(torch.bfloat16))


# ----------------------------------------------------------------------------------------------------------------- trainer
def test_trainer_validates_captions_and_exports_with_the_average(tmp_path):
    """--ema_decay through the trainer entry point (launch plans on): validation and test captioning run inside ema_weights(), every
    checkpoint gets an inference twin whose weights are the average, and the stand-alone caption generator — which knows nothing of
    averages — reproduces from that twin the captions the trainer wrote from the swapped-in weights."""
    import importlib.util
    import json
    from vacnic_amd import checkpoint, streams

    def load(path, name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    trainer = load("train_mmbart_enc_self_face_name_ids_retrieve_crossattn_bart_guide_match.py", "trainer_ema_test")
    args = trainer.parser.parse_args(["--plm_type", "facebook/bart-base", "--clip_type", "ViT-B/32", "--enc_fusion_layer", "0", "1",
                                      "--dim_common", "768", "--train_batch_size", "2", "--article_max_length", "64", "--steps_per_epoch", "4",
                                      "--log_every", "2", "--out_dir", str(tmp_path), "--experiment_name", "t", "--lr_bart", "1e-3",
                                      "--ema_decay", "0.9", "--val_steps", "1", "--test_steps", "1", "--beam_size", "2", "--max_length", "8"])
    assert trainer.ema_eval(args)
    try:
        hist = trainer.run(args)
    finally:
        streams.enable(False)
        torch.cuda.synchronize()
    assert len(hist) == 2 and np.isfinite([h["loss"] for h in hist]).all()
    files = sorted(f for f in os.listdir(tmp_path) if f.endswith(".pt"))
    assert files == ["t.pt", "t_ema.pt", "tlast.pt", "tlast_ema.pt"], files
    full = torch.load(tmp_path / "tlast.pt", map_location="cpu", weights_only=False)
    twin = torch.load(tmp_path / "tlast_ema.pt", map_location="cpu", weights_only=False)
    assert full["schedule"]["ema_decay"] == 0.9 and full["optimizer"]["step"] == 4
    assert sorted(twin) == ["meta", "model"] and twin["meta"]["weights"] == "ema" and twin["meta"]["config"] == full["meta"]["config"]
    moved = 0
    for name, avg in full["optimizer"]["ema"].items():
        assert torch.equal(twin["model"][name], avg), name
        moved += int(not torch.equal(avg, full["model"][name]))
    assert moved > 0.5 * len(full["optimizer"]["ema"]), "the saved weights are the weights, not the average (swapped back before saving)"
    assert checkpoint.ema_as_model(full)["model"].keys() == twin["model"].keys()
    want = json.load(open(tmp_path / "t.json"))                     # the trainer's test captions, generated inside ema_weights()
    gen = load(os.path.join("utils", "test_mmbart_clip_ddp.py"), "generator_ema_test")
    gargs = gen.parser.parse_args(["--model_dir", str(tmp_path), "--model_name", "tlast_ema", "--beam_size", "2", "--max_length", "8",
                                   "--length_penalty", "1.0", "--test_batch_size", "1", "--test_steps", "1", "--article_max_length", "64"])
    gen.run(gargs)
    torch.cuda.synchronize()
    got = json.load(open(tmp_path / "tlast_emabeam2_max8t_S684331_lp1.0.json"))
    assert got["0"]["gen"] == want["0"]["gen"] and got["0"]["gt"] == want["0"]["gt"], (got, want)
