"""Gradient accumulation on the MI355X (vacnic_lr_step_accum, the step word's third value, FusedAdamW(accum_steps=k),
--grad_accum_steps): a held micro-batch writes nothing but the counters; the applying one writes bit for bit what the existing
entry points write for the summed gradient scaled by 1 / k; against torch.optim.AdamW + LambdaLR fed the group means; with the
guard and the statistics; and the optimizer, launch plan, checkpoint and trainer at model level.  Helpers, sizes and tolerances are
those of tests/test_grad_guard_gpu.py (rtol 1e-5 / atol 1e-7 on fp32 parameters, 4e-3 / 1e-6 for the bf16 shadow)."""
import importlib.util
import io
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_grad_guard_gpu as G                      # noqa: E402  (its helpers, and its one gradient per size, made once)

N, NBIG, LR, WARM, TOTAL, NAN = G.N, G.NBIG, G.LR, G.WARM, G.TOTAL, G.NAN
EMA_DECAY = 0.999
SENT = -7.0                                          # pre-fill of the clip pair {coefficient, norm}: neither can be negative
# statistics slots (offset, numel) per size: single elements, an unaligned start, a gap, a slot of many units on the big arena
STAT_SLOTS = {4: [(0, 1), (1, 3)], N: [(0, 1), (1, 3), (5, 4095), (4101, 3)], NBIG: [(0, 1), (1, 4099), (4101, NBIG - 4101)]}


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


def fresh(n, j):
    """the gradient micro-batch j adds: the file's one gradient per size, rotated and rescaled (never written)"""
    return torch.roll(G.grad(n), 17 * j) * (1.0 + 0.25 * j)


def bits(t):
    """bitwise comparison that also holds for NaN"""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.int64)


def same(x, y):
    return torch.equal(bits(x), bits(y))


class Run:
    """everything one optimizer over a raw arena owns, for the kernel-level tests"""

    def __init__(self, K, n, grouped, ema):
        from vacnic_amd.arena import stats_table_from_slots
        self.K, self.n = K, n
        self.st, self.hyper, _ = G.state(n, K)
        self.ema = G.rnd(n, dtype=torch.float32, seed=5) if ema else None
        self.tab = G.tab_for(n, grouped)
        self.g = torch.zeros(n, device="cuda")
        self.rng = torch.zeros(1, device="cuda", dtype=torch.int64)
        self.out = torch.full((2,), SENT, device="cuda")
        self.partials = torch.zeros(1024, device="cuda")
        self.stab = stats_table_from_slots(STAT_SLOTS[n]).to("cuda")
        self.work = K.param_stats_workspace(self.stab, "cuda")
        self.out_f = torch.full((self.stab.nslot, 4), SENT, device="cuda")
        self.out_i = torch.full((self.stab.nslot, 2), -7, device="cuda", dtype=torch.int64)
        self.stamp = torch.zeros(4, device="cuda", dtype=torch.int64)

    def tensors(self):
        """what a held micro-batch must leave bitwise as it is"""
        return self.st + ([self.ema] if self.ema is not None else []) + [self.g, self.hyper, self.out, self.out_f, self.out_i, self.stamp]

    def names(self):
        return ["p", "m", "v", "shadow"] + (["ema"] if self.ema is not None else []) + ["g", "hyper", "clip out", "stats out_f",
                                                                                        "stats out_i", "stats stamp"]

    def optimizer_passes(self, scale, word, hold, clip_groups):
        """clip norm, statistics, AdamW: through the entry points that take `hold` (clip_groups) or the ones of before"""
        K, n = self.K, self.n
        if clip_groups:
            K.grad_clip_coef_groups(self.g, n, 0.1, self.tab, scale, self.partials, self.out, hold=hold)
        elif self.tab is None:
            K.grad_clip_coef(self.g, n, 0.1, scale, self.partials, self.out)
        else:
            K.grad_clip_coef_groups(self.g, n, 0.1, self.tab, scale, self.partials, self.out)
        K.param_stats(self.g, self.st[0], n, self.stab, self.hyper, 1, word, scale, self.work, self.out_f, self.out_i, self.stamp)
        p, m, v, p16 = self.st
        kw = dict(grad_scale=scale, clip_coef=self.out, skip=word)
        if self.ema is not None:
            K.adamw_ema(p, self.g, m, v, p16, self.hyper, n, self.ema, EMA_DECAY, True, self.tab, 0, **kw)
        elif self.tab is None:
            K.adamw(p, self.g, m, v, p16, self.hyper, n, **kw)
        else:
            K.adamw_groups(p, self.g, m, v, p16, self.hyper, n, self.tab, 0, **kw)


# --------------------------------------------------------------------------------- 1: hold writes nothing, apply is the old step
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("ema", [False, True])
@pytest.mark.parametrize("n,grouped", G.SIZES)
def test_hold_writes_nothing_and_apply_is_the_existing_step_bit_for_bit(K, n, grouped, ema, k):
    acc, ref = Run(K, n, grouped, ema), Run(K, n, grouped, ema)
    accum = K.accum_state("cuda")
    calls = 0
    for group in range(2):                                   # the second group: a hold after an apply, hyper and out no longer pristine
        for j in range(k):
            acc.g += fresh(n, group * k + j)
            before = [t.clone() for t in acc.tensors()]
            K.lr_step_accum(acc.hyper, LR, WARM, TOTAL, accum, k, acc.rng)
            calls += 1
            word = accum.tolist()
            assert acc.rng.item() == calls, "every micro-batch advances the dropout counter"
            if j < k - 1:
                assert word == [2, j + 1, group, 0], word
                acc.optimizer_passes(1.0 / k, accum, accum, clip_groups=True)
                for x, y, nm in zip(acc.tensors(), before, acc.names()):
                    assert same(x, y), f"group {group}, held micro-batch {j}: {nm} was written"
                continue
            assert word == [0, 0, group + 1, 0], word
            # the existing entry points on clones holding the same summed gradient, after a plain lr_step
            ref.g.copy_(acc.g)
            K.lr_step(ref.hyper, LR, WARM, TOTAL)
            assert same(acc.hyper, ref.hyper), (acc.hyper.tolist(), ref.hyper.tolist())
            ref.optimizer_passes(1.0 / k, None, None, clip_groups=False)
            acc.optimizer_passes(1.0 / k, accum, accum, clip_groups=True)
            for x, y, nm in zip(acc.tensors(), ref.tensors(), acc.names()):
                assert same(x, y), f"group {group}, applying micro-batch: {nm} differs in {(bits(x) != bits(y)).sum().item()} elements"
            assert (acc.g == 0).all() and acc.stamp.tolist()[:3] == [group + 1, group + 1, 0]
            assert acc.out[1].item() > 0 and (n == 4 or acc.out[0].item() < 1.0), "the clip bites: the coefficient is in the comparison"
    assert acc.hyper[1].item() == 2.0
    # the comparison is not one of two idle runs: the first moment of every trained element has moved (a quarter of the grouped
    # N = 4104 table is frozen), and weights have (the first group's learning rate is 0: the warm-up starts there)
    p0, m0 = G.state(n, K)[0][:2]
    assert (acc.st[1] != m0).float().mean().item() > (0.5 if grouped else 0.99) and (acc.st[0] != p0).any()


def test_k_of_one_is_lr_step_bit_for_bit_across_the_warmup_edge(K):
    ha, hb = torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda")
    ra, rb = torch.zeros(1, device="cuda", dtype=torch.int64), torch.zeros(1, device="cuda", dtype=torch.int64)
    accum = K.accum_state("cuda")
    for i in range(8):                                       # WARM = 5: calls 1..5 on the ramp, 6..8 on the decay
        K.lr_step_accum(ha, LR, WARM, TOTAL, accum, 1, ra)
        K.lr_step(hb, LR, WARM, TOTAL, rb)
        assert same(ha, hb), (i, ha.tolist(), hb.tolist())
        assert ra.item() == rb.item() == i + 1 and accum.tolist() == [0, 0, i + 1, 0]
    assert ha[1].item() == 8.0 and 0 < ha[0].item() < LR


def test_k_below_one_is_refused_before_any_launch(K):
    hyper, accum = torch.zeros(2, device="cuda"), K.accum_state("cuda")
    for k in (0, -3):
        with pytest.raises(ValueError, match="must be >= 1"):
            K.lr_step_accum(hyper, LR, WARM, TOTAL, accum, k)
    torch.cuda.synchronize()
    assert hyper.tolist() == [0.0, 0.0] and accum.tolist() == [0, 0, 0, 0]


def test_clip_groups_entry_without_a_table_is_the_plain_clip_pass(K):
    """null table pointers mean "ungrouped", as for the guard: FusedAdamW uses this entry for the plain clip path under accumulation"""
    for n in (4, N, NBIG):
        g = G.grad(n)
        want = K.grad_clip_coef(g, n, 0.1, 0.5)
        got = K.grad_clip_coef_groups(g, n, 0.1, None, 0.5)
        assert same(got, want), (n, got.tolist(), want.tolist())


# ---------------------------------------------------------------------------------------------------------- 2: against torch
def test_six_groups_of_three_match_torch_fed_the_group_means():
    from vacnic_amd.training import FusedAdamW
    a = G._Arena(G.rnd(N, dtype=torch.float32, seed=1))
    opt = FusedAdamW(a, lr=LR, weight_decay=0.01, num_warmup_steps=WARM, num_training_steps=TOTAL, accum_steps=3)
    ref = torch.nn.Parameter(a.flat32.clone())
    topt = torch.optim.AdamW([ref], lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    lam = lambda k: k / max(1.0, WARM) if k < WARM else max(0.0, (TOTAL - k) / max(1.0, TOTAL - WARM))
    sched = torch.optim.lr_scheduler.LambdaLR(topt, lam)
    for group in range(6):
        parts = [fresh(N, 3 * group + j) for j in range(3)]
        for j, part in enumerate(parts):
            a.grad += part                                   # what backward does: it adds into the arena
            opt.step()
            assert (a.grad == 0).all() if j == 2 else (a.grad != 0).any()
        ref.grad = ((parts[0].double() + parts[1].double() + parts[2].double()) / 3.0).float()
        topt.step(); sched.step()
    G.close(a.flat32, ref.data, 1e-5, 1e-7, "parameters after 6 groups of 3")
    G.close(a.flat16, a.flat32, 4e-3, 1e-6, "bf16 shadow")
    assert opt.hyper[1].item() == 6.0
    assert opt.accum_report() == {"accum_steps": 3, "pending": 0, "groups": 6}


# --------------------------------------------------------------------------------------------------------------- 3: the guard
@pytest.mark.parametrize("grouped", [False, True])
def test_guard_judges_the_group_and_a_nan_in_its_first_micro_batch_drops_it(K, grouped):
    tab = G.tab_for(N, grouped)
    where = 3000                                             # in a trained segment of the grouped table
    st, hyper, gs = G.state(N, K)
    accum = K.accum_state("cuda")
    out = torch.full((2,), SENT, device="cuda")
    g = torch.zeros(N, device="cuda")
    before = [t.clone() for t in st]
    g += fresh(N, 0)
    g[where] = NAN
    held = g.clone()
    K.lr_step_accum(hyper, LR, 0.0, TOTAL, accum, 2)
    K.grad_guard(g, N, hyper, gs, 0.1, tab, 0.5, out=out, hold=accum)
    G.adamw(K, st, g, hyper, N, tab, gs, clip=out)
    assert gs.tolist() == [2, 0, 0, -1], "held: nothing is counted, the verdict is 'hold'"
    assert same(g, held) and out.tolist() == [SENT, SENT] and hyper.tolist() == [0.0, 0.0] and accum.tolist() == [2, 1, 0, 0]
    for x, y in zip(st, before):
        assert same(x, y)
    g += fresh(N, 1)
    K.lr_step_accum(hyper, LR, 0.0, TOTAL, accum, 2)
    K.grad_guard(g, N, hyper, gs, 0.1, tab, 0.5, out=out, hold=accum)
    G.adamw(K, st, g, hyper, N, tab, gs, clip=out)
    assert gs.tolist() == [1, 1, 1, where], gs.tolist()
    assert (g == 0).all(), "the dropped group's gradient is zeroed"
    assert hyper[1].item() == 0.0, "a dropped group advances neither Adam's t nor the schedule position"
    assert accum.tolist() == [0, 0, 1, 0]
    for x, y, nm in zip(st, before, ("p", "m", "v", "shadow")):
        assert same(x, y), f"the dropped group wrote {nm}"
    # the next group is finite: applied, bitwise what the guard without `hold` gives for the same sum
    twin, th, tgs = G.state(N, K)
    tg = torch.zeros(N, device="cuda")
    tout = torch.zeros(2, device="cuda")
    for j in (2, 3):
        g += fresh(N, j); tg += fresh(N, j)
        K.lr_step_accum(hyper, LR, 0.0, TOTAL, accum, 2)
        K.grad_guard(g, N, hyper, gs, 0.1, tab, 0.5, out=out, hold=accum)
        G.adamw(K, st, g, hyper, N, tab, gs, clip=out)
    K.lr_step(th, LR, 0.0, TOTAL)
    K.grad_guard(tg, N, th, tgs, 0.1, tab, 0.5, out=tout)
    G.adamw(K, twin, tg, th, N, tab, tgs, clip=tout)
    assert gs.tolist() == [0, 1, 0, where] and hyper[1].item() == 1.0
    assert (st[0] != before[0]).any(), "(no warm-up: the applied group's learning rate is not 0)"
    for x, y, nm in zip(st + [g, hyper, out], twin + [tg, th, tout], ("p", "m", "v", "shadow", "g", "hyper", "{coef, norm}")):
        assert same(x, y), f"applied group after a dropped one: {nm} differs"


# ---------------------------------------------------------------------------------------------------------- 4: the statistics
def test_statistics_interval_counts_optimizer_steps(K):
    r = Run(K, N, False, False)
    accum = K.accum_state("cuda")
    fired = []
    for call in range(8):
        r.g += fresh(N, call)
        K.lr_step_accum(r.hyper, LR, WARM, TOTAL, accum, 2)
        K.param_stats(r.g, r.st[0], N, r.stab, r.hyper, 2, accum, 0.5, r.work, r.out_f, r.out_i, r.stamp)
        K.adamw(r.st[0], r.g, r.st[1], r.st[2], r.st[3], r.hyper, N, grad_scale=0.5, skip=accum)
        fired.append(r.stamp.tolist()[:2])
    assert fired == [[0, 0], [0, 0], [0, 0], [1, 2], [1, 2], [1, 2], [1, 2], [2, 4]], fired


# ------------------------------------------------------------------------------------------------------------ model level
def _clean_batches(cfg, count, seed=60):
    from vacnic_amd import synthetic
    from vacnic_amd.training import to_device
    return [to_device(synthetic.make_batch(cfg, 3, S=32, T=12, F=3, seed=seed + i, image_size=32), "cuda") for i in range(count)]


def _opt(model, k, **kw):
    from vacnic_amd.training import FusedAdamW
    return FusedAdamW(model.arena, lr=1e-4, weight_decay=0.01, num_warmup_steps=0, num_training_steps=20, accum_steps=k, **kw)


def _targs(k):
    from vacnic_amd.training import TrainArgs
    return TrainArgs(num_training_steps=20, warmup_rate=0.0, lr_bart=1e-4, grad_accum_steps=k)


def _grad_alone(model, guide, batch, args):
    """one batch's gradient from a plain forward / backward, no optimizer call; the arena is left zeroed"""
    from vacnic_amd import ops, streams
    from vacnic_amd.training import forward_losses
    a = model.arena
    ops.begin_step()
    total, _, _ = forward_losses(model, guide, batch, args)
    with torch.autograd.set_multithreading_enabled(False):
        total.backward(ops.const_one(total.device))
    ops.flush_wgrads()
    streams.join_all()
    torch.cuda.synchronize()
    g = a.grad.cpu().double()
    a.grad.zero_()
    return g


def test_eager_two_batches_are_one_step_on_their_mean_gradient():
    from vacnic_amd import ops, streams
    from vacnic_amd.training import build_models, train_step
    cfg = G.small_cfg()
    bs = _clean_batches(cfg, 2)
    streams.enable(False)
    ops.Rng.manual_seed(3); ops.Rng.device_counter().zero_()
    model, guide, _ = build_models(cfg, G._vcfg(), init="synthetic", seed=0)
    model.train()
    a = model.arena
    args = _targs(2)
    gref = (_grad_alone(model, guide, bs[0], args) + _grad_alone(model, guide, bs[1], args)) / 2.0      # float64, on the host
    p0, s0 = a.flat32.clone(), a.flat16.clone()
    opt = _opt(model, 2)
    before = G._arena_state(a) + [opt.hyper.clone()]
    train_step(model, guide, opt, bs[0], args)
    torch.cuda.synchronize()
    for x, y, nm in zip(G._arena_state(a) + [opt.hyper], before, ("flat32", "flat16", "exp_avg", "exp_avg_sq", "hyper")):
        assert same(x, y), f"the held batch wrote {nm}"
    assert (a.grad != 0).any() and opt.accum_report() == {"accum_steps": 2, "pending": 1, "groups": 0}
    train_step(model, guide, opt, bs[1], args)
    torch.cuda.synchronize()
    assert (a.grad == 0).all() and opt.accum_report() == {"accum_steps": 2, "pending": 0, "groups": 1}
    assert opt.hyper[1].item() == 1.0
    # float64 AdamW, first step (t = 1, zero moments), lr = lr_bart (no warm-up, schedule position 0)
    lr, wd, b1, b2, eps = 1e-4, 0.01, 0.9, 0.999, 1e-8
    # (the reference gradient was summed on the host; the float64 arithmetic on it runs on the device, where it takes no time)
    gref = gref.cuda()
    m, v = (1 - b1) * gref, (1 - b2) * gref * gref
    want = p0.double() * (1 - lr * wd) - (lr / (1 - b1)) * m / (v.sqrt() / np.sqrt(1 - b2) + eps)
    del gref, m, v
    err, bound = (a.flat32.double() - want).abs(), 1e-7 + 1e-5 * want.abs()
    print(f"accumulated step vs float64 AdamW on the mean gradient: max err {err.max().item():.3e}, "
          f"{(err > bound).sum().item()}/{err.numel()} over the bound, max err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all(), (err.max().item(), (err > bound).sum().item())
    # control: the same two batches as two optimizer steps land elsewhere
    a.flat32.copy_(p0); a.flat16.copy_(s0)
    for hook in a.refresh_hooks:
        hook()
    opt1 = _opt(model, 1)                                    # (re-creates zeroed moments on the same arena)
    for b in bs:
        train_step(model, guide, opt1, b, _targs(1))
    torch.cuda.synchronize()
    far = (a.flat32.double() - want).abs() > 10.0 * bound
    assert far.any() and opt1.hyper[1].item() == 2.0, "control: accum_steps=1 is a different computation"


def _four_micro_batches(record_at):
    """four batches, k = 2, through train_step (record_at None) or with a launch plan recorded on batch `record_at` (0: a held
    micro-batch, 1: an applying one) and replayed for the later ones; returns (losses, final flat32, hyper[1])."""
    from vacnic_amd import ops, streams
    from vacnic_amd.training import PlannedTrainStep, build_models, train_step
    cfg = G.small_cfg()
    args = _targs(2)
    bs = _clean_batches(cfg, 4)
    streams.enable(True)
    step = None
    try:
        ops.Rng.manual_seed(3); ops.Rng.device_counter().zero_()
        model, guide, _ = build_models(cfg, G._vcfg(), init="synthetic", seed=0)
        a = model.arena
        opt = _opt(model, 2)
        # a recording needs a warmed-up model (lazy buffers): one eager step (a held one), then everything it changed is put back
        keep = G._arena_state(a) + [opt.hyper.clone(), ops.Rng.device_counter().clone(), opt.accum.clone()]
        train_step(model, guide, opt, bs[0], args)
        torch.cuda.synchronize()
        for t, s_ in zip((a.flat32, a.flat16, a.exp_avg, a.exp_avg_sq, opt.hyper, ops.Rng.device_counter(), opt.accum), keep):
            t.copy_(s_)
        a.grad.zero_()
        for hook in a.refresh_hooks:
            hook()
        losses = []
        for i, b in enumerate(bs):
            if record_at is not None and i == record_at:
                step = PlannedTrainStep(model, guide, opt, args, b, warmup=0)
                out4 = step.out4
            elif step is not None:
                out4 = step(b)
            else:
                out4 = train_step(model, guide, opt, b, args)
            losses.append(out4.tolist())
            torch.cuda.synchronize()
        assert opt.accum_report() == {"accum_steps": 2, "pending": 0, "groups": 2} and (a.grad == 0).all()
        return losses, a.flat32.clone(), opt.hyper[1].item()
    finally:
        if step is not None:
            step.close()
        streams.enable(False)


_EAGER4 = {}


@pytest.mark.parametrize("record_at", [0, 1])
def test_a_plan_recorded_on_either_kind_of_micro_batch_replays_both(record_at):
    if not _EAGER4:
        _EAGER4["run"] = _four_micro_batches(None)
    want_l, want_w, want_t = _EAGER4["run"]
    losses, flat32, t = _four_micro_batches(record_at)
    assert t == 2.0 and want_t == 2.0
    np.testing.assert_allclose(np.array(losses), np.array(want_l), rtol=2e-3, atol=1e-4)
    rel = ((flat32 - want_w).norm() / want_w.norm()).item()
    assert rel < 1e-4, rel
    assert want_l[0] != want_l[2], "the second group runs on moved weights"


def test_checkpoint_on_a_group_boundary_resumes_and_mid_group_is_refused():
    from vacnic_amd import checkpoint, ops, streams
    from vacnic_amd.training import build_models, train_step
    cfg = G.small_cfg()
    args = _targs(2)
    bs = _clean_batches(cfg, 4, seed=20)
    streams.enable(False)
    ops.Rng.manual_seed(7); ops.Rng.device_counter().zero_()
    model, guide, _ = build_models(cfg, G._vcfg(), init="synthetic", seed=0)
    opt = _opt(model, 2)
    train_step(model, guide, opt, bs[0], args)
    with pytest.raises(RuntimeError, match="middle of an accumulation group: 1 of 2"):
        checkpoint.save_checkpoint(io.BytesIO(), model, opt, step=1)
    train_step(model, guide, opt, bs[1], args)
    buf = io.BytesIO()
    ck = checkpoint.save_checkpoint(buf, model, opt, step=2)
    assert ck["schedule"]["accum_steps"] == 2 and ck["optimizer"]["groups"] == 1 and ck["optimizer"]["step"] == 1
    assert ck["meta"]["step"] == 2, "meta.step stays the data position"
    want = [train_step(model, guide, opt, b, args).tolist() for b in bs[2:]]
    model2, _, _ = build_models(cfg, G._vcfg(), init="synthetic", seed=5)
    model2.clip_model = model.clip_model
    buf.seek(0)
    with pytest.raises(ValueError, match=r"accum_steps=2.*accum_steps=3"):
        checkpoint.load_checkpoint(buf, model2, _opt(model2, 3))
    opt2 = _opt(model2, 2)
    buf.seek(0)
    assert checkpoint.load_checkpoint(buf, model2, opt2)["step"] == 2 and opt2.hyper[1].item() == 1.0
    assert opt2.accum.tolist() == [0, 0, 1, 0]
    got = [train_step(model2, guide, opt2, b, args).tolist() for b in bs[2:]]
    assert np.isfinite(want).all()
    np.testing.assert_allclose(np.array(got), np.array(want), rtol=2e-4, atol=1e-5)
    assert opt2.accum_report() == {"accum_steps": 2, "pending": 0, "groups": 2} and opt2.hyper[1].item() == 2.0


def test_trainer_uses_whole_groups_of_an_epoch_and_writes_a_checkpoint_that_loads(tmp_path, capsys):
    from vacnic_amd import checkpoint, streams, synthetic
    from vacnic_amd.training import FusedAdamW, build_models
    spec = importlib.util.spec_from_file_location(
        "trainer_accum_test", os.path.join(ROOT, "train_mmbart_enc_self_face_name_ids_retrieve_crossattn_bart_guide_match.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parser.parse_args(["--plm_type", "facebook/bart-base", "--clip_type", "ViT-B/32", "--enc_fusion_layer", "0", "1",
                                  "--dim_common", "768", "--train_batch_size", "2", "--article_max_length", "64", "--steps_per_epoch", "5",
                                  "--log_every", "1", "--out_dir", str(tmp_path), "--experiment_name", "t",
                                  "--grad_accum_steps", "2"])
    cfg, vcfg = mod.build_config(args)
    batches = [synthetic.make_batch(cfg, 2, S=64, T=12, seed=90, step=i) for i in range(5)]
    try:
        hist = mod.run(args, batches)                        # batch 1 eager, batch 2 recorded into a plan, 3 and 4 replayed
    finally:
        streams.enable(False)
        torch.cuda.synchronize()
    assert [r["step"] for r in hist] == [1, 2, 3, 4], "5 batches per epoch, k = 2: four are consumed"
    assert [r["optimizer_step"] for r in hist] == [0, 1, 1, 2]
    assert np.isfinite([r["loss"] for r in hist]).all()
    assert '"used": 4' in capsys.readouterr().out, "the truncation is logged"
    ck = torch.load(os.path.join(str(tmp_path), "tlast.pt"), map_location="cpu", weights_only=False)
    assert ck["meta"]["step"] == 4 and ck["optimizer"]["step"] == 2 and ck["optimizer"]["groups"] == 2
    assert ck["schedule"]["accum_steps"] == 2 and ck["schedule"]["num_training_steps"] == 2.0
    model, _, _ = build_models(cfg, vcfg, init="device", seed=1, with_guide=False)
    opt = FusedAdamW(model.arena, lr=args.lr_bart, num_training_steps=2, accum_steps=2)
    assert checkpoint.load_checkpoint(ck, model, opt)["step"] == 4
    assert opt.hyper[1].item() == 2.0 and opt.accum_report() == {"accum_steps": 2, "pending": 0, "groups": 2}
