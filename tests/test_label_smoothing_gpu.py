"""Label smoothing on the MI355X: the fused LM-head cross entropy, the materialised pair, the autograd Function, the model's
`labels=` path and the planned train step against torch's own `F.cross_entropy(..., label_smoothing=eps)`:

    row_loss = (1 - eps) (lse - z_t) + eps (lse - mean_j z_j),   dz_j = (softmax_j - (1 - eps) [j == t] - eps / V) g / count

Targets are chosen so that the smoothed and the plain loss differ (with uniformly random targets they agree in expectation): half
of the rows aim at the arg-max logit.  eps == 0 must be the path without the option, bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOSS_RTOL = 2e-3            # the gate of the existing fused / materialised cross-entropy tests
CASES = [(64, 1000, 128, 0.3), (300, 50267, 256, 0.1)]      # (R, V, d, eps)
CH = 16384                  # ops.LMHEAD_CHUNK


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


def sensitive_targets(logits, V, seed):
    """random ids; every second row aims at its arg-max logit (there the smoothed loss differs most from the plain one); then the
    pattern of the existing tests: every 7th row ignored, the last and the first vocabulary entry."""
    R = logits.shape[0]
    tgt = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(seed)).cuda()
    tgt[::2] = logits[::2, :V].float().argmax(-1)
    tgt[::7] = 1; tgt[5] = V - 1; tgt[6] = 0
    return tgt


def assert_sensitive(logits, tgt, eps):
    """torch's smoothed and plain losses must be at least 10x the loss tolerance apart, or the loss checks show nothing."""
    sm = F.cross_entropy(logits, tgt, ignore_index=1, label_smoothing=eps).item()
    pl = F.cross_entropy(logits, tgt, ignore_index=1).item()
    print(f"torch loss: smoothed {sm:.6f} plain {pl:.6f} rel diff {abs(sm - pl) / abs(sm):.4f}")
    assert abs(sm - pl) >= 10 * LOSS_RTOL * abs(sm), (sm, pl)


_FUSED = {}


def fused_case(R, V, d, eps, with_bias=False):
    """inputs built as in test_lmhead_ce_fused_matches_materialised_logits (the padded rows of E are zero) + torch's references,
    computed once per case and left unchanged."""
    key = (R, V, d, eps, with_bias)
    if key not in _FUSED:
        Vp = (V + 31) // 32 * 32
        h = rnd(R, d, scale=1.0, seed=1)
        E = torch.zeros(Vp, d, device="cuda", dtype=torch.bfloat16)
        E[:V] = rnd(V, d, scale=0.08, seed=2)
        bias = (rnd(V, scale=0.5, dtype=torch.float32, seed=5) + 0.7) if with_bias else None     # non-zero mean: it must reach mean_j z_j
        hf = h.float().requires_grad_(True); Ef = E[:V].float().requires_grad_(True)
        logits = hf @ Ef.t()
        if bias is not None:
            logits = logits + bias
        tgt = sensitive_targets(logits.detach(), V, seed=3)
        assert_sensitive(logits.detach(), tgt, eps)
        ref = F.cross_entropy(logits, tgt, ignore_index=1, label_smoothing=eps)
        ref.backward()
        valid = (tgt != 1).float()
        want = (torch.softmax(logits.detach(), -1) - (1.0 - eps) * F.one_hot(tgt, V).float() - eps / V) * valid[:, None]    # g = 1 per row
        _FUSED[key] = dict(h=h, E=E, bias=bias, tgt=tgt, logits=logits.detach(), ref=ref.item(), want=want, dh=hf.grad, dE=Ef.grad, Vp=Vp)
    return _FUSED[key]


@pytest.mark.parametrize("R,V,d,eps,with_bias", [c + (False,) for c in CASES] + [CASES[0] + (True,)])
def test_fused_kernels_match_torch_label_smoothing(K, R, V, d, eps, with_bias):
    c = fused_case(R, V, d, eps, with_bias)
    h, E, tgt, bias = c["h"], c["E"], c["tgt"], c["bias"]
    lse0, _ = K.lmhead_ce_fwd(h, E, tgt, V, ignore_index=1, bias=bias)
    lse, acc = K.lmhead_ce_fwd(h, E, tgt, V, ignore_index=1, label_smoothing=eps, bias=bias)
    assert torch.equal(lse, lse0), "row_lse must not depend on label_smoothing"
    close(lse, torch.logsumexp(c["logits"], -1), 1e-4, 2e-3, "row lse")
    count = (tgt != 1).sum().item()
    assert acc[1].item() == count
    got = (acc[0] / acc[1]).item()
    print(f"fused loss {got:.6f} torch {c['ref']:.6f} rel err {abs(got - c['ref']) / abs(c['ref']):.3e}")
    assert abs(got - c["ref"]) <= LOSS_RTOL * abs(c["ref"]), (got, c["ref"])
    # dlogits, chunk by chunk, with grad_scale = count so that g = 1 per row.  rtol: the existing bf16 gate; atol at most a quarter
    # of the uniform term eps / V, so that the term shows (the existing 2e-6 would hide it at V = 50267)
    rowp = K.lmhead_ce_rowp(lse, tgt, acc, grad_out=None, grad_scale=float(count), ignore_index=1, label_smoothing=eps, V=V)
    assert rowp.shape == (R, 4)
    atol = 0.25 * eps / V
    dl = torch.full((R, CH), 9.0, device="cuda", dtype=torch.bfloat16)
    rows = torch.arange(R, device="cuda")
    for c0 in range(0, V, CH):
        n = min(CH, V - c0); n8 = (n + 7) // 8 * 8
        K.lmhead_ce_dlogits(h, E, tgt, V, rowp, dl, c0, n, ignore_index=1, label_smoothing=eps, bias=bias)
        err = (dl[:, :n].float() - c["want"][:, c0:c0 + n]).abs()
        print(f"dlogits chunk at {c0}: max abs err {err.max().item():.3e} (atol {atol:.3e}, eps/V {eps / V:.3e})")
        close(dl[:, :n], c["want"][:, c0:c0 + n], 2e-2, atol, f"dlogits chunk at {c0}")
        assert (dl[:, n:n8] == 0).all(), "pad columns of a ragged chunk must be zeros"
        # the (1 - eps) weight on its own: target columns of valid rows inside this chunk
        sel = (tgt >= c0) & (tgt < c0 + n) & (tgt != 1)
        if sel.any():
            gt = dl[rows[sel], tgt[sel] - c0].float()
            wt = c["want"][rows[sel], tgt[sel]]
            close(gt, wt, 2e-2, atol, f"target columns of chunk at {c0}")
            assert (gt < 0).all() and (gt > -(1.0 - eps) * (1 + 2e-2)).all(), "a target column lies in (-(1 - eps), 0): the one-hot weight is 1 - eps"
    ign = tgt == 1
    K.lmhead_ce_dlogits(h, E, tgt, V, rowp, dl, 0, min(CH, V), ignore_index=1, label_smoothing=eps, bias=bias)
    assert (dl[ign, :min(CH, V)] == 0).all(), "ignored rows carry no gradient, the uniform term included"


@pytest.mark.parametrize("R,V,d,eps", CASES)
def test_zero_label_smoothing_is_the_existing_path_bit_for_bit(K, R, V, d, eps):
    """label_smoothing=0.0 against the same call without the argument: row_lse, the count, rowp and dlogits are torch.equal.
    loss_sum (acc[0]) is an fp32 atomic accumulation over the rows whose order varies from launch to launch — two identical calls
    WITHOUT the argument already differ in its last bits (measured at R = 300: 2963.27173 vs 2963.27026) — so it is compared
    within the reordering bound of a sum of R positive fp32 terms, R * 2^-24 relative."""
    def same_acc(a, b):
        return a[1].item() == b[1].item() and abs(a[0].item() - b[0].item()) <= R * 2.0 ** -24 * abs(a[0].item())
    c = fused_case(R, V, d, eps)
    h, E, tgt = c["h"], c["E"], c["tgt"]
    tiles = (V + 255) // 256
    garbage = torch.full((R, tiles), float("nan"), device="cuda")
    K.lmhead_ce_fwd(h, E, tgt, V, ignore_index=1, label_smoothing=eps, part_sum=garbage)       # the eps > 0 path used this scratch ...
    garbage.fill_(float("nan"))                                                                # ... and it holds garbage again
    lse_a, acc_a = K.lmhead_ce_fwd(h, E, tgt, V, ignore_index=1)
    lse_b, acc_b = K.lmhead_ce_fwd(h, E, tgt, V, ignore_index=1, label_smoothing=0.0, part_sum=garbage)
    assert torch.equal(lse_a, lse_b) and same_acc(acc_a, acc_b), (acc_a.tolist(), acc_b.tolist())
    assert torch.isnan(garbage).all(), "label_smoothing == 0 must not touch part_sum"
    rp_a = K.lmhead_ce_rowp(lse_a, tgt, acc_a, ignore_index=1)
    rp_b = K.lmhead_ce_rowp(lse_b, tgt, acc_b, ignore_index=1, label_smoothing=0.0, V=V)
    assert rp_b.shape == (R, 2) and torch.equal(rp_a, rp_b)
    n = min(CH, V)
    dl_a = torch.full((R, CH), 9.0, device="cuda", dtype=torch.bfloat16); dl_b = dl_a.clone()
    K.lmhead_ce_dlogits(h, E, tgt, V, rp_a, dl_a, 0, n, ignore_index=1)
    K.lmhead_ce_dlogits(h, E, tgt, V, rp_b, dl_b, 0, n, ignore_index=1, label_smoothing=0.0)
    assert torch.equal(dl_a, dl_b)
    # the materialised pair on the same logits
    lg = c["logits"].to(torch.bfloat16) if V % 8 == 0 else F.pad(c["logits"], (0, (-V) % 8)).to(torch.bfloat16)
    for logits in (lg, lg.float()):
        l_a, a_a = K.ce_fwd(logits, tgt, V, ignore_index=1)
        l_b, a_b = K.ce_fwd(logits, tgt, V, ignore_index=1, label_smoothing=0.0)
        assert torch.equal(l_a, l_b) and same_acc(a_a, a_b), (a_a.tolist(), a_b.tolist())
        d_a = torch.empty(R, lg.shape[1], device="cuda", dtype=torch.bfloat16); d_b = torch.empty_like(d_a)
        K.ce_bwd(logits, tgt, V, l_a, a_a, d_a)
        K.ce_bwd(logits, tgt, V, l_b, a_b, d_b, label_smoothing=0.0)
        assert torch.equal(d_a, d_b)


@pytest.mark.parametrize("R,V,d,eps", CASES)
def test_autograd_function_with_label_smoothing(K, R, V, d, eps):
    """ops.lm_head_ce(label_smoothing=eps): loss, dh and dE against torch autograd on fp32 logits (the tolerances of the existing
    fused test)."""
    from vacnic_amd import ops
    c = fused_case(R, V, d, eps)
    egrad = torch.zeros(c["Vp"], d, device="cuda")
    hh = c["h"].clone().requires_grad_(True)
    anchor = torch.zeros(1, device="cuda", requires_grad=True)
    loss, _ = ops.lm_head_ce(hh, anchor, c["E"], egrad, c["tgt"], V, 1, label_smoothing=eps)
    assert abs(loss.item() - c["ref"]) <= LOSS_RTOL * abs(c["ref"]), (loss.item(), c["ref"])
    loss.backward()
    close(hh.grad, c["dh"], 3e-2, 2e-2 * c["dh"].abs().max().item(), "dh")
    close(egrad[:V], c["dE"], 3e-2, 2e-2 * c["dE"].abs().max().item(), "dE")
    assert (egrad[V:] == 0).all()


@pytest.mark.parametrize("f32", [False, True])
def test_materialised_pair_with_label_smoothing(K, f32):
    """the test_cross_entropy construction (pad columns at 100.0 must stay ignored) with eps = 0.1 and sensitive targets."""
    R, V, ld, eps = 50, 50267, 50272, 0.1
    logits = torch.zeros(R, ld, device="cuda", dtype=torch.float32 if f32 else torch.bfloat16)
    logits[:, :V] = rnd(R, V, scale=2.0, seed=1).to(logits.dtype)
    logits[:, V:] = 100.0
    tgt = sensitive_targets(logits, V, seed=2)
    lf = logits[:, :V].float().requires_grad_(True)
    assert_sensitive(lf.detach(), tgt, eps)
    ref = F.cross_entropy(lf, tgt, ignore_index=1, label_smoothing=eps)
    ref.backward()
    lse, acc = K.ce_fwd(logits, tgt, V, ignore_index=1, label_smoothing=eps)
    count = (tgt != 1).sum().item()
    got = (acc[0] / acc[1]).item()
    print(f"materialised loss {got:.6f} torch {ref.item():.6f}")
    assert abs(got - ref.item()) < LOSS_RTOL * abs(ref.item()), (got, ref.item())
    assert acc[1].item() == count
    dl = torch.empty(R, ld, device="cuda", dtype=torch.bfloat16)
    K.ce_bwd(logits, tgt, V, lse, acc, dl, grad_scale=float(count), label_smoothing=eps)       # g = 1 per row
    err = (dl[:, :V].float() - lf.grad * count).abs()
    print(f"materialised dlogits max abs err {err.max().item():.3e} (atol {0.25 * eps / V:.3e})")
    close(dl[:, :V], lf.grad * count, 2e-2, 0.25 * eps / V, "dlogits")
    assert (dl[:, V:] == 0).all()


@pytest.mark.parametrize("eps", [1.0, -0.1])
def test_label_smoothing_outside_0_1_is_a_value_error(K, eps):
    c = fused_case(*CASES[0])
    R, V = CASES[0][0], CASES[0][1]
    h, E, tgt = c["h"], c["E"], c["tgt"]
    lse, acc = K.lmhead_ce_fwd(h, E, tgt, V, ignore_index=1)
    with pytest.raises(ValueError, match="label_smoothing"):
        K.lmhead_ce_fwd(h, E, tgt, V, ignore_index=1, label_smoothing=eps)
    with pytest.raises(ValueError, match="label_smoothing"):
        K.lmhead_ce_rowp(lse, tgt, acc, ignore_index=1, label_smoothing=eps, V=V)
    rowp = K.lmhead_ce_rowp(lse, tgt, acc, ignore_index=1)
    dl = torch.full((R, CH), 9.0, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="label_smoothing"):
        K.lmhead_ce_dlogits(h, E, tgt, V, rowp, dl, 0, V, ignore_index=1, label_smoothing=eps)
    assert (dl == 9.0).all(), "a rejected call launches nothing"
    lg = F.pad(c["logits"], (0, (-V) % 8)).to(torch.bfloat16)
    with pytest.raises(ValueError, match="label_smoothing"):
        K.ce_fwd(lg, tgt, V, ignore_index=1, label_smoothing=eps)
    l2, a2 = K.ce_fwd(lg, tgt, V, ignore_index=1)
    d2 = torch.full((R, lg.shape[1]), 9.0, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="label_smoothing"):
        K.ce_bwd(lg, tgt, V, l2, a2, d2, label_smoothing=eps)
    assert (d2 == 9.0).all()
    from vacnic_amd.config import VacnicConfig
    with pytest.raises(ValueError, match="label_smoothing"):
        VacnicConfig(label_smoothing=eps).validate()


# ---------------------------------------------------------------------------------------------- model level
def small_cfg(**kw):
    from vacnic_amd.config import VacnicConfig
    base = dict(d_model=768, encoder_layers=1, decoder_layers=1, encoder_attention_heads=12, decoder_attention_heads=12,
                encoder_ffn_dim=3072, decoder_ffn_dim=3072, enc_fusion_layer=[0], dim_common=768, clip_width=768, dropout=0.0)
    base.update(kw)
    return VacnicConfig(**base)


def _vcfg():
    from vacnic_amd.config import ClipVisionConfig
    return ClipVisionConfig(width=768, layers=1, patch_size=16, image_size=32, output_dim=64)


def _self_captioned(model, batch):
    """the batch with the model's own greedy caption as its target: every target is then (close to) the arg-max logit of its row, so
    z_t - mean_j z_j > 0 everywhere and the smoothed loss lies measurably ABOVE the plain one (synthetic captions are random ids:
    there the two agree in expectation)."""
    from vacnic_amd.training import _model_inputs
    src, src_mask, feats, kw = _model_inputs(model, batch)
    T = batch["caption_ids"].shape[1]
    was = model.training
    model.eval()
    ids = model.greedy_generate(src, src_mask, T + 1, image_features=feats, **kw)
    model.train(was)
    return dict(batch, caption_ids=ids[:, 1:].contiguous())


def test_model_forward_label_smoothing_kwarg_and_config_default():
    from vacnic_amd import synthetic
    from vacnic_amd.training import _model_inputs, build_models, to_device
    losses = {}
    cfg = small_cfg()
    model, _, _ = build_models(cfg, _vcfg(), init="synthetic", seed=0, with_guide=False)
    model.eval()
    batch = _self_captioned(model, to_device(synthetic.make_batch(cfg, 3, S=32, T=12, F=3, seed=40, image_size=32), "cuda"))
    src, src_mask, feats, kw = _model_inputs(model, batch)
    tgt = batch["caption_ids"]
    for name, cfg_eps, kw_eps in (("kwarg", 0.0, 0.1), ("config", 0.1, None), ("plain", 0.0, None)):
        model.config.label_smoothing = cfg_eps                # read at every forward: the default of label_smoothing=None
        with torch.no_grad():
            out = model(input_ids=src, attention_mask=src_mask, image_features=feats, labels=tgt, output_logits=True,
                        **({} if kw_eps is None else {"label_smoothing": kw_eps}), **kw)
        losses[name] = out["loss"].item()
        if name == "kwarg":
            lg = out["logits"].float()[..., :model.V].reshape(-1, model.V)
            ref = F.cross_entropy(lg, tgt.reshape(-1), ignore_index=cfg.pad_token_id, label_smoothing=0.1).item()
            plain = F.cross_entropy(lg, tgt.reshape(-1), ignore_index=cfg.pad_token_id).item()
    print(f"model losses {losses}; torch on the model's logits: smoothed {ref:.6f} plain {plain:.6f}")
    assert abs(losses["kwarg"] - ref) <= 1e-2 * abs(ref), (losses["kwarg"], ref)          # the project's bf16 model gate
    # the same launches; loss_sum is an fp32 atomic sum over the rows whose order varies: equal within rows * 2^-24 relative
    assert abs(losses["config"] - losses["kwarg"]) <= tgt.numel() * 2.0 ** -24 * abs(losses["kwarg"]), \
        "config.label_smoothing is the default of forward(label_smoothing=None)"
    assert losses["plain"] < losses["kwarg"] - 1e-2 * abs(ref), "with label_smoothing = 0.0 in config and no kwarg the loss is the plain one"
    # same weights, same targets: smoothed - plain = eps * mean(z_t - mean_j z_j), which torch gives from the model's own (bf16)
    # logits; 2e-2 relative = the bf16 gate on that difference
    assert ref - plain > 0
    assert abs((losses["kwarg"] - losses["plain"]) - (ref - plain)) <= 2e-2 * (ref - plain), (losses, ref, plain)


def test_planned_steps_with_label_smoothing_replay_like_eager():
    """three planned steps with config.label_smoothing = 0.1 against three eager steps (the comparison of
    test_planned_step_replays_like_eager), and the first step's text loss against an eps = 0 run from the same weights."""
    from vacnic_amd import ops, streams, synthetic
    from vacnic_amd.training import FusedAdamW, PlannedTrainStep, TrainArgs, build_models, forward_losses, to_device, train_step
    eps = 0.1
    cfg = small_cfg(label_smoothing=eps)
    vcfg = _vcfg()
    args = TrainArgs(num_training_steps=20, warmup_rate=0.1, lr_bart=1e-4)
    batches = [to_device(synthetic.make_batch(cfg, 3, S=32, T=12, F=3, seed=40 + i, image_size=32), "cuda") for i in range(3)]
    streams.enable(True)
    try:
        runs, weights, first = [], [], {}
        for planned in (False, True):
            ops.Rng.manual_seed(3); ops.Rng.device_counter().zero_()
            model, guide, _ = build_models(cfg, vcfg, init="synthetic", seed=0)
            opt = FusedAdamW(model.arena, lr=args.lr_bart, weight_decay=args.weight_decay, num_warmup_steps=2, num_training_steps=20)
            if not planned:
                batches[0] = _self_captioned(model, batches[0])       # (from the initial weights, before the first step)
            if planned:
                step = PlannedTrainStep(model, guide, opt, args, batches[0], warmup=2)
                losses = [step(b).tolist() for b in batches[1:] + batches[:1]]
                step.close()
            else:
                # eps = 0 from the same weights: the step's own forward on the same batch with the config switched, nothing updated
                model.config.label_smoothing = 0.0
                with torch.no_grad():
                    first[0.0] = forward_losses(model, guide, batches[0], args)[1].tolist()
                model.config.label_smoothing = eps
                first[eps] = train_step(model, guide, opt, batches[0], args).tolist()
                for _ in range(2):
                    train_step(model, guide, opt, batches[0], args)
                losses = [train_step(model, guide, opt, b, args).tolist() for b in batches[1:] + batches[:1]]
            torch.cuda.synchronize()
            runs.append(np.array(losses))
            weights.append(model.arena.flat32.clone())
        assert np.isfinite(runs[1]).all()
        np.testing.assert_allclose(runs[1], runs[0], rtol=2e-3, atol=1e-4)
        rel = ((weights[1] - weights[0]).norm() / weights[0].norm()).item()
        assert rel < 1e-4, rel
        txt_s, txt_p = first[eps][1], first[0.0][1]
        print(f"step 1 text loss: eps=0.1 {txt_s:.6f}, eps=0 {txt_p:.6f}")
        # the targets of batches[0] are the model's own arg-max tokens, so z_t - mean_j z_j > 0 in every row and the smoothed loss
        # exceeds the plain one by eps times its mean; fp32 losses of ~10 resolve 1e-6, "measurably" = 100x that
        assert txt_s - txt_p > 1e-4, (txt_s, txt_p)
        np.testing.assert_allclose(first[eps][2:], first[0.0][2:], rtol=1e-5, err_msg="label smoothing touches the text loss only")
    finally:
        streams.enable(False)
