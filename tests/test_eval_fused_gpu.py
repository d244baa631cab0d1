"""The fused validation head at model level on the MI355X: model(..., output_token_stats=True), model.score,
training.eval_epoch_fused / score_captions against eval_epoch (the path with materialised bf16 logits, unchanged) and against
float64 on the CPU from the model's own last decoder state.  Small model configuration of tests/test_model_gpu.py, three
synthetic batches; margins of tests/test_lmhead_eval.py."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_loss_gpu import F32, F64, FUSED_NFAC, check, host, span_of          # noqa: E402
from test_model_gpu import small_cfg                                          # noqa: E402

_STATE = {}


def setup():
    """one model and three host batches for the whole module.  A randomly initialised model predicts none of a random caption's
    tokens, so the captions are the model's own teacher-forced predictions for random captions (pad positions kept): some of them
    it predicts again, and token accuracy is not a comparison of zeros."""
    if not _STATE:
        from vacnic_amd import ops, streams, synthetic
        from vacnic_amd.config import ClipVisionConfig
        from vacnic_amd.training import build_models
        streams.enable(False)
        ops.Rng.manual_seed(3)
        cfg = small_cfg()
        vcfg = ClipVisionConfig(width=768, layers=1, patch_size=16, image_size=32, output_dim=64)       # width = cfg.clip_width
        model, _, _ = build_models(cfg, vcfg, init="synthetic", seed=0)
        model.train()
        from vacnic_amd.training import eval_epoch_fused
        batches = [synthetic.make_batch(cfg, 3, S=32, T=12, F=3, seed=60 + i, image_size=32) for i in range(3)]
        _, first, _ = eval_epoch_fused(model, batches)
        for step, b in enumerate(batches):
            keep = b["caption_ids"] != cfg.pad_token_id
            b["caption_ids"] = torch.where(keep, torch.tensor(first[step]["logit_output"]), b["caption_ids"])
        _STATE.update(cfg=cfg, model=model, batches=batches)
    return _STATE["cfg"], _STATE["model"], _STATE["batches"]


def bf16_ulp(x):
    return 2.0 ** (math.floor(math.log2(abs(x))) - 7) if x != 0 else 0.0


def test_eval_epoch_fused_matches_eval_epoch():
    from vacnic_amd import kernels as K
    from vacnic_amd.training import _model_inputs, eval_epoch, eval_epoch_fused, score_captions, to_device
    cfg, model, batches = setup()
    want_loss, want = eval_epoch(model, batches)
    loss, got, metrics = eval_epoch_fused(model, batches)
    assert model.training, "the mode is restored"
    print(f"EVALCHK val_loss fused={loss!r} eval_epoch={want_loss!r} rel={abs(loss - want_loss) / abs(want_loss):.3e}")
    assert abs(loss - want_loss) <= 1e-6 * abs(want_loss)
    assert sorted(got) == sorted(want) == [0, 1, 2]
    total = differ = tokens = correct = 0
    model.eval()
    for step, batch in enumerate(batches):
        assert got[step]["gt_cap"] == want[step]["gt_cap"] == batch["caption_ids"].tolist()
        a, b = torch.tensor(got[step]["logit_output"]), torch.tensor(want[step]["logit_output"])
        tgt = batch["caption_ids"]
        assert a.shape == b.shape == tgt.shape
        total += a.numel()
        bad = (a != b).nonzero().tolist()
        differ += len(bad)
        if bad:                           # the old path rounds the logits to bf16 before its argmax: only such near-ties may differ
            dev = to_device(batch, "cuda")
            src, src_mask, feats, kw = _model_inputs(model, dev)
            _, tgt_in = K.prep_ids(dev["caption_ids"], cfg.pad_token_id, start_id=cfg.eos_token_id)
            with torch.no_grad():
                lg = model(input_ids=src, attention_mask=src_mask, decoder_input_ids=tgt_in, image_features=feats, add_ner_ffn=True,
                           **kw)["logits"].float().cpu()
            for i, j in bad:
                x, y = lg[i, j, a[i, j]].item(), lg[i, j, b[i, j]].item()
                print(f"EVALCHK step {step} position ({i}, {j}): fused id {a[i, j]} logit {x}, materialised id {b[i, j]} logit {y}")
                assert abs(x - y) <= bf16_ulp(max(abs(x), abs(y)))
        keep = tgt != cfg.pad_token_id
        tokens += int(keep.sum())
        correct += int(((a == tgt) & keep).sum())
    model.train()
    print(f"EVALCHK predicted ids: {differ}/{total} positions differ; tokens={tokens} correct={correct} metrics={ {k: v for k, v in metrics.items() if k != 'seq_logprob'} }")
    assert differ <= 0.01 * total
    assert 0 < correct < tokens, "the accuracy check compares something"
    assert metrics["tokens"] == tokens and metrics["sequences"] == 9 and metrics["token_accuracy"] == correct / tokens
    assert len(metrics["seq_logprob"]) == 9 and all(v < 0 for v in metrics["seq_logprob"])
    nll = -sum(metrics["seq_logprob"])
    assert abs(metrics["perplexity"] - math.exp(nll / tokens)) <= 1e-5 * metrics["perplexity"]
    sc = score_captions(model, batches)
    assert sc["logprob"] == metrics["seq_logprob"] and sum(sc["tokens"]) == tokens and sum(sc["correct"]) == correct
    assert [len(v) for v in sc.values()] == [9, 9, 9]


def test_score_matches_float64_from_the_models_last_state():
    from vacnic_amd import kernels as K
    from vacnic_amd.training import _model_inputs, to_device
    cfg, model, batches = setup()
    dev = to_device(batches[1], "cuda")
    src, src_mask, feats, kw = _model_inputs(model, dev)
    tgt = dev["caption_ids"]
    _, tgt_in = K.prep_ids(tgt, cfg.pad_token_id, start_id=cfg.eos_token_id)
    inputs = dict(input_ids=src, attention_mask=src_mask, decoder_input_ids=tgt_in, image_features=feats, add_ner_ffn=True, **kw)
    stats = model.score(labels=tgt, **inputs)
    assert model.training, "score() restores the mode"
    model.eval()
    with torch.no_grad():
        out = model(labels=tgt, output_token_stats=True, **inputs)
        plain = model(labels=tgt, output_logits=False, label_smoothing=0.0, **inputs)
    model.train()
    for k, v in out["token_stats"].items():
        assert torch.equal(v, stats[k]), f"score() and forward(output_token_stats=True) differ in {k}"
    assert "logits" not in out and "token_stats" not in plain
    B, T = tgt.shape
    V = model.V
    h = host(out["decoder_hidden_states"][-1]).reshape(B * T, -1)
    E = host(model.emb16_pad)[:V]
    t = host(tgt).reshape(-1)
    pad = t == cfg.pad_token_id

    def logprobs(dt):
        z = h.to(dt) @ E.to(dt).t()
        lp = z.gather(1, t[:, None])[:, 0] - torch.logsumexp(z, -1)
        return torch.where(pad, torch.zeros_like(lp), lp), z
    lp64, z64 = logprobs(F64)
    lp32, _ = logprobs(F32)
    S, lmax = span_of(z64)
    check("score token_logprobs", stats["token_logprobs"].reshape(-1), lp64, lp32, extra=2.0 ** -23 * (S + FUSED_NFAC) + 2.0 ** -22 * lmax)
    tl = host(stats["token_logprobs"])
    assert pad.any() and (tl.reshape(-1)[pad] == 0).all(), "pad positions are 0"
    seq = host(stats["seq_logprob"]).to(F64)
    err = (seq - tl.to(F64).sum(1)).abs().max().item()
    print(f"EVALCHK seq_logprob vs the sum of its token_logprobs: err={err:.3e}")
    assert err <= T * 2.0 ** -23 * seq.abs().max().item()
    assert torch.equal(host(stats["seq_tokens"]).long(), (~pad).view(B, T).sum(1))
    pred = host(stats["pred_ids"])
    assert stats["pred_ids"].dtype == torch.int64 and pred.shape == (B, T) and ((pred >= 0) & (pred < V)).all()
    assert torch.equal(host(stats["seq_correct"]).long(), ((pred.reshape(-1) == t) & ~pad).view(B, T).sum(1))
    # the loss of the pass is the loss of the fused training head (same row_lse, no label smoothing)
    a, b = out["loss"].item(), plain["loss"].item()
    assert abs(a - b) <= 1e-6 * abs(b), (a, b)
    assert abs(a + host(stats["seq_logprob"]).to(F64).sum().item() / int((~pad).sum())) <= 1e-6 * abs(a)


def test_token_stats_refusals_and_default_keys():
    from vacnic_amd import kernels as K
    from vacnic_amd.training import _model_inputs, to_device
    cfg, model, batches = setup()
    dev = to_device(batches[0], "cuda")
    src, src_mask, feats, kw = _model_inputs(model, dev)
    tgt = dev["caption_ids"]
    inputs = dict(input_ids=src, attention_mask=src_mask, image_features=feats, add_ner_ffn=True, **kw)
    with pytest.raises(ValueError, match="no_grad"):
        model(labels=tgt, output_token_stats=True, **inputs)
    with torch.no_grad():
        with pytest.raises(ValueError, match="output_logits"):
            model(labels=tgt, output_token_stats=True, output_logits=True, **inputs)
        with pytest.raises(ValueError, match="labels"):
            model(output_token_stats=True, **inputs)
        want_keys = {"loss", "loss_acc", "decoder_hidden_states", "encoder_last_hidden_state", "hidden_states_img", "hidden_states_ner",
                     "hidden_states_face"}
        for flag in ({}, {"output_token_stats": None}, {"output_token_stats": False}):
            out = model(labels=tgt, **inputs, **flag)
            assert set(out) == want_keys, sorted(out)
        assert "logits" in model(decoder_input_ids=tgt, **inputs)
