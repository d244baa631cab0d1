"""GPU: generate(do_sample=True) end to end — sampling session, hipGraph replay with run-time parameters, seeds, the [B * n, L]
layout, logits processors and log-probs — on a small model (d_model 768, one layer, vocabulary 2048) and, for the top_k = 1 ==
greedy identity, also on the prompts behind tests/golden/generate_small.npz (full vocabulary)."""
import os

import numpy as np
import pytest
import torch

from test_sample import F32, chi2_quantile, host_processors, host_warp

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EOS, PAD, START = 2, 1, 2


def build(vocab, sharpen):
    from vacnic_amd import kernels as K, synthetic
    from vacnic_amd.config import ClipVisionConfig, VacnicConfig
    from vacnic_amd.training import build_models
    cfg = VacnicConfig(d_model=768, encoder_layers=1, decoder_layers=1, encoder_attention_heads=12, decoder_attention_heads=12,
                       encoder_ffn_dim=3072, decoder_ffn_dim=3072, enc_fusion_layer=[0], dim_common=768, clip_width=768, dropout=0.0,
                       vocab_size=vocab)
    vcfg = ClipVisionConfig(width=128, layers=1, patch_size=16, image_size=32, output_dim=64)
    sd = synthetic.make_state_dict(synthetic.mmbart_param_shapes(cfg), seed=1)
    sd["model.shared.weight"] = sd["model.shared.weight"] * sharpen
    model, _, _ = build_models(cfg, vcfg, init="synthetic",
                               state_dicts=(sd, synthetic.make_state_dict(synthetic.guide_bart_param_shapes(cfg), seed=2),
                                            synthetic.make_state_dict(synthetic.clip_visual_param_shapes(vcfg), seed=4, std=0.05)))
    model.eval()

    def inputs(B):
        """generate() keywords of B synthetic captions (the batch of the generate_small golden for B = 2, full vocabulary)"""
        batch = synthetic.make_batch(cfg, B, S=24, T=8, F=2, seed=9, image_size=32)
        if vocab < 50265:
            for name in ("article_ids", "names_art_ids"):
                ids = batch[name]
                batch[name] = torch.where(ids >= 3, 3 + ids % (vocab - 3), ids)
        dev = {k: v.cuda() for k, v in batch.items()}
        mask, _ = K.prep_ids(dev["article_ids"], 1)
        nmask, _ = K.prep_ids(dev["names_art_ids"], 1)
        return dict(input_ids=dev["article_ids"], attention_mask=mask, image_features=synthetic._normal("img_cls", (B, 768), 1.0, 3).cuda(),
                    face_features=dev["face_emb"], face_mask=K.face_mask(dev["face_emb"]), name_ids=dev["names_art_ids"], name_mask=nmask,
                    add_ner_ffn=True)
    return model, inputs


@pytest.fixture(scope="module")
def small():
    """random-init scale: the logits of a position are close to normal(0, 0.55) over the 2048 tokens, so sampling has something to
    choose from (with the tied matrix scaled by synthetic.GEN_SHARPEN every position is all but certain: eos first, then repeats)"""
    return build(2048, 1.0)


def rows_are_well_formed(ids, max_length):
    ids = ids.cpu().numpy()
    assert ids.shape[1] <= max_length and (ids[:, 0] == START).all()
    ends = []
    for row in ids:
        (where,) = np.nonzero(row[1:] == EOS)
        assert len(where) >= 1, row
        e = int(where[0]) + 1
        assert (row[e + 1:] == PAD).all(), row
        ends.append(e + 1)
    assert max(ends) == ids.shape[1]                       # L is the longest row
    return ends


@pytest.mark.parametrize("vocab", [2048, 50267])
def test_top_k_1_equals_greedy_eager_and_replayed(vocab, small):
    from vacnic_amd import synthetic
    model, inputs = small if vocab == 2048 else build(vocab, synthetic.GEN_SHARPEN)      # the golden's weights
    # min_length keeps every row alive (both models would otherwise end with eos as their first token), so the identity is
    # checked over many decoded positions: the token fed back, the KV-cache position, eos suppression in replayed graphs and the
    # eos forced at max_length - 1.  The no-repeat cases make the greedy caption change its token from position to position.
    cases = (((2, 1, 8, 0), (1, 1, 11, 0), (3, 4, 10, 0), (3, 4, 9, 2)) if vocab == 2048 else ((2, 1, 4, 0), (2, 1, 4, 2)))
    for B, n, min_length, ngram in cases:
        kw = dict(inputs(B), max_length=12, min_length=min_length, no_repeat_ngram_size=ngram)
        greedy = model.generate(num_beams=1, **kw)
        if vocab != 2048 and ngram == 0:                   # these prompts are the golden's: its greedy-sized case (1 beam, min_length 4)
            assert np.array_equal(greedy.cpu().numpy(), np.load(os.path.join(G, "generate_small.npz"))["seq2"])
        decoded = ((greedy[:, 1:] != PAD) & (greedy[:, 1:] != EOS)).sum(1)
        assert int(decoded.min()) >= min_length - 1 >= 3, greedy.tolist()     # several decoded tokens per row, not eos at once
        if ngram:
            assert all(len(set(row[1:1 + min_length - 1])) > 1 for row in greedy.tolist()), greedy.tolist()
        want = greedy.repeat_interleave(n, dim=0)
        model.__dict__.pop("_sample_sessions", None)
        first = model.generate(do_sample=True, top_k=1, num_return_sequences=n, seed=5, **kw)                                  # eager
        (ses,) = model._sample_sessions.values()
        assert not ses.graphs and torch.equal(first, want), (B, n, first.tolist(), want.tolist())
        other = model.generate(do_sample=True, temperature=1.7, top_p=0.8, num_return_sequences=n, seed=6, **kw)                # captures
        assert ses.graphs and len(model._sample_sessions) == 1 and other.shape[0] == B * n
        third = model.generate(do_sample=True, top_k=1, temperature=0.6, num_return_sequences=n, seed=7, **kw)                  # replays
        assert torch.equal(third, want), (B, n, third.tolist(), want.tolist())
        again = model.generate(do_sample=True, temperature=1.7, top_p=0.8, num_return_sequences=n, seed=6, **kw)
        assert torch.equal(again, other) and (vocab != 2048 or not torch.equal(other, want))
        rows_are_well_formed(first, 12)


def test_seeds_rows_and_layout(small):
    model, inputs = small
    for B, n in ((1, 4), (3, 4), (3, 1)):
        kw = dict(inputs(B), do_sample=True, temperature=1.5, num_return_sequences=n, max_length=10)
        a, la = model.generate(seed=123, return_logprobs=True, **kw)
        b, lb = model.generate(seed=123, return_logprobs=True, **kw)
        c = model.generate(seed=124, **kw)
        assert a.dtype == torch.int64 and la.dtype == torch.float32 and a.shape == la.shape and a.shape[0] == B * n
        assert torch.equal(a, b) and torch.equal(la, lb)
        assert a.shape != c.shape or not torch.equal(a, c)
        ends = rows_are_well_formed(a, 10)
        la = la.cpu().numpy()
        for r, e in enumerate(ends):
            assert la[r, 0] == 0 and (la[r, e:] == 0).all() and (la[r, 1:e] <= 0).all()
        if n == 4:
            for item in range(B):                          # the samples of one item differ among themselves
                assert len({tuple(row) for row in a[item * n:(item + 1) * n].tolist()}) > 1
    # 64 samples of one item: after the start token (= eos, tied embeddings) eos is the likeliest first token of this model, so at
    # temperature 1.5 some rows end at once (eos, then pad) while others run on to max_length
    ids = model.generate(seed=3, **dict(inputs(1), do_sample=True, temperature=1.5, num_return_sequences=64, max_length=10))
    ends = rows_are_well_formed(ids, 10)
    assert 1 <= sum(e < ids.shape[1] for e in ends) < 64, ends
    # max_length forces eos: with eos suppressed until the end every row is exactly max_length long
    kw = dict(inputs(3), do_sample=True, num_return_sequences=4, max_length=9, min_length=9)
    ids = model.generate(seed=1, **kw)
    assert ids.shape == (12, 9) and (ids[:, -1] == EOS).all() and (ids[:, 1:-1] != EOS).all()
    # seed=None: successive calls differ, and a program that re-seeds torch repeats
    import vacnic_amd.generate as gen
    kw = dict(inputs(1), do_sample=True, temperature=1.5, num_return_sequences=4, max_length=10)
    torch.manual_seed(99)
    calls = gen._SAMPLE_CALLS
    x, y = model.generate(**kw), model.generate(**kw)
    assert x.shape != y.shape or not torch.equal(x, y)
    gen._SAMPLE_CALLS = calls
    torch.manual_seed(99)
    assert torch.equal(model.generate(**kw), x)


def test_first_token_distribution(small):
    """4096 samples of one item: the tokens at position 1 against softmax(z / T) cut at top-p 0.9, z = the decoder's own position-0
    logits (every row sees the same source and start token).  Pearson's chi-square below the 1 - 1e-6 quantile of chi-square(kept - 1)."""
    model, inputs = small
    n, T, p = 4096, 1.3, 0.9
    ids = model.generate(do_sample=True, temperature=T, top_p=p, num_return_sequences=n, max_length=3, seed=31, **inputs(1))
    assert ids.shape == (n, 3)
    ses = [s for s in model._sample_sessions.values() if s.R == n][0]
    start = torch.full((n, 1), START, device="cuda", dtype=torch.long)
    z = ses.dec.step(start, 0)[:, :model.V].float().cpu().numpy()
    assert np.array_equal(z[0], z[n - 1])
    w = host_warp(z[0], T, 0, p)
    counts = np.bincount(ids[:, 1].cpu().numpy(), minlength=model.V)
    assert counts[~w["kept"]].sum() == 0
    exp = w["p"][w["kept"]] * n
    chi2 = float((((counts[w["kept"]] - exp) ** 2) / exp).sum())
    limit = chi2_quantile(int(w["kept"].sum()) - 1)
    print(f"kept {int(w['kept'].sum())} smallest expected count {exp.min():.2f} chi2 {chi2:.1f} limit {limit:.1f}")
    assert chi2 < limit, (chi2, limit)


def bigrams_repeat(row):
    toks = [t for t in row]
    seen = set()
    for a, b in zip(toks, toks[1:]):
        if (a, b) in seen:
            return True
        seen.add((a, b))
    return False


@pytest.mark.parametrize("top_k", [0, 3])
def test_no_repeat_ngram_while_sampling(top_k, small):
    """temperature 2.0, no_repeat_ngram_size 2.  top_k = 0 draws from the whole vocabulary: on the flat logits of `small` a bigram
    would all but never repeat (the precondition could not hold), so this case runs the sharpened model, whose few likely tokens
    come back by themselves.  top_k = 3 keeps `small` inside three tokens per position, where bigrams repeat as well."""
    from vacnic_amd import synthetic
    model, inputs = small if top_k else build(2048, synthetic.GEN_SHARPEN)
    kw = dict(inputs(3), do_sample=True, temperature=2.0, top_k=top_k, num_return_sequences=4, max_length=40, min_length=40, seed=17)
    free = model.generate(no_repeat_ngram_size=0, **kw).tolist()
    print(f"top_k {top_k}: {sum(bigrams_repeat(r) for r in free)} of 12 rows repeat a bigram without the processor")
    assert any(bigrams_repeat(r) for r in free), "precondition: without the processor some row repeats a bigram"
    held = model.generate(no_repeat_ngram_size=2, **kw)
    assert held.shape == (12, 40)
    assert not any(bigrams_repeat(r) for r in held.tolist())


def test_logprobs_match_a_teacher_forced_pass(small):
    """sum of the returned log-probs per sequence == the sum recomputed on the host from a teacher-forced forward pass through the
    same processors and warpers, to 2e-2 relative (bf16 weights and fp32 logits on both sides; the two passes associate their sums
    differently)."""
    model, inputs = small
    B, n, ML, T, k, p = 3, 4, 10, 0.8, 0, 0.9
    kw = inputs(B)
    ids, lp = model.generate(do_sample=True, temperature=T, top_k=k, top_p=p, num_return_sequences=n, max_length=ML, min_length=3,
                             no_repeat_ngram_size=2, seed=8, return_logprobs=True, **kw)
    L = ids.shape[1]
    rep = {key: (v.repeat_interleave(n, dim=0) if torch.is_tensor(v) else v) for key, v in kw.items()}
    with torch.no_grad():
        logits = model(decoder_input_ids=ids[:, :-1].contiguous(), **rep)["logits"].float().cpu().numpy()
    ids, lp = ids.cpu().numpy(), lp.cpu().numpy()
    for r in range(B * n):
        total, done = 0.0, False
        for t in range(1, L):
            if done:
                assert ids[r, t] == PAD and lp[r, t] == 0
                continue
            z = host_processors(logits[r, t - 1, :model.V].astype(F32), history=ids[r, :t], ngram=2, eos=EOS, suppress_eos=t < 3,
                                forced=EOS if t == ML - 1 else -1)
            w = host_warp(z, T, k, p)
            assert w["kept"][ids[r, t]], (r, t, "token outside the host's kept set")
            total += float(np.log(w["p"][ids[r, t]]))
            done = ids[r, t] == EOS
        got = float(lp[r].sum())
        assert abs(got - total) <= 2e-2 * max(abs(total), 1e-3), (r, got, total)


def test_trainer_loop_and_caption_pipeline_pass_sampling_through():
    """training.gen_caption_from_loader_bart(do_sample=True, ...) — the plain loop and CaptionPipeline — hand the sampling keywords
    to generate(): the same seed gives the same rows either way, num_return_sequences rows per caption, "logprobs" next to "gen"
    when asked for, no staged encoder side, and generate()'s refusals come through."""
    from vacnic_amd import synthetic
    from vacnic_amd.config import ClipVisionConfig, VacnicConfig, generation_defaults
    from vacnic_amd.generate import CaptionPipeline
    from vacnic_amd.training import _model_inputs, build_models, gen_caption_from_loader_bart, to_device
    cfg = VacnicConfig(d_model=768, encoder_layers=1, decoder_layers=1, encoder_attention_heads=12, decoder_attention_heads=12,
                       encoder_ffn_dim=3072, decoder_ffn_dim=3072, enc_fusion_layer=[0], dim_common=768, clip_width=128, dropout=0.0)
    vcfg = ClipVisionConfig(width=128, layers=1, patch_size=16, image_size=32, output_dim=64)
    model, _, _ = build_models(cfg, vcfg, init="synthetic", seed=5)
    n = 3
    kw = dict(do_sample=True, temperature=1.5, top_p=0.9, num_return_sequences=n, seed=11, min_length=5)
    for B in (1, 2):
        batches = [synthetic.make_batch(cfg, B, S=24, T=8, F=2, seed=70 + i, image_size=32) for i in range(3)]
        plain = gen_caption_from_loader_bart(model, batches, 1, 10, pipeline=False, **kw)
        piped = gen_caption_from_loader_bart(model, batches, 1, 10, pipeline=True, return_logprobs=True, **kw)
        assert len(plain) == len(piped) == 3
        for i in range(3):
            gen = piped[i]["gen"]
            assert gen == plain[i]["gen"], (B, i, gen, plain[i]["gen"])
            assert "logprobs" not in plain[i] and len(gen) == B * n
            lp = piped[i]["logprobs"]
            assert len(lp) == B * n and all(len(a) == len(b) for a, b in zip(lp, gen))
            assert all(row[0] == START and EOS in row[1:] for row in gen)
            for item in range(B):                          # drawn, not greedy: the samples of one caption differ
                assert len({tuple(r) for r in gen[item * n:(item + 1) * n]}) > 1
            assert all(v <= 0 for row in lp for v in row) and any(v < 0 for row in lp for v in row)
        pipe = CaptionPipeline(model, lambda b: _model_inputs(model, b, graphed=True), 1, max_length=10, add_ner_ffn=True,
                               **dict(generation_defaults(), **kw))
        direct = [g.tolist() for _, g in pipe(to_device(b, "cuda") for b in batches)]
        assert not pipe.stages and direct == [plain[i]["gen"] for i in range(3)]
    with pytest.raises(ValueError, match="num_beams"):
        gen_caption_from_loader_bart(model, batches[:1], 2, 10, pipeline=False, **kw)
    with pytest.raises(ValueError, match="top_p"):
        gen_caption_from_loader_bart(model, batches[:1], 1, 10, pipeline=True, **dict(kw, top_p=0.0))


def test_sampling_sessions_are_bounded(small):
    """a model keeps at most generate._SAMPLE_SESSIONS_MAX sampling sessions, the most recently used ones; a session that comes
    back after it was dropped draws what it drew before"""
    import vacnic_amd.generate as gen
    model, inputs = small
    model.__dict__.pop("_sample_sessions", None)
    kw = dict(inputs(1), do_sample=True, temperature=1.5, seed=4, max_length=6, min_length=6)
    first = model.generate(num_return_sequences=1, **kw)
    for n in range(2, gen._SAMPLE_SESSIONS_MAX + 1):
        model.generate(num_return_sequences=n, **kw)
    assert [k[0] for k in model._sample_sessions] == list(range(1, gen._SAMPLE_SESSIONS_MAX + 1))
    assert torch.equal(model.generate(num_return_sequences=1, **kw), first)              # used again: now the most recent
    model.generate(num_return_sequences=gen._SAMPLE_SESSIONS_MAX + 1, **kw)
    assert [k[0] for k in model._sample_sessions] == list(range(3, gen._SAMPLE_SESSIONS_MAX + 1)) + [1, gen._SAMPLE_SESSIONS_MAX + 1]
    model.generate(num_return_sequences=2, **kw)                                         # dropped above: built anew
    assert len(model._sample_sessions) == gen._SAMPLE_SESSIONS_MAX and list(model._sample_sessions)[-1][0] == 2
