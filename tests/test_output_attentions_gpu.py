"""forward(output_attentions=True) on the MI355X: the attention maps of the small full model and of the only_image model
against an fp32 CPU restatement built from the oracle's own pieces (its hidden states are pinned to the real reference by
tests/golden/*.npz; the probabilities are an intermediate of the same formulas, MFULL:509-541)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# Closeness of a map to the fp32 restatement.  The bound comes from the bf16 model's own contract, not from the code under
# test: the model tests accept 1e-2 relative on hidden states, the scores scale * q . k inherit that error and a probability
# moves by at most |p| * |delta score| — so the maps cannot be asked for more than about 1e-2 absolute, and an error above
# 5e-2 would be a bug, not rounding.  Measured on the GPU over every map of both models (profiles/attn_probs_error.txt):
# max |map - restatement| = 5.457e-03 (only_image, decoder_attentions[1]); the bound is 4x that.
MAP_ABS_BOUND = 4 * 5.457e-03
QK_GAIN = 1.5           # the synthetic N(0, 0.02) projections give flat maps (row maxima ~0.1); q/k weights x1.5 give maxima of 0.3-0.8


def small_cfg(**kw):
    from vacnic_amd.config import VacnicConfig
    base = dict(d_model=768, encoder_layers=2, decoder_layers=2, encoder_attention_heads=12, decoder_attention_heads=12,
                encoder_ffn_dim=3072, decoder_ffn_dim=3072, enc_fusion_layer=[0], dim_common=768, clip_width=768, dropout=0.0)
    base.update(kw)
    return VacnicConfig(**base)


def state_dict_for(cfg):
    from vacnic_amd import synthetic
    sd = synthetic.make_state_dict(synthetic.mmbart_param_shapes(cfg), seed=1)
    for name, w in sd.items():
        if name.endswith("q_proj.weight") or name.endswith("k_proj.weight"):
            w.mul_(QK_GAIN)
    return sd


def build(cfg):
    from vacnic_amd import synthetic
    from vacnic_amd.config import ClipVisionConfig
    from vacnic_amd.training import build_models
    sd = state_dict_for(cfg)
    vcfg = ClipVisionConfig(width=128, layers=1, patch_size=16, image_size=32, output_dim=64)
    clip_sd = synthetic.make_state_dict(synthetic.clip_visual_param_shapes(vcfg), seed=4, std=0.05)
    model, _, _ = build_models(cfg, vcfg, state_dicts=(sd, None, clip_sd), with_guide=False)
    return model, sd


def inputs(cfg, B, S, T, F, seed):
    """(kwargs for the HIP model, kwargs for the oracle, masks) of one masked ragged batch."""
    from oracle import vacnic_oracle as O
    from vacnic_amd import kernels as K, synthetic
    batch = synthetic.make_batch(cfg, B, S=S, T=T, F=F, seed=seed, image_size=32)
    img = synthetic.image_features(cfg, B)
    src, tgt = batch["article_ids"].cuda(), batch["caption_ids"].cuda()
    src_mask, _ = K.prep_ids(src, 1)
    _, tgt_in = K.prep_ids(tgt, 1, start_id=2)
    gpu = dict(input_ids=src, attention_mask=src_mask, decoder_input_ids=tgt_in, image_features=img.cuda(), labels=tgt, output_logits=True)
    cpu = dict(input_ids=batch["article_ids"], attention_mask=O.create_src_mask_bart(batch["article_ids"]),
               decoder_input_ids=O.shift_tokens_right(batch["caption_ids"], 1, 2), image_features=img)
    masks = {"src": cpu["attention_mask"].bool()}
    if not cfg.only_image:
        face = batch["face_emb"].cuda()
        names_mask, _ = K.prep_ids(batch["names_art_ids"].cuda(), 1)
        gpu.update(face_features=face, face_mask=K.face_mask(face), name_ids=batch["names_art_ids"].cuda(), name_mask=names_mask)
        cpu.update(face_features=batch["face_emb"], face_mask=O.create_src_mask_bart(batch["face_emb"][:, :, -1]),
                   name_ids=batch["names_art_ids"], name_mask=O.create_src_mask_bart(batch["names_art_ids"]))
        masks["face_name"] = torch.cat((cpu["face_mask"], cpu["name_mask"]), dim=1).bool()
    return gpu, cpu, masks


def restated_maps(sd, cfg, cpu):
    """fp32 CPU maps per attention module: the oracle's forward runs unchanged; its `attention` is wrapped for the duration of the
    call so that, for every attention it evaluates, q and k are recomputed from the hidden states it was handed (the oracle's
    linear, the reference's head split and scaling) and softmax(q k^T + mask) is kept under the module's parameter prefix."""
    from oracle import vacnic_oracle as O
    maps, orig = {}, O.attention

    def recording(sd_, prefix, hidden, num_heads, key_value_states=None, attention_mask=None):
        B, T, d = hidden.shape
        hd = d // num_heads
        src = hidden if key_value_states is None else key_value_states
        q = (O.linear(sd_, prefix + ".q_proj", hidden) * hd ** -0.5).view(B, T, num_heads, hd).transpose(1, 2)
        k = O.linear(sd_, prefix + ".k_proj", src).view(B, -1, num_heads, hd).transpose(1, 2)
        w = torch.matmul(q, k.transpose(-1, -2))
        if attention_mask is not None:
            w = w + attention_mask
        maps[prefix] = torch.softmax(w, dim=-1)
        return orig(sd_, prefix, hidden, num_heads, key_value_states, attention_mask)

    O.attention = recording
    try:
        with torch.no_grad():
            O.mmbart_forward(sd, cfg, **cpu)
    finally:
        O.attention = orig
    return maps


def expected(cfg, maps):
    """output key -> per-layer list of restated maps (None where the model returns None)."""
    e, d = "model.encoder.layers.", "model.decoder.layers."
    fused = [i in cfg.enc_fusion_layer for i in range(cfg.encoder_layers)]
    return {
        "encoder_attentions": [maps[f"{e}{i}.self_attn"] for i in range(cfg.encoder_layers)],
        "encoder_name_face_attentions": [maps[f"{e}{i}.self_attn_img_name"] if f and not cfg.only_image else None for i, f in enumerate(fused)],
        "encoder_img_ner_cross_attentions": [maps[f"{e}{i}.cross_attn_img_ner"] if f else None for i, f in enumerate(fused)],
        "decoder_attentions": [maps[f"{d}{i}.self_attn"] for i in range(cfg.decoder_layers)],
        "cross_attentions": [maps[f"{d}{i}.encoder_attn"] for i in range(cfg.decoder_layers)],
    }


MAP_KEYS = ("encoder_attentions", "decoder_attentions", "cross_attentions", "encoder_name_face_attentions",
            "encoder_img_ner_cross_attentions")


def map_errors(out, want):
    """{(key, layer): max abs error} over every map."""
    errs = {}
    for key in MAP_KEYS:
        for i, (got, ref) in enumerate(zip(out[key], want[key])):
            if ref is not None:
                errs[(key, i)] = (got.float().cpu() - ref).abs().max().item()
    return errs


def check_structure(cfg, out, want, masks, B, S, T):
    H = cfg.encoder_attention_heads
    for key in MAP_KEYS:
        assert key in out, f"{key} missing"
        assert isinstance(out[key], tuple) and len(out[key]) == len(want[key]), key
        for i, (got, ref) in enumerate(zip(out[key], want[key])):
            if ref is None:
                assert got is None, f"{key}[{i}]: a layer that is not fused returns None"
                continue
            assert got is not None, f"{key}[{i}] is None"
            assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape), (key, i, got.dtype, tuple(got.shape), tuple(ref.shape))
            assert not got.requires_grad and got.grad_fn is None, f"{key}[{i}] carries an autograd graph"
    P = cfg.prompt_len
    assert tuple(out["encoder_attentions"][0].shape) == (B, H, S, S)
    assert tuple(out["decoder_attentions"][0].shape) == (B, H, T, T)
    assert tuple(out["cross_attentions"][0].shape) == (B, H, T, S)
    assert tuple(out["encoder_img_ner_cross_attentions"][0].shape) == (B, H, S, P if cfg.only_image else P + cfg.max_ner_type_len_gt)
    # padded keys and the causal triangle: exactly zero
    dead = ~masks["src"].cuda()                                   # [B, S]
    assert dead.any(), "the batch must be ragged for this check to mean anything"
    for m in out["encoder_attentions"] + out["cross_attentions"]:
        assert (m.permute(0, 3, 1, 2)[dead] == 0).all(), "a padded article key got probability"
    upper = torch.ones(T, T, dtype=torch.bool, device="cuda").triu(1)
    for m in out["decoder_attentions"]:
        assert (m[..., upper] == 0).all(), "the causal upper triangle got probability"
    if not cfg.only_image:
        N = cfg.max_ner_type_len
        fn = masks["face_name"].cuda()                            # [B, F + N]
        live = fn.any(1)
        m = out["encoder_name_face_attentions"][0]
        assert tuple(m.shape) == (B, H, N, fn.shape[1])
        assert (m.permute(0, 3, 1, 2)[(~fn) & live[:, None]] == 0).all(), "a padded face / name key got probability"


FULL = (dict(), dict(B=3, S=48, T=12, F=3, seed=7))
ONLY_IMAGE = (dict(only_image=True, enc_fusion_layer=[0, 1]), dict(B=2, S=32, T=8, F=0, seed=8))


@pytest.mark.parametrize("ckw,dims", [FULL, ONLY_IMAGE], ids=["full", "only_image"])
def test_maps_match_the_restatement_and_leave_the_outputs_alone(ckw, dims):
    cfg = small_cfg(**ckw)
    model, sd = build(cfg)
    model.eval()
    gpu, cpu, masks = inputs(cfg, **dims)
    with torch.no_grad():
        plain = model(**gpu)
        out = model(output_attentions=True, **gpu)
        off = model(output_attentions=False, **gpu)
    for key in MAP_KEYS:
        assert key not in plain and key not in off, f"{key} returned without output_attentions=True"
    # the flag changes nothing the model already returned: bit-identical
    assert torch.equal(out["logits"], plain["logits"])
    assert torch.equal(out["decoder_hidden_states"][-1], plain["decoder_hidden_states"][-1])
    if not cfg.only_image:
        assert torch.equal(out["hidden_states_face"], plain["hidden_states_face"])
    want = expected(cfg, restated_maps(sd, cfg, cpu))
    check_structure(cfg, out, want, masks, dims["B"], dims["S"], dims["T"])
    errs = map_errors(out, want)
    for k, v in sorted(errs.items()):
        print(f"map error (eval, {'only_image' if cfg.only_image else 'full'}) {k[0]}[{k[1]}]: {v:.3e}")
    worst = max(errs.values())
    assert worst <= MAP_ABS_BOUND, f"max map error {worst:.3e} > {MAP_ABS_BOUND:.3e}: {max(errs, key=errs.get)}"


def test_config_output_attentions_is_the_default_of_the_kwarg():
    cfg = small_cfg(encoder_layers=1, decoder_layers=1, output_attentions=True)
    model, _ = build(cfg)
    model.eval()
    gpu, _, _ = inputs(cfg, B=2, S=32, T=8, F=2, seed=9)
    with torch.no_grad():
        assert "encoder_attentions" in model(**gpu)                                  # None -> config.output_attentions
        assert "encoder_attentions" not in model(output_attentions=False, **gpu)     # an explicit False wins


def test_decoding_ignores_config_output_attentions():
    """generate() and greedy_generate() return ids only (maps are out of scope there): with config.output_attentions=True they
    run, give the ids of the same model without the flag, and issue the same number of C-ABI calls — no map kernel, no map
    allocation."""
    from vacnic_amd import _lib
    got = {}
    for flag in (False, True):
        cfg = small_cfg(encoder_layers=1, decoder_layers=1, output_attentions=flag)
        model, _ = build(cfg)
        model.eval()
        gpu, _, _ = inputs(cfg, B=2, S=24, T=8, F=2, seed=9)
        kw = {k: gpu[k] for k in ("image_features", "face_features", "face_mask", "name_ids", "name_mask")}
        c0 = _lib.CALLS
        greedy = model.greedy_generate(gpu["input_ids"], gpu["attention_mask"], 6, **kw)
        c1 = _lib.CALLS
        beams = model.generate(input_ids=gpu["input_ids"], attention_mask=gpu["attention_mask"], num_beams=2, max_length=8,
                               add_ner_ffn=True, **kw)
        c2 = _lib.CALLS
        got[flag] = (greedy.cpu(), beams.cpu(), c1 - c0, c2 - c1)
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1])
    assert got[True][2] == got[False][2], f"greedy_generate: {got[True][2]} C-ABI calls with the flag in the config, {got[False][2]} without"
    assert got[True][3] == got[False][3], f"generate: {got[True][3]} C-ABI calls with the flag in the config, {got[False][3]} without"


def test_training_mode_maps_are_pre_dropout_and_carry_no_graph():
    """attention_dropout=0.1, train mode: the maps are the softmax BEFORE dropout (MFULL:534 vs :546); the loss still
    back-propagates and no gradient flows through the maps.  Hidden-state dropout is off (dropout=0.0), so attention dropout is
    the only difference between the two modes.

    What "pre-dropout" implies, and what is asserted:
      - a map whose inputs no dropout has touched yet (the first encoder self-attention, the first name attention, the first
        decoder self-attention) IS the eval-mode map of the same weights: asserted to the bit;
      - every map is a softmax: each row sums to 1 within the kernel test's derived bound and every visible key has a
        probability > 0 — a map taken after dropout has a tenth of its entries zeroed, the rest scaled by 1/0.9, and rows that
        do not sum to 1.
    The later maps cannot equal their eval-mode counterparts to rounding, in the reference no more than here: their q and k
    come from hidden states that dropped probabilities have already moved.  Measured against the eval-mode maps with the seed
    below (profiles/attn_probs_error.txt): encoder_attentions[1] 1.06e-2, encoder_img_ner_cross_attentions[0] 1.01e-2,
    cross_attentions 2.02e-2 / 3.57e-2, decoder_attentions[1] 6.60e-2 — the size of the dropout noise, against 0 for the three
    first maps and 5.5e-3 of bf16 error."""
    from vacnic_amd import ops
    ops.Rng.manual_seed(1234)                       # the dropout masks of this test do not depend on what ran before it
    cfg = small_cfg(attention_dropout=0.1)
    model, sd = build(cfg)
    dims = dict(B=3, S=48, T=12, F=3, seed=7)
    gpu, cpu, masks = inputs(cfg, **dims)
    model.eval()
    with torch.no_grad():
        ev = model(output_attentions=True, **gpu)
    model.train()
    tr = model(output_attentions=True, **gpu)
    want = expected(cfg, restated_maps(sd, cfg, cpu))
    check_structure(cfg, tr, want, masks, dims["B"], dims["S"], dims["T"])
    errs = {}
    for key in MAP_KEYS:
        for i, (a, b) in enumerate(zip(tr[key], ev[key])):
            if a is None:
                assert b is None
                continue
            assert not a.requires_grad
            errs[(key, i)] = (a - b).abs().max().item()
            Tk = a.shape[-1]
            rowsum = (a.double().sum(-1) - 1.0).abs().max().item()
            print(f"map train-vs-eval {key}[{i}]: {errs[(key, i)]:.3e}  max|rowsum-1| {rowsum:.3e}")
            assert rowsum <= (Tk + 8) * 2.0 ** -23, f"{key}[{i}]: rows of a train-mode map do not sum to 1 ({rowsum:.3e})"
            assert ((a > 0) == (b > 0)).all(), f"{key}[{i}]: train-mode map has zeros where the eval-mode map has none"
    for first in (("encoder_attentions", 0), ("encoder_name_face_attentions", 0), ("decoder_attentions", 0)):
        assert errs[first] == 0.0, f"{first}: no dropout upstream, yet the train-mode map differs from the eval-mode map"
    tr["loss"].backward()
    torch.cuda.synchronize()
    g = model.model.decoder.layers[0].self_attn.q_proj.weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().max().item() > 0
