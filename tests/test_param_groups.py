"""AdamW parameter groups, host side: the group-table builder on host arenas, spec errors, the trainers' flags, the checkpoint
field and the argument checks of the two C entry points (no GPU)."""
import importlib.util
import io
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRAINERS = {"run_full_train": "train_mmbart_enc_self_face_name_ids_retrieve_crossattn_bart_guide_match.py",
            "run_onlyvis_train": "run_train_mmbart_enc_self_onlyvis_retrieve_crossattn.py"}
WD = 0.01


def small_cfg(**kw):
    from vacnic_amd.config import VacnicConfig
    base = dict(d_model=768, encoder_layers=2, decoder_layers=1, encoder_attention_heads=12, decoder_attention_heads=12,
                encoder_ffn_dim=256, decoder_ffn_dim=256, enc_fusion_layer=[0], dim_common=768, clip_width=768, vocab_size=50267)
    base.update(kw)
    return VacnicConfig(**base)


_MODELS = {}


def host_model(init_attn_weight=False):
    from vacnic_amd.models.mmbart import BartForMultiModalGeneration
    if init_attn_weight not in _MODELS:
        cfg = small_cfg()
        _MODELS[init_attn_weight] = BartForMultiModalGeneration(cfg, enc_fusion_layer=[0], dim_common=768, prompt_size=cfg.prompt_size,
                                                                init_attn_weight=init_attn_weight).finalize("cpu")
    return _MODELS[init_attn_weight]


def _load(fname):
    spec = importlib.util.spec_from_file_location("trainer_under_test_" + fname[:3], os.path.join(ROOT, fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def per_element(table, n):
    """(lr_scale, weight_decay, frozen) of every arena element, expanded from the table."""
    lr, wd, fr = torch.empty(n), torch.empty(n), torch.empty(n, dtype=torch.bool)
    for s, e, a, b, c in table.segments():
        lr[s:e] = a; wd[s:e] = b; fr[s:e] = c
    return lr, wd, fr


# ------------------------------------------------------------------------------------------------ 1: the table builder
@pytest.mark.parametrize("tied_attn", [False, True])
def test_group_table_on_a_host_arena(built_lib, tied_attn):
    from vacnic_amd.arena import no_decay_spec
    m = host_model(tied_attn)
    a = m.arena
    spec = no_decay_spec(m)
    t = a.group_table(m.named_parameters(), spec, WD)
    segs = t.segments()
    # tiles [0, n) in ascending order without overlap
    assert segs[0][0] == 0 and segs[-1][1] == a.n
    assert all(s < e for s, e, *_ in segs) and all(segs[i][1] == segs[i + 1][0] for i in range(len(segs) - 1))
    assert t.seg_start.dtype == torch.int64 and t.first_seg.dtype == torch.int32 and t.seg.shape == (len(segs), 4)
    # adjacent equal segments are merged
    assert all(segs[i][2:] != segs[i + 1][2:] for i in range(len(segs) - 1))
    assert len(segs) < len(a.slots)
    # first_seg[b] is the segment that holds element 1024 b
    assert t.first_seg.numel() == a.n // 1024
    for b in (0, 1, a.n // 2048, a.n // 1024 - 1):
        s = int(t.first_seg[b])
        assert segs[s][0] <= 1024 * b < segs[s][1]
    lr, wd, fr = per_element(t, a.n)
    assert (lr == 1.0).all() and not fr.any()
    ln_params = {id(p) for mod in m.modules() if isinstance(mod, torch.nn.LayerNorm) for p in mod.parameters()}
    seen, n_nodecay = set(), 0
    for name, p in m.named_parameters(remove_duplicate=False):
        if id(p) in seen:
            continue
        seen.add(id(p))
        o, n, cap = a.slots[id(p)]
        if name.endswith(".bias") or id(p) in ln_params:
            assert (wd[o:o + n] == 0.0).all(), name
            n_nodecay += 1
        elif p.dim() >= 2:
            assert (wd[o:o + n] == WD).all(), name
        else:
            raise AssertionError(f"{name}: neither a bias, a LayerNorm parameter nor a matrix")
    assert n_nodecay == len(spec[0]["match"]) and n_nodecay > 20
    assert any("layernorm_embedding" in x for x in spec[0]["match"]) and any("_layer_norm.weight" in x for x in spec[0]["match"])
    # a tied weight appears once, under its first name
    assert "lm_head.weight" not in spec[0]["match"] and len(seen) == len(a.slots)
    if tied_attn:
        l0 = m.model.encoder.layers[0]
        assert l0.self_attn_img_name.q_proj.weight is l0.self_attn.q_proj.weight
        assert not any("self_attn_img_name.q_proj.weight" in nm for nm, _ in m.named_parameters())
    # the pad_rows rows of the embedding (and the gap behind it) belong to the embedding's segment
    emb = m.model.shared.weight
    o, n, cap = a.slots[id(emb)]
    assert cap == m.V_pad * emb.shape[1] > n
    nxt = min([s[0] for s in a.slots.values() if s[0] > o] + [a.n])
    assert (wd[o:nxt] == WD).all() and nxt >= o + cap

    # a spec that touches the embedding: its padding follows it; freezing by alias name is refused
    t2 = a.group_table(m.named_parameters(), [{"match": r"^model\.shared\.weight$", "frozen": True, "lr_scale": 3.0}] + spec, WD)
    lr2, wd2, fr2 = per_element(t2, a.n)
    assert fr2[o:nxt].all() and (lr2[o:nxt] == 3.0).all() and int(fr2.sum()) == nxt - o
    assert torch.equal(wd2, wd), "weight_decay resolves on its own: the freeze entry does not set it"
    with pytest.raises(ValueError, match="first name"):
        a.group_table(m.named_parameters(), [{"match": ["lm_head.weight"], "frozen": True}], WD)


def test_fields_resolve_independently_and_first_match_wins(built_lib):
    from vacnic_amd.arena import resolve_spec
    names = ["a.weight", "a.bias", "b.weight", "b.bias"]
    spec = [{"match": r"^b\.", "frozen": True}, {"match": r"^a\.", "lr_scale": 10.0}, {"match": r"\.weight$", "lr_scale": 2.0},
            {"match": ["a.bias", "b.bias"], "weight_decay": 0.0}]
    got = resolve_spec(names, spec, 0.05)
    assert got == {"a.weight": (10.0, 0.05, False), "a.bias": (10.0, 0.0, False), "b.weight": (2.0, 0.05, True), "b.bias": (1.0, 0.0, True)}
    full = [{"match": "weight", "lr_scale": 1.0, "weight_decay": 0.3, "frozen": False}, {"match": r"^a\.", "lr_scale": 5.0, "weight_decay": 0.0, "frozen": True}]
    got = resolve_spec(names, full, 0.05)
    assert got["a.weight"] == (1.0, 0.3, False) and got["a.bias"] == (5.0, 0.0, True) and got["b.bias"] == (1.0, 0.05, False)


def test_table_from_segments_merges_and_checks(built_lib):
    from vacnic_amd.arena import table_from_segments
    t = table_from_segments(4104, [(0, 1, 0.01, False), (1, 1, 0.01, False), (3, 10, 0.0, False), (1024, 1, 0, True), (4100, 1, 0, True)])
    assert t.segments() == [(0, 3, 1.0, pytest.approx(0.01), False), (3, 1024, 10.0, 0.0, False), (1024, 4104, 1.0, 0.0, True)]
    assert t.first_seg.tolist() == [0, 2, 2, 2, 2]          # ceil(4104 / 1024) blocks
    for bad in ([(1, 1, 0, False)], [(0, 1, 0, False), (0, 2, 0, False)], [(0, 1, 0, False), (8, 2, 0, False), (4, 1, 0, False)],
                [(0, 1, 0, False), (4104, 2, 0, False)], []):
        with pytest.raises(ValueError):
            table_from_segments(4104, bad)


# ------------------------------------------------------------------------------------------------------ 2: spec errors
def test_spec_errors(built_lib):
    m = host_model()
    a = m.arena
    with pytest.raises(ValueError, match="matches no parameter"):
        a.group_table(m.named_parameters(), [{"match": r"encoder\.layerz\.", "lr_scale": 2.0}], WD)
    with pytest.raises(ValueError, match="name no parameter"):
        a.group_table(m.named_parameters(), [{"match": ["model.shared.weigth"], "frozen": True}], WD)
    both = ["model.shared.weight", "model.encoder.layernorm_embedding.bias"]
    with pytest.raises(ValueError, match="both list"):
        a.group_table(m.named_parameters(), [{"match": both, "weight_decay": 0.0}, {"match": both[1:], "weight_decay": 0.1}], WD)
    # ... but two lists that set different fields combine
    a.group_table(m.named_parameters(), [{"match": both, "weight_decay": 0.0}, {"match": both[1:], "lr_scale": 2.0}], WD)
    with pytest.raises(ValueError, match="lr_scale"):
        a.group_table(m.named_parameters(), [{"match": "shared", "lr_scale": -1.0}], WD)
    with pytest.raises(ValueError, match="weight_decay"):
        a.group_table(m.named_parameters(), [{"match": "shared", "weight_decay": float("nan")}], WD)
    with pytest.raises(ValueError, match="sets none"):
        a.group_table(m.named_parameters(), [{"match": "shared"}], WD)
    with pytest.raises(ValueError, match="an entry is a dict"):
        a.group_table(m.named_parameters(), [{"match": "shared", "lr": 2.0}], WD)
    with pytest.raises(ValueError, match="bad regex"):
        a.group_table(m.named_parameters(), [{"match": "shared(", "frozen": True}], WD)
    from vacnic_amd.training import FusedAdamW
    with pytest.raises(ValueError, match="named_parameters"):
        FusedAdamW(a, lr=1e-4, param_groups=[{"match": "shared", "frozen": True}])


# --------------------------------------------------------------------------------------------------- 3: trainer flags
@pytest.mark.parametrize("which", sorted(TRAINERS))
def test_trainer_flags_build_the_spec(built_lib, which):
    from vacnic_amd.arena import no_decay_spec
    from vacnic_amd.training import param_group_spec
    mod = _load(TRAINERS[which])
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_trainer_flags.json")))[which]
    assert ref["script"] == TRAINERS[which]
    args = mod.parser.parse_args(ref["argv"])                      # the reference's flag lines parse unchanged ...
    assert args.no_decay_bias_ln is False and args.lr_scale == [] and args.freeze == []
    targs = mod.train_args(args, 100)
    assert targs.lr_bart == 3e-5 and targs.weight_decay == 0.01 and targs.num_training_steps == 100
    m = host_model()
    assert param_group_spec(m, targs) is None                      # ... and absent flags mean no groups
    args = mod.parser.parse_args(ref["argv"] + ["--no_decay_bias_ln", "True", "--lr_scale", "prompt_mlp|visual_map=10",
                                                "--lr_scale", r"cross_attn_img_ner\.=2.5", "--freeze", r"^model\.shared\.",
                                                "--freeze", r"encoder\.layers\.1\."])
    targs = mod.train_args(args, 100)
    assert targs.freeze == (r"^model\.shared\.", r"encoder\.layers\.1\.") and targs.no_decay_bias_ln is True
    assert targs.lr_scale == (("prompt_mlp|visual_map", 10.0), (r"cross_attn_img_ner\.", 2.5))
    spec = param_group_spec(m, targs)
    assert spec == [{"match": r"^model\.shared\.", "frozen": True}, {"match": r"encoder\.layers\.1\.", "frozen": True},
                    {"match": "prompt_mlp|visual_map", "lr_scale": 10.0}, {"match": r"cross_attn_img_ner\.", "lr_scale": 2.5}] + no_decay_spec(m)
    lr, wd, fr = per_element(m.arena.group_table(m.named_parameters(), spec, targs.weight_decay), m.arena.n)
    named = dict(m.named_parameters())

    def at(name):
        o = m.arena.slots[id(named[name])][0]
        return lr[o].item(), round(wd[o].item(), 6), fr[o].item()
    pm_bias = next(n for n in named if "prompt_mlp" in n and n.endswith(".bias"))
    pm_weight = next(n for n in named if "prompt_mlp" in n and n.endswith(".weight"))
    assert at(pm_bias) == (10.0, 0.0, False) and at(pm_weight) == (10.0, 0.01, False)      # scaled AND un-decayed
    assert at("model.shared.weight") == (1.0, 0.01, True)
    assert at("model.encoder.layers.1.self_attn_layer_norm.weight") == (1.0, 0.0, True)
    assert at("model.encoder.layers.0.self_attn_layer_norm.weight") == (1.0, 0.0, False)
    assert at("model.decoder.layers.0.fc1.weight") == (1.0, 0.01, False)
    only = param_group_spec(m, mod.train_args(mod.parser.parse_args(ref["argv"] + ["--no_decay_bias_ln", "True"]), 100))
    assert only == no_decay_spec(m)
    with pytest.raises(ValueError, match="REGEX=FLOAT"):
        mod.train_args(mod.parser.parse_args(ref["argv"] + ["--lr_scale", "prompt_mlp"]), 100)


# ------------------------------------------------------------------------------------------------------ 4: checkpoint
def test_checkpoint_carries_the_spec(built_lib):
    from vacnic_amd import checkpoint
    from vacnic_amd.arena import no_decay_spec
    from vacnic_amd.training import FusedAdamW
    m = host_model()
    spec = [{"match": r"^model\.shared\.", "frozen": True}, {"match": "prompt_mlp", "lr_scale": 10}] + no_decay_spec(m)

    def opt(groups):
        return FusedAdamW(m.arena, lr=3e-5, num_warmup_steps=5, num_training_steps=100, param_groups=groups,
                          named_parameters=m.named_parameters())
    o1 = opt(spec)
    assert o1.table.nseg > 3 and o1.state_dict()["param_groups"] == o1.param_groups
    assert "param_groups" not in opt(None).state_dict()
    o1.arena.exp_avg.normal_(); o1.hyper.copy_(torch.tensor([1.25e-5, 7.0]))
    want = o1.arena.exp_avg.clone()
    buf = io.BytesIO()
    ck = checkpoint.save_checkpoint(buf, m, o1, step=7)
    saved = ck["schedule"]["param_groups"]
    assert saved == o1.param_groups and saved[1] == {"match": "prompt_mlp", "lr_scale": 10.0, "weight_decay": None, "frozen": None}
    assert json.loads(json.dumps(saved)) == saved, "plain data"
    buf.seek(0)
    o2 = opt(json.loads(json.dumps(spec)))
    assert checkpoint.load_checkpoint(buf, m, o2)["step"] == 7      # through torch.save / torch.load
    assert torch.equal(o2.hyper, o1.hyper)
    for o, n, _ in m.arena.slots.values():                          # (moments are restored where a parameter lives)
        assert torch.equal(o2.arena.exp_avg[o:o + n], want[o:o + n])
    other = opt(spec[:1])
    with pytest.raises(ValueError) as err:
        checkpoint.load_checkpoint(ck, m, other)
    assert "prompt_mlp" in str(err.value) and str(other.param_groups) in str(err.value), "the message names both specs"
    with pytest.raises(ValueError, match="param_groups=None"):
        checkpoint.load_checkpoint(ck, m, opt(None))
    # a checkpoint without the key: loads into a group-less optimizer as before, not into a grouped one
    plain = checkpoint.save_checkpoint(io.BytesIO(), m, opt(None), step=3)
    assert "param_groups" not in plain["schedule"]
    assert checkpoint.load_checkpoint(plain, m, opt(None))["step"] == 3
    with pytest.raises(ValueError, match="param_groups=None"):
        checkpoint.load_checkpoint(plain, m, o2)


# --------------------------------------------------------------------------------------------------- 5: bad arguments
def test_grouped_entries_return_status_not_abort(built_lib):
    """validation happens before any launch: fake non-null addresses are never dereferenced."""
    from vacnic_amd import _lib
    ok = dict(stream=None, p=16, g=32, m=48, v=64, p_bf16=None, hyper=16, n=8, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0,
              zero_grad=1, clip_coef=None, seg_start=16, seg=16, first_seg=16, nseg=1, nblocks=1, elem_base=0)
    for bad, msg in ((dict(p=None), "null operand"), (dict(hyper=None), "null operand"), (dict(n=6), "multiple of 4"),
                     (dict(g=36), "16-byte aligned"), (dict(p_bf16=4), "16-byte aligned"), (dict(seg=None), "null group table"),
                     (dict(first_seg=None), "null group table"), (dict(nseg=0), "nseg=0"), (dict(elem_base=-4), "elem_base=-4"),
                     (dict(elem_base=1020), "outside the table")):
        with pytest.raises(ValueError, match=msg):
            _lib.call_struct("vacnic_adamw_groups", **dict(ok, **bad))
    ok = dict(stream=None, g=32, n=8, grad_scale=1.0, max_norm=0.1, partials=16, out=16, seg_start=16, seg=16, first_seg=16,
              nseg=1, nblocks=1, elem_base=0)
    for bad, msg in ((dict(g=None), "null operand"), (dict(out=None), "null operand"), (dict(n=6), "multiple of 4"),
                     (dict(g=36), "16-byte aligned"), (dict(max_norm=0.0), "max_norm"), (dict(seg_start=None), "null group table"),
                     (dict(nseg=0), "nseg=0"), (dict(elem_base=-4), "elem_base=-4"), (dict(n=2048), "outside the table")):
        with pytest.raises(ValueError, match=msg):
            _lib.call_struct("vacnic_grad_clip_coef_groups", **dict(ok, **bad))
