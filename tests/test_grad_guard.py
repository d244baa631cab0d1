"""CPU: the host side of the non-finite gradient guard — trainer flags and their defaults, TrainArgs, and the mapping of an arena
offset to the (first) name of the parameter that holds it.  The kernels are in tests/test_grad_guard_gpu.py."""
import importlib.util
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRAINERS = {"full": "train_mmbart_enc_self_face_name_ids_retrieve_crossattn_bart_guide_match.py",
            "onlyvis": "run_train_mmbart_enc_self_onlyvis_retrieve_crossattn.py"}


def _load(fname):
    spec = importlib.util.spec_from_file_location("trainer_guard_" + fname[:3], os.path.join(ROOT, fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference_flags():
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_trainer_flags.json")))
    by_script = {v["script"]: v for v in ref.values()}
    return {which: by_script[script] for which, script in TRAINERS.items()}


@pytest.mark.parametrize("which", sorted(TRAINERS))
def test_trainer_flags_and_defaults(built_lib, which):
    from vacnic_amd.training import TrainArgs
    assert TrainArgs().skip_nonfinite is False
    mod = _load(TRAINERS[which])
    ref = _reference_flags()[which]
    args = mod.parser.parse_args(ref["argv"])                      # the reference's flag lines parse unchanged, the guard off
    assert args.skip_nonfinite is False and args.max_consecutive_skips == 8
    assert mod.train_args(args, 100).skip_nonfinite is False
    args = mod.parser.parse_args(ref["argv"] + ["--skip_nonfinite", "True", "--max_consecutive_skips", "3"])
    assert args.skip_nonfinite is True and args.max_consecutive_skips == 3
    targs = mod.train_args(args, 100)
    assert targs.skip_nonfinite is True and targs.num_training_steps == 100


class _P:
    def __init__(self, n):
        self.n = n


class _StubArena:
    """the fields arena.first_names / arena.name_at read: slots = {id(p): (offset, numel, capacity)}"""

    def __init__(self, layout):
        self.slots = {id(p): (o, p.n, cap) for p, o, cap in layout}


def test_offset_maps_to_the_first_name_of_its_parameter(built_lib):
    from vacnic_amd.arena import name_at
    emb, w, b = _P(10), _P(6), _P(3)
    # emb: 10 elements in a slot padded to 16 (pad rows); w at 16..21, alignment gap 22..23; b at 24..26, tail up to 32
    arena = _StubArena([(emb, 0, 16), (w, 16, 6), (b, 24, 3)])
    named = [("model.shared.weight", emb), ("model.encoder.embed_tokens.weight", emb), ("fc.weight", w), ("lm_head.weight", emb),
             ("fc.bias", b)]
    assert name_at(arena, named, 0) == "model.shared.weight" and name_at(arena, named, 9) == "model.shared.weight"   # tied: first name
    assert name_at(arena, named, 10) is None and name_at(arena, named, 15) is None          # pad rows
    assert name_at(arena, named, 16) == "fc.weight" and name_at(arena, named, 21) == "fc.weight"
    assert name_at(arena, named, 22) is None and name_at(arena, named, 23) is None          # alignment gap
    assert name_at(arena, named, 24) == "fc.bias" and name_at(arena, named, 26) == "fc.bias"
    assert name_at(arena, named, 27) is None and name_at(arena, named, 31) is None          # the arena's tail
    assert name_at(arena, named, -1) is None


def test_offset_mapping_on_a_host_arena(built_lib):
    """a real (CPU-built) arena: first and last element of every parameter, the padding after the tied embedding, and the name the
    tied LM head / embedding goes by."""
    from vacnic_amd.arena import first_names, name_at
    from vacnic_amd.config import VacnicConfig
    from vacnic_amd.models.mmbart import BartForMultiModalGeneration
    cfg = VacnicConfig(d_model=768, encoder_layers=1, decoder_layers=1, encoder_attention_heads=12, decoder_attention_heads=12,
                       encoder_ffn_dim=3072, decoder_ffn_dim=3072, enc_fusion_layer=[0], dim_common=768, clip_width=768, dropout=0.0)
    m = BartForMultiModalGeneration(cfg, enc_fusion_layer=[0], dim_common=768, prompt_size=cfg.prompt_size).finalize("cpu")
    a = m.arena
    named = list(m.named_parameters(remove_duplicate=False))
    firsts = first_names(a, named)
    assert len(named) > len(firsts), "the model ties weights: some parameter has more than one name"
    covered = torch.zeros(a.n, dtype=torch.bool)
    for name, p in firsts:
        o, n, _ = a.slots[id(p)]
        covered[o:o + n] = True
        assert name_at(a, named, o) == name and name_at(a, named, o + n - 1) == name
    tied = [nm for nm, p in named if p is m.model.shared.weight]
    assert len(tied) > 1 and name_at(a, named, a.slots[id(m.model.shared.weight)][0]) == tied[0]
    gaps = (~covered).nonzero().flatten().tolist()
    assert gaps, "the arena has padding (alignment, padded rows or its tail)"
    for off in (gaps[0], gaps[len(gaps) // 2], gaps[-1]):
        assert name_at(a, named, off) is None


def test_guard_report_needs_the_option(built_lib):
    from vacnic_amd.training import FusedAdamW

    class A:
        device, n = torch.device("cpu"), 8

        def init_optimizer_state(self):
            pass
    opt = FusedAdamW(A(), lr=1e-4)
    assert opt.skip_nonfinite is False and opt.guard is None
    with pytest.raises(RuntimeError, match="skip_nonfinite=False"):
        opt.guard_report()
