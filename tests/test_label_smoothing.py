"""Label smoothing, host side: the trainers' flag, the config field (and checkpoints written before it existed), the C structs."""
import importlib.util
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRAINERS = ["train_mmbart_enc_self_face_name_ids_retrieve_crossattn_bart_guide_match.py",
            "run_train_mmbart_enc_self_onlyvis_retrieve_crossattn.py"]


def _load(fname):
    spec = importlib.util.spec_from_file_location("trainer_under_test_" + fname[:3], os.path.join(ROOT, fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("fname", TRAINERS)
def test_trainers_parse_label_smoothing_and_carry_it_into_the_config(fname, built_lib):
    mod = _load(fname)
    build_config = mod.build_config
    base = ["--enc_fusion_layer", "0", "1"]
    args = mod.parser.parse_args(base)
    assert args.label_smoothing == 0.0
    cfg, _ = build_config(args)
    assert cfg.label_smoothing == 0.0
    args = mod.parser.parse_args(base + ["--label_smoothing", "0.1"])
    assert args.label_smoothing == pytest.approx(0.1)
    cfg, _ = build_config(args)
    assert cfg.label_smoothing == pytest.approx(0.1)
    assert dict(cfg.__dict__)["label_smoothing"] == pytest.approx(0.1), "what the trainer stores as the checkpoint's meta.config"
    with pytest.raises(ValueError, match="label_smoothing"):
        build_config(mod.parser.parse_args(base + ["--label_smoothing", "1.0"]))


def test_meta_config_without_the_field_loads_with_zero(built_lib):
    from vacnic_amd.config import VacnicConfig
    old = dict(VacnicConfig().__dict__)
    del old["label_smoothing"]                          # a checkpoint written before the field existed
    cfg = VacnicConfig(**old).validate()
    assert cfg.label_smoothing == 0.0
    new = VacnicConfig(**dict(VacnicConfig(label_smoothing=0.1).__dict__)).validate()
    assert new.label_smoothing == pytest.approx(0.1)
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="label_smoothing"):
            VacnicConfig(label_smoothing=bad).validate()


def test_c_structs_expose_label_smoothing_last(built_lib):
    """appended at the end, so that code written against the older header still compiles and a zero-initialised struct means "no
    smoothing".  (tests/test_abi.py checks the layout against the header.)"""
    import ctypes as C
    from vacnic_amd import _lib
    for st in (_lib.LmheadCeArgs, _lib.CeArgs):
        name, typ = st._fields_[-1][:2]
        assert name == "label_smoothing" and typ is C.c_float, st._fields_[-1]
        assert st().label_smoothing == 0.0
    names = [f[0] for f in _lib.LmheadCeArgs._fields_]
    assert names[-3:] == ["ignore_index", "part_sum", "label_smoothing"]
    assert [f[0] for f in _lib.CeArgs._fields_][-2:] == ["logits_f32", "label_smoothing"]
    assert "vacnic_lmhead_ce_rowp_smooth" in _lib.EXPORTED
