"""CPU: the host side of the deterministic mode — the switch, TrainArgs, the trainers' --deterministic flag, the documents that
name it, the host-side sizing of the ordered bias gradient and the refusals that need no GPU.  The kernels and the step are in
tests/test_deterministic_gpu.py."""
import importlib.util
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRAINERS = {"full": "train_mmbart_enc_self_face_name_ids_retrieve_crossattn_bart_guide_match.py",
            "onlyvis": "run_train_mmbart_enc_self_onlyvis_retrieve_crossattn.py"}


def _load(fname):
    spec = importlib.util.spec_from_file_location("trainer_det_" + fname[:3], os.path.join(ROOT, fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_switch_is_off_by_default_and_restores(built_lib):
    from vacnic_amd import kernels as K
    from vacnic_amd import ops
    assert ops.deterministic() is False and K.DETERMINISTIC is False
    ops.set_deterministic(True)
    try:
        assert ops.deterministic() is True
        with ops.deterministic_mode(False):
            assert ops.deterministic() is False
        assert ops.deterministic() is True
    finally:
        ops.set_deterministic(False)
    with pytest.raises(RuntimeError):
        with ops.deterministic_mode():
            assert ops.deterministic() is True
            raise RuntimeError("inside")
    assert ops.deterministic() is False


@pytest.mark.parametrize("which", sorted(TRAINERS))
def test_trainers_parse_deterministic(built_lib, which):
    from vacnic_amd.training import TrainArgs
    assert TrainArgs().deterministic is False
    mod = _load(TRAINERS[which])
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_trainer_flags.json")))
    ref = {v["script"]: v for v in ref.values()}[TRAINERS[which]]
    args = mod.parser.parse_args(ref["argv"])                      # the reference's flag lines parse unchanged, the mode off
    assert args.deterministic is False and mod.train_args(args, 100).deterministic is False
    args = mod.parser.parse_args(ref["argv"] + ["--deterministic", "True"])
    assert args.deterministic is True
    targs = mod.train_args(args, 100)
    assert targs.deterministic is True and targs.num_training_steps == 100
    assert mod.parser.parse_args(ref["argv"] + ["--deterministic", "False"]).deterministic is False


def test_documents_name_the_flag():
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "--deterministic" in open(os.path.join(ROOT, doc)).read(), doc


def test_bias_partials_sizing(built_lib):
    """rows of the partials scratch: clamp(ceil(M / 64), 1, 256) — a function of M alone."""
    from vacnic_amd import kernels as K
    for M, want in [(0, 1), (1, 1), (64, 1), (65, 2), (1000, 16), (16384, 256), (16385, 256), (1 << 20, 256)]:
        assert K.bias_grad_ordered_rows(M) == want, M


def test_struct_tail_defaults_to_the_old_behaviour(built_lib):
    from vacnic_amd import _lib
    names = [f[0] for f in _lib.AddLnBwdArgs._fields_]
    assert names[-2:] == ["defer_fold", "partials_any"]
    assert _lib.AddLnBwdArgs().partials_any == 0


def test_bad_arguments_return_status(built_lib):
    """validation before any launch: status + message, no GPU needed."""
    from vacnic_amd import _lib
    with pytest.raises(ValueError, match="fold_ordered"):
        _lib.call("vacnic_fold_ordered", 16, 8, None, None, 4, 8, None)
    with pytest.raises(ValueError, match="fold_ordered: ld="):
        _lib.call("vacnic_fold_ordered", 16, 4, 16, None, 4, 8, None)
    with pytest.raises(ValueError, match="bias_grad_ordered: null operand"):
        _lib.call("vacnic_bias_grad_ordered", None, 16, 4, 8, 8, 16, 1, None)
    with pytest.raises(ValueError, match="16-byte aligned"):
        _lib.call("vacnic_bias_grad_ordered", 16, 16, 4, 8, 12, 16, 1, None)
    with pytest.raises(ValueError, match="scatter_ordered"):
        _lib.call("vacnic_scatter_ordered", 16, 16, 16, None, 4, 4, 10, 8, 2, 1, 1.0, None)
    with pytest.raises(ValueError, match="sum_ordered"):
        _lib.call("vacnic_sum_ordered", None, 4, 16, None)
    with pytest.raises(ValueError, match="lmhead_row_loss"):
        _lib.call("vacnic_lmhead_row_loss", 16, 16, 16, None, 4, 300, 2, 1, 0.1, 16, None)
    with pytest.raises(ValueError, match="embed_ln_bwd_ordered: null operand"):
        _lib.call("vacnic_embed_ln_bwd_ordered", _lib.C.byref(_lib.EmbedLnBwdArgs()), None, None, 0, None)
