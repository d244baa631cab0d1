"""CPU: the host side of the weighted LM-head loss and of self-critical training — caption rows to labels, advantages, the stand-in
reward, the argument checks that run before any library call, and the trainers' flags.  Nothing here needs a device."""
import importlib.util
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAINERS = {"full": "train_mmbart_enc_self_face_name_ids_retrieve_crossattn_bart_guide_match.py",
            "onlyvis": "run_train_mmbart_enc_self_onlyvis_retrieve_crossattn.py"}
PAD, EOS, START = 1, 2, 2


def _load(script):
    spec = importlib.util.spec_from_file_location("trainer_" + script.split(".")[0], os.path.join(ROOT, script))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ sequences_to_labels
def test_sequences_to_labels_rows(built_lib):
    """Rule for a pad id before the eos: it stays where it is — it does not end the caption, and as the ignore index that one
    position carries no loss; everything strictly behind the first eos (searched behind the start token, which is itself the eos id
    here) is pad."""
    from vacnic_amd.training import sequences_to_labels
    seqs = torch.tensor([[START, 5, 6, 7, EOS],          # eos in the last column
                         [START, 5, 6, 7, 8],            # no eos at all: every token is kept
                         [START, EOS, PAD, PAD, PAD],    # eos first
                         [START, 5, PAD, 6, EOS],        # a pad id before the eos
                         [START, 5, EOS, 9, 9]])         # (not what generate() writes) ids behind the first eos are dropped
    dec_in, labels = sequences_to_labels(seqs, PAD, EOS)             # T = L - 1
    assert labels.tolist() == [[5, 6, 7, EOS], [5, 6, 7, 8], [EOS, PAD, PAD, PAD], [5, PAD, 6, EOS], [5, EOS, PAD, PAD]]
    assert dec_in.tolist() == [[START, 5, 6, 7], [START, 5, 6, 7], [START, EOS, PAD, PAD], [START, 5, PAD, 6], [START, 5, EOS, PAD]]
    assert dec_in.is_contiguous() and labels.is_contiguous() and labels.dtype == seqs.dtype
    # shift right: decoder input = start token, then the labels without their last column
    assert torch.equal(dec_in[:, 1:], labels[:, :-1]) and (dec_in[:, 0] == START).all()


def test_sequences_to_labels_widths(built_lib):
    from vacnic_amd.training import sequences_to_labels
    seqs = torch.tensor([[START, 5, EOS], [START, EOS, PAD]])
    d6, l6 = sequences_to_labels(seqs, PAD, EOS, T=6)                # L < T + 1: padded to the fixed width
    assert l6.tolist() == [[5, EOS, PAD, PAD, PAD, PAD], [EOS, PAD, PAD, PAD, PAD, PAD]]
    assert d6.tolist() == [[START, 5, EOS, PAD, PAD, PAD], [START, EOS, PAD, PAD, PAD, PAD]]
    d2, l2 = sequences_to_labels(seqs, PAD, EOS, T=2)                # L == T + 1
    assert l2.tolist() == [[5, EOS], [EOS, PAD]] and d2.tolist() == [[START, 5], [START, EOS]]
    with pytest.raises(ValueError, match="do not fit"):
        sequences_to_labels(seqs, PAD, EOS, T=1)
    with pytest.raises(ValueError, match="rows, L >= 2"):
        sequences_to_labels(seqs[:, :1], PAD, EOS)


# ------------------------------------------------------------------------------------------------ group_advantages
def test_group_advantages_exact_values(built_lib):
    from vacnic_amd.training import group_advantages
    r = [1.0, 2.0, 3.0, 6.0]
    assert group_advantages(r, 2).tolist() == [-0.5, 0.5, -1.5, 1.5]
    assert group_advantages(r, 4).tolist() == [-2.0, -1.0, 0.0, 3.0]
    assert group_advantages(r, 2, "leave_one_out").tolist() == [-1.0, 1.0, -3.0, 3.0]
    got = group_advantages(r, 4, "leave_one_out")
    want = torch.tensor([1 - 11 / 3, 2 - 10 / 3, 3 - 9 / 3, 6 - 6 / 3], dtype=torch.float64).float()
    assert torch.equal(got, want) and got.dtype == torch.float32
    g = torch.Generator().manual_seed(0)
    a = group_advantages(torch.rand(24, generator=g).tolist(), 4)
    assert a.view(-1, 4).double().sum(1).abs().max().item() <= 4 * 2.0 ** -24       # "mean" sums to 0 per group (fp32 rounding of 4 terms)
    with pytest.raises(ValueError, match="at least 2"):
        group_advantages(r, 1)
    with pytest.raises(ValueError, match="groups of"):
        group_advantages(r, 3)
    with pytest.raises(ValueError, match="baseline"):
        group_advantages(r, 2, "greedy")


# ------------------------------------------------------------------------------------------------ overlap_f1_reward
def test_overlap_f1_reward(built_lib):
    from vacnic_amd.training import overlap_f1_reward
    sp = (PAD, EOS)
    assert overlap_f1_reward([[START, 5, 6, 7, EOS, PAD]], [[5, 6, 7, EOS]], sp) == [1.0]                  # identical
    assert overlap_f1_reward([[5, 6, 7]], [[8, 9]], sp) == [0.0]                                         # disjoint
    # clipping: 5 occurs three times in the sample, once in the reference -> overlap 1; p = 1/3, r = 1/2, F1 = 2 (1/6) / (5/6) = 0.4
    assert overlap_f1_reward([[5, 5, 5]], [[5, 6]], sp) == [pytest.approx(0.4, abs=1e-12)]
    # specials excluded from both sides: without them the pair is disjoint although pad / eos coincide
    assert overlap_f1_reward([[START, 5, EOS, PAD, PAD]], [[6, EOS, PAD]], sp) == [0.0]
    assert overlap_f1_reward([[START, 5, EOS, PAD, PAD]], [[6, EOS, PAD]]) [0] > 0.0
    assert overlap_f1_reward([[START, EOS, PAD]], [[5, 6]], sp) == [0.0]                                  # empty sample
    assert overlap_f1_reward([[]], [[5, 6]], sp) == [0.0]
    assert overlap_f1_reward([[5, 6], [7]], [[5, 6], [8]], sp) == [1.0, 0.0]                              # one float per pair
    with pytest.raises(ValueError, match="references"):
        overlap_f1_reward([[5]], [[5], [6]], sp)


# ------------------------------------------------------------------------------------------------ checks before any library call
def test_weight_validation_needs_no_device(built_lib):
    """every refusal names the offending value and is raised before a pointer is taken: the tensors here live on the host, where a
    library call would be a RuntimeError ("no CPU fallback"), not a ValueError."""
    from vacnic_amd import kernels as K, ops
    R, T, d, V = 16, 8, 32, 100
    h = torch.zeros(R, d, dtype=torch.bfloat16)
    E = torch.zeros(128, d, dtype=torch.bfloat16)
    tgt = torch.zeros(R, dtype=torch.int64)
    w = torch.ones(R)
    lse, acc = torch.zeros(R), torch.zeros(4)

    def fwd(weights, rpw=1, norm="tokens"):
        K.lmhead_ce_fwd_weighted(h, E, tgt, V, weights, rpw, norm)

    def op(weights, rpw=1, norm="tokens"):
        ops.lm_head_ce(h.view(2, T, d), None, E, None, tgt.view(2, T), V, 1, weights=weights, rows_per_weight=rpw, norm=norm)

    def rowp(weights, rpw=1, norm="tokens"):
        K.lmhead_ce_rowp(lse, tgt, acc, weights=weights, rows_per_weight=rpw)

    for call in (fwd, op, rowp):
        with pytest.raises(ValueError, match="float64"):
            call(w.double())
        with pytest.raises(ValueError, match="float32 tensor, got list"):
            call([1.0] * R)
        with pytest.raises(ValueError, match="meta"):
            call(torch.ones(R, device="meta"))
        with pytest.raises(ValueError, match=r"contiguous, got strides \(2,\)"):
            call(torch.ones(2 * R)[::2])
        with pytest.raises(ValueError, match=f"hold {R - 1} elements"):
            call(torch.ones(R - 1))
        with pytest.raises(ValueError, match="hold 16 elements.*need 2"):
            call(w, T)                                               # per-caption stride with per-token weights
        with pytest.raises(ValueError, match="rows_per_weight=3"):
            call(torch.ones(5), 3)                                   # 16 rows are no whole number of 3-row captions
        with pytest.raises(ValueError, match="rows_per_weight=0"):
            call(w, 0)
    for call in (fwd, op):
        with pytest.raises(ValueError, match="norm='sum'"):
            call(w, 1, "sum")
    with pytest.raises(ValueError, match="norm='sum'"):
        ops.lm_head_ce(h.view(2, T, d), None, E, None, tgt.view(2, T), V, 1, norm="sum")          # checked without weights too
    # what is valid gets past the checks and fails at the first pointer: there is no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback|need"):
        fwd(torch.ones(2), T, "weights")
    assert K.LOSS_NORMS == {"tokens": 0, "weights": 1}


def test_model_forward_refuses_before_anything_runs(built_lib):
    from vacnic_amd.config import VacnicConfig
    from vacnic_amd.models.mmbart import BartForMultiModalGeneration
    cfg = VacnicConfig(d_model=768, encoder_layers=1, decoder_layers=1, encoder_attention_heads=12, decoder_attention_heads=12,
                       encoder_ffn_dim=768, decoder_ffn_dim=768, enc_fusion_layer=[0], dim_common=768, clip_width=768, vocab_size=128)
    model = BartForMultiModalGeneration(cfg)
    model.arena = object()                                           # (the checks under test come before any use of it)
    labels = torch.full((2, 8), 5)
    with pytest.raises(ValueError, match="pass labels="):
        model(loss_weights=torch.ones(2))
    with torch.no_grad():
        with pytest.raises(ValueError, match="output_token_stats"):
            model(labels=labels, loss_weights=torch.ones(2), output_token_stats=True)
    with pytest.raises(ValueError, match=r"shape \(3,\)"):
        model(labels=labels, loss_weights=torch.ones(3))
    with pytest.raises(ValueError, match=r"shape \(2, 7\)"):
        model(labels=labels, loss_weights=torch.ones(2, 7))


# ------------------------------------------------------------------------------------------------ step-level refusals, flags
def test_recorded_steps_refuse_a_batch_of_the_other_kind(built_lib):
    from vacnic_amd.training import _same_loss_weights_key
    plain, weighted = {"caption_ids": 0}, {"caption_ids": 0, "loss_weights": torch.ones(2)}
    _same_loss_weights_key("PlannedTrainStep", plain, plain)
    _same_loss_weights_key("PlannedTrainStep", weighted, weighted)
    with pytest.raises(ValueError, match="recorded with batch.*called without"):
        _same_loss_weights_key("PlannedTrainStep", weighted, plain)
    with pytest.raises(ValueError, match="recorded without batch.*called with"):
        _same_loss_weights_key("GraphedTrainStep", plain, weighted)


def test_self_critical_step_refusals_need_no_device(built_lib):
    from vacnic_amd.ddp import DistributedDataParallel
    from vacnic_amd.training import TrainArgs, self_critical_step

    class Opt:
        accum_steps = 1
    wrapped = DistributedDataParallel.__new__(DistributedDataParallel)          # (isinstance is all the check looks at)
    with pytest.raises(ValueError, match="one process"):
        self_critical_step(wrapped, Opt(), {}, TrainArgs())
    with pytest.raises(ValueError, match="grad_accum_steps 2"):
        self_critical_step(object(), Opt(), {}, TrainArgs(grad_accum_steps=2))
    two = Opt()
    two.accum_steps = 2
    with pytest.raises(ValueError, match="grad_accum_steps 2"):
        self_critical_step(object(), two, {}, TrainArgs())
    with pytest.raises(ValueError, match="at least 2"):
        self_critical_step(object(), Opt(), {}, TrainArgs(), n_samples=1)


@pytest.mark.parametrize("which", sorted(TRAINERS))
def test_trainer_flags(built_lib, which):
    from vacnic_amd.training import TrainArgs, check_scst_flags
    assert TrainArgs().loss_norm == "tokens"
    mod = _load(TRAINERS[which])
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_trainer_flags.json")))
    argv = {v["script"]: v for v in ref.values()}[TRAINERS[which]]["argv"]
    args = mod.parser.parse_args(argv)                              # the reference's flag lines parse unchanged, everything off
    assert (args.scst_samples, args.scst_ce_weight, args.scst_temperature, args.scst_top_k, args.scst_top_p, args.scst_baseline,
            args.loss_norm) == (0, 0.0, 1.0, 0, 1.0, "mean", "tokens")
    assert mod.train_args(args, 100).loss_norm == "tokens"
    args = mod.parser.parse_args(argv + ["--scst_samples", "4", "--scst_ce_weight", "0.25", "--scst_temperature", "0.8", "--scst_top_k", "50",
                                         "--scst_top_p", "0.9", "--scst_baseline", "leave_one_out", "--loss_norm", "weights"])
    assert (args.scst_samples, args.scst_ce_weight, args.scst_temperature, args.scst_top_k, args.scst_top_p, args.scst_baseline) == \
        (4, 0.25, 0.8, 50, 0.9, "leave_one_out")
    assert mod.train_args(args, 100).loss_norm == "weights"
    with pytest.raises(ValueError, match="--scst_samples 4 with --grad_accum_steps 2"):
        mod.train_args(mod.parser.parse_args(argv + ["--scst_samples", "4", "--grad_accum_steps", "2"]), 100)
    mod.train_args(mod.parser.parse_args(argv + ["--grad_accum_steps", "2"]), 100)                  # accumulation alone stays fine
    with pytest.raises(ValueError, match="world_size 2"):
        check_scst_flags(4, 1, 2)
    with pytest.raises(ValueError, match="at least 2"):
        check_scst_flags(1)
    check_scst_flags(0, 4, 8)                                       # off: nothing to refuse
    with pytest.raises(SystemExit):
        mod.parser.parse_args(argv + ["--loss_norm", "sum"])


def test_documents_name_the_flags():
    for doc in ("README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for flag in ("--scst_samples", "--loss_norm"):
            assert flag in text, (doc, flag)
    assert "vacnic_lmhead_ce_wloss" in open(os.path.join(ROOT, "DESIGN.md")).read()
