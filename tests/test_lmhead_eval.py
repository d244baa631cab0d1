"""CPU: the float64 host model of the fused validation head (vacnic_lmhead_eval; csrc/gemm.hip, the AM epilogue of
gemm_kernel.h), written from the kernel comments, the cases the GPU tests of tests/test_lmhead_eval_gpu.py run, and — the
convention of tests/test_loss_gpu.py — that every deliberately wrong model (a "mutant") lies at least 10x the check's margin
away, or differs exactly where the output is an integer or an exact zero.

The model: logits z = h . E[:V]^T (+ bias) over the V REAL columns only; pred = first maximum; row_nll = lse - z_t, an exact 0 in
rows whose target equals ignore_index; a caption is rows_per_seq consecutive rows; seq_tokens counts its non-ignored rows,
seq_correct those of them with pred == target, seq_nll sums their row_nll; totals = {sum nll, tokens, correct, captions}.

Margins.  row_nll: the margins tests/test_loss_gpu.py derives for the fused path — 8x the deviation of the fp32 restatement on
the same inputs (floored at 1e-6 max|ref|) plus A_lse = 2^-23 (S + 72) + 2^-22 max|lse - max|.  seq_nll: rows_per_seq times that.
pred: fp32 accumulation of a d-term dot product of bf16 operands in any order, then alpha = 1 and one bias addition, is within
a_r = 2 (d + 2) 2^-24 max_j (sum_k |h_rk| |E_jk| + |b_j|) of the float64 logit (gamma_{d+2} at unit roundoff 2^-24, doubled), so a
kernel may only pick a column whose float64 logit is within a_r of the maximum, and must pick the float64 argmax wherever the
float64 top-2 gap exceeds a_r.  The random cases are asserted here to have NO row inside a_r, which makes their integer outputs
exact; the integer case (every logit an exact integer in fp32) carries the ties."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_loss_gpu import (BF16, F32, F64, FUSED_NFAC, assert_sensitive, bound_of, cpu_randint, cpu_randn,  # noqa: E402
                           round_up, span_of)

EVAL_V = [255, 256, 257, 513]
EVAL_RS = [(1, 1), (255, 5), (257, 1), (260, 65)]        # (R, rows_per_seq): both sides of the 256-row tile, one caption across it
CONDITION_SHAPES = [(255, 1, 64), (257, 255, 64), (513, 257, 64), (600, 300, 72), (50265, 64, 64)]     # (V, R, d)
_CASES = {}


def eval_model(z64, tgt, ignore, rps, tie="first", count_ignored=False, shift=0, ignored_nll=False):
    """the outputs of vacnic_lmhead_eval from float64 logits over the real columns.  The keyword arguments build the mutants."""
    z = z64.numpy()
    R = z.shape[0]
    t = tgt.numpy()
    pred = z.argmax(1) if tie == "first" else z.shape[1] - 1 - z[:, ::-1].argmax(1)          # numpy: first occurrence
    lse = torch.logsumexp(z64, -1).numpy()
    valid = t != ignore
    zt = z[np.arange(R), np.where(valid, t, 0)]
    nll = np.where(valid, lse - zt, (lse - z[:, 0]) if ignored_nll else 0.0)
    counted = np.ones(R, bool) if count_ignored else valid
    seq = (np.arange(R) + shift) // rps                          # shift = 1: every caption boundary one row early
    S = R // rps
    seq_nll, seq_tokens, seq_correct = np.zeros(S), np.zeros(S, np.int32), np.zeros(S, np.int32)
    for r in range(R):
        s = min(seq[r], S - 1)
        if counted[r]:
            seq_nll[s] += nll[r]
            seq_tokens[s] += 1
            seq_correct[s] += int(pred[r] == t[r])
    totals = np.array([seq_nll.sum(), seq_tokens.sum(), seq_correct.sum(), S], np.float64)
    return dict(lse=torch.from_numpy(lse), nll=torch.from_numpy(nll), pred=torch.from_numpy(pred.astype(np.int64)),
                seq_nll=torch.from_numpy(seq_nll), seq_tokens=torch.from_numpy(seq_tokens), seq_correct=torch.from_numpy(seq_correct),
                totals=torch.from_numpy(totals))


def argmax_allowance(h, E, bias, V):
    """a_r per row (module docstring)."""
    d = h.shape[1]
    mag = h.to(F64).abs() @ E[:V].to(F64).abs().t()
    if bias is not None:
        mag = mag + bias.to(F64).abs()
    return 2.0 * (d + 2) * 2.0 ** -24 * mag.max(1).values


def top2_gap(z64):
    if z64.shape[1] < 2:
        return torch.full((z64.shape[0],), float("inf"), dtype=F64)
    top = z64.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def place_targets(tgt, pred, V, R, rps, ignore):
    """targets on both sides of every tile edge, at 0 and V - 1, a third of them equal to the prediction, some ignored and — with
    more than one caption — one caption ignored whole."""
    if R == 1:
        tgt[0] = V - 1
        return tgt
    tgt[::3] = pred[::3]
    for i, t in enumerate(t for t in (0, V - 1, 255, 256, 511, 512) if t < V):
        tgt[3 * i + 2] = t
    tgt[7::11] = ignore
    S = R // rps
    if S > 1:
        s = S // 2
        tgt[s * rps:(s + 1) * rps] = ignore
    assert ((tgt == ignore) | ((tgt >= 0) & (tgt < V))).all()
    return tgt


def eval_case(V, R, d, rps, with_bias, ignore=1):
    """inputs built like fused_case of tests/test_loss_gpu.py: h ~ N(0, 1), E ~ 0.3 N(0, 1) with zero pad rows up to
    round_up(V, 32), bias ~ 0.5 N(0, 1) + 0.7, all bf16-rounded (the bias fp32)."""
    key = (V, R, d, rps, with_bias, ignore)
    if key in _CASES:
        return _CASES[key]
    Vp = round_up(V, 32)
    h = cpu_randn(R, d, seed=V * 7 + R)
    E = torch.zeros(Vp, d, dtype=BF16)
    E[:V] = cpu_randn(V, d, seed=V * 11 + R + 1, scale=0.3)
    bias = (cpu_randn(V, seed=5, scale=0.5, dtype=F32) + 0.7) if with_bias else None

    def logits(dt):
        z = h.to(dt) @ E[:V].to(dt).t()
        return z if bias is None else z + bias.to(dt)
    z64, z32 = logits(F64), logits(F32)
    tgt = place_targets(cpu_randint(0, V, (R,), seed=V + R), z64.argmax(1), V, R, rps, ignore)
    S, lmax = span_of(z64)
    c = dict(V=V, R=R, d=d, rps=rps, ignore=ignore, Vp=Vp, h=h, E=E, bias=bias, tgt=tgt, z64=z64, z32=z32,
             m64=eval_model(z64, tgt, ignore, rps), m32=eval_model(z32.to(F64), tgt, ignore, rps),
             a_lse=2.0 ** -23 * (S + FUSED_NFAC) + 2.0 ** -22 * lmax, a_r=argmax_allowance(h, E, bias, V), gap=top2_gap(z64))
    _CASES[key] = c
    return c


def row_margin(c):
    """the scalar margin of row_nll at this case (8x the fp32 deviation, floored, plus A_lse)."""
    return bound_of(c["m64"]["nll"], c["m32"]["nll"], extra=c["a_lse"])[0]


EXACT_PAIRS = [(0, 255), (255, 256), (256, None)]        # None: V - 1


def exact_case(V, pair, with_bias, rps=8, R=64, d=64, ignore=1):
    """h, E integers in [-2, 2]: every logit is an exact integer in fp32 (|z| <= 4 d + 3 < 2^24), so the kernel's argmax must be
    THE first maximum.  Column 0 of E is 2 in every real row, so rows with h = (-2, one entry of -1 / 0 / 1 elsewhere) have only
    negative logits (-4 +- 2, and -4 +- 2 + b_j with the integer bias b_j in [-2, 0]): a zero pad column would win there.  Columns
    `pair` hold the same vector u (entries +-2, equal bias), and rows 0..3 are u itself: their maximum 4 d sits in both columns at
    once.  Row 20 is column 1's own vector and its target is ignore_index = 1: an ignored row whose prediction equals its target."""
    a, b = pair
    b = V - 1 if b is None else b
    key = ("exact", V, a, b, with_bias)
    if key in _CASES:
        return _CASES[key]
    Vp = round_up(V, 32)
    h = cpu_randint(-2, 3, (R, d), seed=V + 3 * a).to(BF16)
    E = torch.zeros(Vp, d, dtype=BF16)
    E[:V] = cpu_randint(-2, 3, (V, d), seed=V + 5 * a + 1).to(BF16)
    E[:V, 0] = 2.0
    u = (cpu_randint(0, 2, (d,), seed=17 + a) * 4 - 2).to(BF16)
    u[0] = 2.0
    if a != b:
        E[a] = u
        E[b] = u
        h[0:4] = u
    u1 = (cpu_randint(0, 2, (d,), seed=31 + a) * 4 - 2).to(BF16)
    u1[0] = 2.0
    E[1] = u1
    h[20] = u1
    h[8:16] = 0.0
    h[8:16, 0] = -2.0
    for i in range(8, 16):
        h[i, 1 + i] = float(i % 3 - 1)
    bias = (cpu_randint(-2, 1, (V,), seed=23).to(F32)) if with_bias else None
    if bias is not None:
        bias[b] = bias[a]
    z64 = h.to(F64) @ E[:V].to(F64).t()
    if bias is not None:
        z64 = z64 + bias.to(F64)
    tgt = place_targets(cpu_randint(0, V, (R,), seed=V + a), z64.argmax(1), V, R, rps, ignore)
    tgt[20] = ignore
    zp = torch.cat([z64, torch.zeros(R, Vp - V, dtype=F64)], 1)        # what the pad columns [V, round_up(V, 32)) would hold
    c = dict(V=V, R=R, d=d, rps=rps, ignore=ignore, Vp=Vp, h=h, E=E, bias=bias, tgt=tgt, z64=z64, zpad=zp, pair=(a, b),
             m64=eval_model(z64, tgt, ignore, rps))
    _CASES[key] = c
    return c


# --------------------------------------------------------------------------------------------------------------- the tests
def test_model_is_torch_on_a_case_without_ties():
    c = eval_case(257, 255, 64, 5, True)
    z, tgt, m = c["z64"], c["tgt"], c["m64"]
    assert torch.equal(m["pred"], torch.argmax(z, 1))
    nll = torch.nn.functional.cross_entropy(z, tgt, ignore_index=1, reduction="none")
    assert torch.allclose(m["nll"], nll, rtol=1e-12, atol=1e-12) and (m["nll"][tgt == 1] == 0).all()
    assert int(m["totals"][1]) == int((tgt != 1).sum()) and int(m["totals"][3]) == 51
    assert int(m["totals"][2]) == int(((m["pred"] == tgt) & (tgt != 1)).sum()) > 50
    assert (m["seq_tokens"] == 0).any(), "one caption is ignored whole"
    assert (m["seq_nll"][m["seq_tokens"] == 0] == 0).all()


@pytest.mark.parametrize("V,R,d", CONDITION_SHAPES)
def test_no_row_of_the_random_cases_is_undecided(V, R, d):
    """the condition of the GPU argmax check: with these inputs no float64 top-2 gap lies within a_r, so pred — and with it
    seq_correct and totals — has ONE admissible value."""
    for with_bias in (False, True):
        c = eval_case(V, R, d, 1, with_bias)
        if V > 1:
            print(f"EVALCOND V={V} R={R} d={d} bias={with_bias} min gap={c['gap'].min().item():.3e} max a_r={c['a_r'].max().item():.3e}")
        assert (c["gap"] > c["a_r"]).all()


@pytest.mark.parametrize("V", EVAL_V)
@pytest.mark.parametrize("R,rps", EVAL_RS)
def test_gpu_cases_are_decided_and_cover_the_edges(V, R, rps):
    for with_bias in (False, True):
        c = eval_case(V, R, 64, rps, with_bias)
        assert (c["gap"] > c["a_r"]).all()
        if R > 1:
            t = c["tgt"]
            assert (t == 0).any() and (t == V - 1).any() and (t == 1).any()
            assert V <= 256 or ((t == 255).any() and (t == 256).any())
            assert (c["m64"]["seq_tokens"] == 0).any() and c["m64"]["totals"][2] > 0


def test_the_d72_gpu_case_is_decided():
    c = eval_case(257, 36, 72, 4, True)
    assert (c["gap"] > c["a_r"]).all() and (c["m64"]["seq_tokens"] == 0).any()


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("V", [513, 257])
def test_exact_cases_hold_the_ties_and_the_negative_rows(V, with_bias):
    tied_rows = 0
    for pair in EXACT_PAIRS:
        c = exact_case(V, pair, with_bias)
        z, (a, b) = c["z64"], c["pair"]
        assert torch.equal(z, z.round()) and z.abs().max() < 2 ** 24
        assert torch.equal((c["h"].float() @ c["E"][:V].float().t() + (0 if c["bias"] is None else c["bias"])).to(F64), z), "exact in fp32"
        assert torch.equal(c["m64"]["pred"], torch.argmax(z, 1)), "torch.argmax on the CPU is the first maximum too"
        if a != b:
            mx = z[0:4].max(1).values
            assert (z[0:4, a] == mx).all() and (z[0:4, b] == mx).all() and (c["m64"]["pred"][0:4] == a).all()
        assert (z[8:16] < 0).all(), "rows with only negative real logits"
        assert c["m64"]["pred"][20] == 1 and c["tgt"][20] == 1
        tied_rows += int((top2_gap(z[21:]) == 0).sum())
    assert tied_rows >= 3, "ties beyond the planted ones"


def test_mutants_are_caught():
    # value outputs: a dropped last column, a shifted caption boundary
    for V, R, rps in [(257, 255, 5), (513, 260, 65)]:
        c = eval_case(V, R, 64, rps, True)
        m64, m32, tgt = c["m64"], c["m32"], c["tgt"]
        cut = eval_model(c["z64"][:, :V - 1], tgt.clamp(max=V - 2), 1, rps)
        assert_sensitive("last column dropped: row_nll", m64["nll"], m32["nll"], cut["nll"], extra=c["a_lse"])
        shifted = eval_model(c["z64"], tgt, 1, rps, shift=1)
        assert ((shifted["seq_nll"] - m64["seq_nll"]).abs().max() >= 10 * rps * row_margin(c))
        assert not torch.equal(shifted["seq_tokens"], m64["seq_tokens"])
        counted = eval_model(c["z64"], tgt, 1, rps, count_ignored=True)
        assert not torch.equal(counted["seq_tokens"], m64["seq_tokens"]) and counted["totals"][1] != m64["totals"][1]
        leak = eval_model(c["z64"], tgt, 1, rps, ignored_nll=True)
        assert (leak["nll"][tgt == 1] != 0).all() and (m64["nll"][tgt == 1] == 0).all()
    # integer outputs on the exact cases: ties to the highest index, pad columns admitted, ignored rows counted as correct
    for with_bias in (False, True):
        for pair in EXACT_PAIRS:
            c = exact_case(513, pair, with_bias)
            m64 = c["m64"]
            last = eval_model(c["z64"], c["tgt"], 1, c["rps"], tie="last")
            assert not torch.equal(last["pred"], m64["pred"]) and not torch.equal(last["seq_correct"], m64["seq_correct"])
            padded = eval_model(c["zpad"], c["tgt"], 1, c["rps"])
            assert (padded["pred"][8:16] >= c["V"]).all() and (m64["pred"][8:16] < c["V"]).all()
            counted = eval_model(c["z64"], c["tgt"], 1, c["rps"], count_ignored=True)
            assert not torch.equal(counted["seq_correct"], m64["seq_correct"]) and not torch.equal(counted["seq_tokens"], m64["seq_tokens"])


def test_trainers_have_the_eval_fused_flag_off_by_default():
    import importlib.util
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ref = json.load(open(os.path.join(root, "tests", "golden", "reference_trainer_flags.json")))
    for which, script in (("run_full_train", "train_mmbart_enc_self_face_name_ids_retrieve_crossattn_bart_guide_match.py"),
                          ("run_onlyvis_train", "run_train_mmbart_enc_self_onlyvis_retrieve_crossattn.py")):
        spec = importlib.util.spec_from_file_location(f"trainer_{which}", os.path.join(root, script))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        argv = ref[which]["argv"]                                  # the reference's own flag line parses unchanged
        assert mod.parser.parse_args(argv).eval_fused is False
        assert mod.parser.parse_args(argv + ["--eval_fused", "True"]).eval_fused is True
        assert mod.parser.parse_args(argv + ["--eval_fused", "False"]).eval_fused is False
    for doc in ("README.md", "INTEGRATION.md"):
        assert "--eval_fused" in open(os.path.join(root, doc)).read()
