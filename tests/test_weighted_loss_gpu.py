"""Per-row weights on the fused LM-head cross entropy on the MI355X, and what is built on them:

    loss = sum_r w_r l_r / N,   dz_rj = w_r / N (softmax_j - (1 - eps) [j == t_r] - eps / V)

with w_r = weights[r // rows_per_weight] (any sign), l_r the row's unweighted term and N the number of non-ignored rows (norm
"tokens") or the sum of their weights (norm "weights").  Kernels (vacnic_lmhead_ce_wloss, vacnic_lmhead_ce_rowp_w) against float64
torch and, bit for bit, against the unweighted calls; then ops.lm_head_ce(weights=), model(loss_weights=), the train step's batch
key, a launch plan recorded with the key, and training.self_critical_step.

Tolerances are the ones tests/test_label_smoothing_gpu.py gates on: LOSS_RTOL = 2e-3 (relative to the ABSOLUTE mass sum |w l| / |N|
here, because signed terms cancel), row lse / row loss rtol 1e-4 + atol 2e-3, dlogits rtol 2e-2, planned-vs-eager rtol 2e-3 +
atol 1e-4."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOSS_RTOL = 2e-3
SHAPES = [(5, 1000, 128),         # fewer rows than one 4-wave block, fewer than 256 strands
          (64, 1000, 128),
          (300, 50267, 256)]      # more than 256 strands; 197 tiles (> 64 lanes), ragged last tile and chunk
EPS = [0.0, 0.3]
NORMS = ["tokens", "weights"]
CH = 16384                        # ops.LMHEAD_CHUNK
IGN = 1


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


def rnd(*shape, scale=1.0, dtype=torch.bfloat16, seed=0, device="cuda"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(device).to(dtype)


def close(a, b, rtol, atol, what=""):
    a = a.double(); b = b.double()
    err = (a - b).abs()
    bound = atol + rtol * b.abs()
    bad = (err > bound).sum().item()
    assert bad == 0, f"{what}: {bad}/{a.numel()} off; max err {err.max().item():.4g} (ref max {b.abs().max().item():.4g})"


def make_inputs(R, V, d, device="cuda"):
    """h, the tied matrix (its pad rows zero), float64 logits, targets and weights of one shape.  Targets: random ids, every second
    row aims at its arg-max logit (a small loss term), every 7th row ignored, ids V - 1 and 0 present.  Weights: seeded normal
    values, hence signed, pushed out to |w| >= 0.25 (so that the smallest coefficient that must show in dlogits is known), and an
    exact 0 on every 4th row — those are arg-max rows, so leaving them out moves the weighted mean away from the plain one."""
    Vp = (V + 31) // 32 * 32
    h = rnd(R, d, seed=1, device=device)
    E = torch.zeros(Vp, d, device=device, dtype=torch.bfloat16)
    E[:V] = rnd(V, d, scale=0.08, seed=2, device=device)
    logits = h.double() @ E[:V].double().t()
    tgt = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(3)).to(device)
    tgt[::2] = logits[::2].argmax(-1)
    tgt[::7] = IGN; tgt[1] = V - 1; tgt[3] = 0
    w = torch.randn(R, generator=torch.Generator().manual_seed(4))
    w = torch.where(w.abs() < 0.25, torch.where(w < 0, -0.25, 0.25), w.double()).float()
    w[::4] = 0.0
    return dict(h=h, E=E, Vp=Vp, logits=logits, tgt=tgt, w=w.to(device))


def reference(c, eps, norm):
    """float64: per-row terms, weighted loss, N, the bound's scale sum |w l| / |N|, and the unweighted mean"""
    tgt, valid = c["tgt"], (c["tgt"] != IGN).double()
    rows = F.cross_entropy(c["logits"], tgt, reduction="none", ignore_index=IGN, label_smoothing=eps) * valid
    w = (c["w"].abs() if norm == "weights" else c["w"]).double()
    N = (valid.sum() if norm == "tokens" else (w * valid).sum()).item()
    return dict(rows=rows, w=w, N=N, loss=((w * rows).sum() / N).item(), scale=((w * rows).abs().sum() / abs(N)).item(),
                plain=(rows.sum() / valid.sum()).item(), valid=valid)


def assert_sensitive(ref):
    """on the reference alone: the weighted and the unweighted loss are at least 10 tolerances apart, or the loss check shows nothing"""
    print(f"reference: weighted {ref['loss']:.6f} plain {ref['plain']:.6f} scale {ref['scale']:.6f} N {ref['N']:.6f}")
    assert abs(ref["loss"] - ref["plain"]) >= 10 * LOSS_RTOL * ref["scale"], (ref["loss"], ref["plain"], ref["scale"])


_CASES = {}


def case(R, V, d):
    """inputs and float64 references of one shape, computed once and left unchanged"""
    if (R, V, d) not in _CASES:
        c = make_inputs(R, V, d)
        c["ref"] = {(eps, norm): reference(c, eps, norm) for eps in EPS for norm in NORMS}
        c["soft"] = torch.softmax(c["logits"], -1)
        _CASES[(R, V, d)] = c
    return _CASES[(R, V, d)]


def chunks(V):
    for c0 in range(0, V, CH):
        n = min(CH, V - c0)
        yield c0, n, (n + 7) // 8 * 8


def dlogits_chunks(K, c, V, rowp, eps):
    """every vocabulary chunk of dlogits as the backward produces them: [(c0, n, n8, bf16 [R, n8] copy)]"""
    R = c["h"].shape[0]
    dl = torch.full((R, CH), 9.0, device="cuda", dtype=torch.bfloat16)
    out = []
    for c0, n, n8 in chunks(V):
        K.lmhead_ce_dlogits(c["h"], c["E"], c["tgt"], V, rowp, dl, c0, n, ignore_index=IGN, label_smoothing=eps)
        out.append((c0, n, n8, dl[:, :n8].clone()))
    return out


def is_zero_bits(t):
    return bool((t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32) == 0).all())


def assert_no_gradient(dl, c0, n, tgt, rows, eps, what):
    """rows of a dlogits chunk that carry no gradient (zero coefficient): all-zero bit patterns — with the one exception the
    unchanged dlogits epilogue makes without label smoothing.  There it forms (softmax - 1) * coef on the row's own target column,
    and a negative number times +0 is -0.0; the unweighted path writes the same -0.0 on its ignored rows at column ignore_index, and
    unit weights must reproduce its bits.  That one element per row must still be a zero; every other element must be +0.0.  (With
    label smoothing the epilogue subtracts its terms from softmax * coef = +0 and every element is +0.0.)"""
    blk = dl[rows, :n].clone()
    if eps == 0:
        t = tgt[rows] - c0
        inside = (t >= 0) & (t < n)
        r = torch.arange(blk.shape[0], device=blk.device)[inside]
        assert (blk[r, t[inside]] == 0).all(), what
        blk[r, t[inside]] = 0
    assert is_zero_bits(blk), what


# ================================================================================================ kernels
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("R,V,d", SHAPES)
def test_weighted_forward_and_dlogits_match_float64(K, R, V, d, eps, norm):
    c = case(R, V, d)
    ref = c["ref"][(eps, norm)]
    assert_sensitive(ref)
    w = ref["w"].float().contiguous()
    tgt = c["tgt"]
    lse, acc, nll = K.lmhead_ce_fwd_weighted(c["h"], c["E"], tgt, V, w, 1, norm, ignore_index=IGN, label_smoothing=eps)
    close(lse, torch.logsumexp(c["logits"], -1), 1e-4, 2e-3, "row lse")
    close(nll, ref["rows"], 1e-4, 2e-3, "row_nll")
    assert is_zero_bits(nll[tgt == IGN]), "ignored rows: an exact 0"
    got = (acc[0] / acc[1]).item()
    print(f"weighted loss {got:.6f} float64 {ref['loss']:.6f} err {abs(got - ref['loss']):.3e} bound {LOSS_RTOL * ref['scale']:.3e}; "
          f"N {acc[1].item():.6f} float64 {ref['N']:.6f}")
    assert abs(got - ref["loss"]) <= LOSS_RTOL * ref["scale"], (got, ref["loss"], ref["scale"])
    if norm == "tokens":
        assert acc[1].item() == ref["N"]
    else:
        assert abs(acc[1].item() - ref["N"]) <= 1e-6 * (ref["w"] * ref["valid"]).abs().sum().item()
    # dlogits chunk by chunk against w_r / N (softmax - (1 - eps) onehot - eps / V).  rtol: the bf16 gate.  atol: the existing rule,
    # a quarter of the smallest term that must show — the uniform term of the smallest non-zero weight, min|w| eps / V / |N|; without
    # smoothing the existing 2e-6 per unit coefficient, scaled by the smallest coefficient min|w| / |N|.
    rowp = K.lmhead_ce_rowp(lse, tgt, acc, ignore_index=IGN, label_smoothing=eps, V=V, weights=w, rows_per_weight=1)
    assert rowp.shape == (R, 4 if eps > 0 else 2)
    coef = ref["w"] * ref["valid"] / ref["N"]
    wmin = ref["w"][ref["w"] != 0].abs().min().item()
    assert wmin >= 0.25
    atol = (0.25 * eps / V if eps > 0 else 2e-6) * wmin / abs(ref["N"])
    dead = (coef == 0)
    for c0, n, n8, dl in dlogits_chunks(K, c, V, rowp, eps):
        onehot = F.one_hot(tgt, V)[:, c0:c0 + n].double()
        want = coef[:, None] * (c["soft"][:, c0:c0 + n] - (1.0 - eps) * onehot - eps / V)
        err = (dl[:, :n].double() - want).abs().max().item()
        print(f"dlogits chunk at {c0}: max abs err {err:.3e} (atol {atol:.3e})")
        close(dl[:, :n], want, 2e-2, atol, f"dlogits chunk at {c0}")
        assert is_zero_bits(dl[:, n:n8]), "pad columns of a ragged chunk are zeros"
        assert_no_gradient(dl, c0, n, tgt, dead, eps, "rows with w == 0 and ignored rows: all-zero bit patterns")
    assert dead.sum().item() > (tgt == IGN).sum().item(), "the case holds zero-weight rows that are not ignored"


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("R,V,d", SHAPES)
def test_unit_weights_are_the_unweighted_path_bit_for_bit(K, R, V, d, eps):
    """3a: weights == 1, norm "tokens".  row_lse, rowp, every dlogits chunk and N equal the unweighted calls; the loss sum and the
    per-row terms equal the deterministic forward's (the same expression and the same order of additions)."""
    c = case(R, V, d)
    h, E, tgt = c["h"], c["E"], c["tgt"]
    ones = torch.ones(R, device="cuda")
    lse_w, acc_w, nll_w = K.lmhead_ce_fwd_weighted(h, E, tgt, V, ones, 1, "tokens", ignore_index=IGN, label_smoothing=eps)
    lse_u, acc_u = K.lmhead_ce_fwd(h, E, tgt, V, ignore_index=IGN, label_smoothing=eps)
    assert torch.equal(lse_w, lse_u) and torch.equal(acc_w[1], acc_u[1])
    tiles = (V + 255) // 256
    part = torch.empty(R, tiles, 2, device="cuda"); tl = torch.empty(R, device="cuda"); lse_o = torch.empty(R, device="cuda")
    part_sum = torch.empty(R, tiles, device="cuda") if eps > 0 else None
    _, acc_o, loss_o = K.lmhead_ce_fwd_ordered(h, E, tgt, V, part, tl, lse_o, IGN, eps, None, part_sum)
    assert torch.equal(lse_w, lse_o) and torch.equal(nll_w, loss_o), "row_nll is vacnic_lmhead_row_loss's row_loss"
    assert torch.equal(acc_w[:2], acc_o[:2]), (acc_w.tolist(), acc_o.tolist())
    rp_w = K.lmhead_ce_rowp(lse_w, tgt, acc_w, ignore_index=IGN, label_smoothing=eps, V=V, weights=ones)
    rp_u = K.lmhead_ce_rowp(lse_u, tgt, acc_u, ignore_index=IGN, label_smoothing=eps, V=V)
    assert torch.equal(rp_w, rp_u)
    g = torch.tensor(0.37, device="cuda")                             # a grad_out and a grad_scale: the same order of operations
    rp_w = K.lmhead_ce_rowp(lse_w, tgt, acc_w, grad_out=g, grad_scale=3.0, ignore_index=IGN, label_smoothing=eps, V=V, weights=ones)
    rp_u = K.lmhead_ce_rowp(lse_u, tgt, acc_u, grad_out=g, grad_scale=3.0, ignore_index=IGN, label_smoothing=eps, V=V)
    assert torch.equal(rp_w, rp_u)
    for (c0, _, _, a), (_, _, _, b) in zip(dlogits_chunks(K, c, V, rp_w, eps), dlogits_chunks(K, c, V, rp_u, eps)):
        assert torch.equal(a, b), f"dlogits chunk at {c0}"


@pytest.mark.parametrize("factor", [2.0, -0.5])
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("R,V,d", SHAPES[1:])
def test_power_of_two_weights_scale_dlogits_exactly(K, R, V, d, eps, factor):
    """3b: a power of two commutes with every rounding on the way (no value here is near the bf16 subnormals)."""
    c = case(R, V, d)
    tgt = c["tgt"]
    const = torch.full((R,), factor, device="cuda")
    lse, acc, _ = K.lmhead_ce_fwd_weighted(c["h"], c["E"], tgt, V, const, 1, "tokens", ignore_index=IGN, label_smoothing=eps)
    lse_u, acc_u = K.lmhead_ce_fwd(c["h"], c["E"], tgt, V, ignore_index=IGN, label_smoothing=eps)
    rp = K.lmhead_ce_rowp(lse, tgt, acc, ignore_index=IGN, label_smoothing=eps, V=V, weights=const)
    rp_u = K.lmhead_ce_rowp(lse_u, tgt, acc_u, ignore_index=IGN, label_smoothing=eps, V=V)
    for (c0, _, _, a), (_, _, _, b) in zip(dlogits_chunks(K, c, V, rp, eps), dlogits_chunks(K, c, V, rp_u, eps)):
        assert torch.equal(a, (b.float() * factor).to(torch.bfloat16)), f"dlogits chunk at {c0}"
        assert b.float().abs().max().item() > 0


@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("norm", NORMS)
def test_per_caption_weights_equal_expanded_weights_and_launches_repeat(K, T, eps, norm):
    """3c: [S] weights with rows_per_weight = T against repeat_interleave(T) per-row weights; 3d: a second launch, the same bits."""
    R, V, d = SHAPES[1]
    c = case(R, V, d)
    tgt = c["tgt"]
    ws = c["w"][:R // T].abs().contiguous() if norm == "weights" else c["w"][:R // T].contiguous()
    runs = []
    for weights, rpw in ((ws, T), (ws.repeat_interleave(T).contiguous(), 1), (ws, T)):
        lse, acc, nll = K.lmhead_ce_fwd_weighted(c["h"], c["E"], tgt, V, weights, rpw, norm, ignore_index=IGN, label_smoothing=eps)
        rp = K.lmhead_ce_rowp(lse, tgt, acc, ignore_index=IGN, label_smoothing=eps, V=V, weights=weights, rows_per_weight=rpw)
        runs.append([lse, acc[:2].clone(), nll.clone(), rp] + [x[3] for x in dlogits_chunks(K, c, V, rp, eps)])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    assert torch.isfinite(runs[0][1]).all() and runs[0][1][0].item() != 0


def test_bad_arguments_are_value_errors_and_launch_nothing(K):
    """4: straight at the C ABI (the Python wrappers refuse most of these before the call)."""
    from vacnic_amd import _lib
    R, V, d = SHAPES[1]
    c = case(R, V, d)
    tgt, w = c["tgt"], c["w"]
    tiles = (V + 255) // 256
    lse, acc, _ = K.lmhead_ce_fwd_weighted(c["h"], c["E"], tgt, V, w, 1, "tokens", ignore_index=IGN)
    tl = torch.zeros(R, device="cuda"); ps = torch.zeros(R, tiles, device="cuda")
    outs = [torch.full((n,), 9.0, device="cuda") for n in (R, R, R, 4, 4 * R)]
    nll, wl, wn, a, rowp = outs
    st = K._stream()

    def wloss(weights=w.data_ptr(), rpw=1, norm_mode=0, eps=0.0, part_sum=ps.data_ptr(), part_tiles=tiles):
        _lib.call("vacnic_lmhead_ce_wloss", lse.data_ptr(), tl.data_ptr(), tgt.data_ptr(), part_sum, weights, rpw, R, V, part_tiles, IGN, eps,
                  norm_mode, nll.data_ptr(), wl.data_ptr(), wn.data_ptr(), a.data_ptr(), st)

    def rowp_w(weights=w.data_ptr(), rpw=1, eps=0.0, norm=acc.data_ptr() + 4):
        _lib.call("vacnic_lmhead_ce_rowp_w", lse.data_ptr(), tgt.data_ptr(), weights, rpw, norm, None, 1.0, eps, V, rowp.data_ptr(), R, IGN, st)

    for fn in (wloss, rowp_w):
        with pytest.raises(ValueError, match="do not split"):
            fn(rpw=7)                                                # 64 % 7 != 0
        with pytest.raises(ValueError, match="do not split"):
            fn(rpw=0)
        with pytest.raises(ValueError, match="label_smoothing"):
            fn(eps=1.0)
        with pytest.raises(ValueError, match="label_smoothing"):
            fn(eps=-0.1)
        with pytest.raises(ValueError, match="null operand"):
            fn(weights=None)
    with pytest.raises(ValueError, match="norm_mode 2"):
        wloss(norm_mode=2)
    with pytest.raises(ValueError, match="norm_mode -1"):
        wloss(norm_mode=-1)
    with pytest.raises(ValueError, match="needs part_sum"):
        wloss(eps=0.3, part_sum=None)
    with pytest.raises(ValueError, match="part_tiles"):
        wloss(part_tiles=tiles + 1)
    with pytest.raises(ValueError, match="null operand"):
        rowp_w(norm=None)
    torch.cuda.synchronize()
    for t in outs:
        assert (t == 9.0).all(), "a rejected call launches nothing"
    wloss(); rowp_w()                                                # the defaults of the helpers are a valid call
    torch.cuda.synchronize()
    assert not (nll == 9.0).any() and not (rowp[:2 * R] == 9.0).any()


@pytest.mark.parametrize("eps", EPS)
def test_zero_weight_sum_under_norm_weights(K, eps):
    """5: sum w = 0 under norm "weights".  All weights zero: 0 / 0, the loss is NaN like torch's mean over nothing.  Weights +1 / -1
    in equal numbers: N is an exact 0 as well, the loss x / 0 is not finite.  Either way every rowp coefficient and all of dlogits
    are exact zeros: no gradient, and no NaN on its way into the gradient arena."""
    R, V, d = SHAPES[1]
    c = case(R, V, d)
    tgt = c["tgt"]
    valid = (tgt != IGN).nonzero().view(-1)
    pm = torch.zeros(R, device="cuda")
    half = valid.numel() // 2
    pm[valid[:half]] = 1.0; pm[valid[half:2 * half]] = -1.0
    for name, w in (("zeros", torch.zeros(R, device="cuda")), ("plus-minus", pm)):
        lse, acc, nll = K.lmhead_ce_fwd_weighted(c["h"], c["E"], tgt, V, w, 1, "weights", ignore_index=IGN, label_smoothing=eps)
        loss = (acc[0] / acc[1]).item()
        out4 = K.combine_losses(acc.data_ptr(), acc.data_ptr() + 4, None, None, 0.0, 0.0, acc.device)
        print(f"{name}: acc {acc[:2].tolist()} loss {loss} combine_losses {out4[1].item()}")
        assert acc[1].item() == 0.0
        assert np.isnan(loss) if name == "zeros" else not np.isfinite(loss)
        assert not np.isfinite(out4[1].item())
        assert torch.isfinite(nll).all() and nll.abs().sum().item() > 0
        rp = K.lmhead_ce_rowp(lse, tgt, acc, ignore_index=IGN, label_smoothing=eps, V=V, weights=w)
        assert torch.equal(rp[:, 0], lse) and is_zero_bits(rp[:, 1:])
        everyone = torch.ones(R, dtype=torch.bool, device="cuda")
        for c0, n, n8, dl in dlogits_chunks(K, c, V, rp, eps):
            assert_no_gradient(dl, c0, n, tgt, everyone, eps, f"dlogits chunk at {c0}")
            assert is_zero_bits(dl[:, n:n8])


# ================================================================================================ autograd
@pytest.mark.parametrize("R,V,d,eps", [(64, 1000, 128, 0.3), (300, 50267, 256, 0.0)])
def test_autograd_function_with_weights(K, R, V, d, eps):
    """6: ops.lm_head_ce(weights=): loss, dh and dE against float64 autograd (gates of test_autograd_function_with_label_smoothing);
    the weights get no gradient."""
    from vacnic_amd import ops
    c = case(R, V, d)
    ref = c["ref"][(eps, "tokens")]
    hf = c["h"].double().requires_grad_(True); Ef = c["E"][:V].double().requires_grad_(True)
    rows = F.cross_entropy(hf @ Ef.t(), c["tgt"], reduction="none", ignore_index=IGN, label_smoothing=eps)
    ((ref["w"] * rows * ref["valid"]).sum() / ref["N"]).backward()
    egrad = torch.zeros(c["Vp"], d, device="cuda")
    hh = c["h"].clone().requires_grad_(True)
    w = c["w"].clone().requires_grad_(True)
    loss, acc, nll = ops.lm_head_ce(hh, None, c["E"], egrad, c["tgt"], V, IGN, label_smoothing=eps, weights=w, rows_per_weight=1)
    assert abs(loss.item() - ref["loss"]) <= LOSS_RTOL * ref["scale"], (loss.item(), ref["loss"])
    assert not acc.requires_grad and not nll.requires_grad
    close(nll, ref["rows"], 1e-4, 2e-3, "row_nll")
    loss.backward()
    assert w.grad is None
    close(hh.grad, hf.grad, 3e-2, 2e-2 * hf.grad.abs().max().item(), "dh")
    close(egrad[:V], Ef.grad, 3e-2, 2e-2 * Ef.grad.abs().max().item(), "dE")
    assert (egrad[V:] == 0).all()


@pytest.mark.parametrize("eps", EPS)
def test_no_weights_is_the_path_of_before(K, eps, monkeypatch):
    """6: weights=None issues the C-ABI calls of the unweighted path and none of the new ones, and in deterministic mode its loss,
    dh and dE are torch.equal to unit weights under norm "tokens" (which is in turn, call for call, the unweighted arithmetic)."""
    from vacnic_amd import _lib, ops
    R, V, d = SHAPES[1]
    c = case(R, V, d)
    names = []
    real = _lib.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(K, "call", call)

    def run(weights):
        del names[:]
        egrad = torch.zeros(c["Vp"], d, device="cuda")
        hh = c["h"].clone().requires_grad_(True)
        out = ops.lm_head_ce(hh, None, c["E"], egrad, c["tgt"], V, IGN, label_smoothing=eps, weights=weights)
        assert len(out) == (2 if weights is None else 3)
        out[0].backward()
        torch.cuda.synchronize()
        return out[0].detach().clone(), out[1][:2].clone(), hh.grad.clone(), egrad, list(names)

    new = {"vacnic_lmhead_ce_wloss", "vacnic_lmhead_ce_rowp_w"}
    with ops.deterministic_mode(True):
        plain, unit = run(None), run(torch.ones(R, device="cuda"))
    assert not new & set(plain[4]) and new <= set(unit[4])
    assert {"vacnic_lmhead_row_loss", "vacnic_sum_ordered"} <= set(plain[4])
    assert ("vacnic_lmhead_ce_rowp_smooth" if eps > 0 else "vacnic_lmhead_ce_rowp") in plain[4]
    for a, b, what in zip(plain[:4], unit[:4], ("loss", "acc", "dh", "dE")):
        assert torch.equal(a, b), what
    default = run(None)                                              # the default mode: the atomic loss sum, no ordered kernels
    assert not (new | {"vacnic_lmhead_row_loss", "vacnic_sum_ordered"}) & set(default[4])


# ================================================================================================ model, step, plan
def small_cfg(**kw):
    from vacnic_amd.config import VacnicConfig
    base = dict(d_model=768, encoder_layers=1, decoder_layers=1, encoder_attention_heads=12, decoder_attention_heads=12,
                encoder_ffn_dim=3072, decoder_ffn_dim=3072, enc_fusion_layer=[0], dim_common=768, clip_width=768, dropout=0.0,
                attention_dropout=0.0, activation_dropout=0.0)
    base.update(kw)
    return VacnicConfig(**base)


def _vcfg():
    from vacnic_amd.config import ClipVisionConfig
    return ClipVisionConfig(width=768, layers=1, patch_size=16, image_size=32, output_dim=64)


def _batch(cfg, B=2, seed=9):
    from vacnic_amd import synthetic
    from vacnic_amd.training import to_device
    return to_device(synthetic.make_batch(cfg, B, S=24, T=8, F=2, seed=seed, image_size=32), "cuda")


def _fresh(cfg, with_guide=False, **opt_kw):
    from vacnic_amd import ops
    from vacnic_amd.training import FusedAdamW, build_models
    ops.Rng.manual_seed(3); ops.Rng.device_counter().zero_()
    model, guide, _ = build_models(cfg, _vcfg(), init="synthetic", seed=0, with_guide=with_guide)
    kw = dict(lr=1e-4, weight_decay=0.01, num_warmup_steps=2, num_training_steps=20)
    kw.update(opt_kw)
    return model, guide, FusedAdamW(model.arena, **kw)


def _reset(model, opt, saved):
    """back to the saved weights with a fresh optimizer: moments, schedule position, gradient, dropout seed and counter as built"""
    from vacnic_amd import ops
    a = model.arena
    a.flat32.copy_(saved); a.refresh_shadow()
    a.exp_avg.zero_(); a.exp_avg_sq.zero_(); a.grad.zero_(); opt.hyper.zero_()
    ops.Rng.manual_seed(3); ops.Rng.device_counter().zero_()
    torch.cuda.synchronize()


def test_model_forward_loss_weights():
    """7: [B] and expanded [B, T] weights give the same bits (loss and the whole gradient arena, deterministic mode); token_nll is
    -score()'s token_logprobs bit for bit in eval mode; the forbidden combinations raise."""
    from vacnic_amd import ops, streams
    from vacnic_amd.training import _model_inputs
    cfg = small_cfg()
    model, _, _ = _fresh(cfg)
    batch = _batch(cfg)
    tgt = batch["caption_ids"]
    B, T = tgt.shape
    w = torch.tensor([1.5, -0.75], device="cuda")
    with torch.no_grad():
        src, src_mask, feats, kw = _model_inputs(model, batch)
    model.train()
    got = []
    with ops.deterministic_mode(True):
        for weights in (w, w[:, None].expand(B, T).contiguous(), None):
            model.arena.grad.zero_()
            ops.Rng.manual_seed(5); ops.Rng.device_counter().zero_()
            ops.begin_step()
            out = model(input_ids=src, attention_mask=src_mask, image_features=feats, labels=tgt, output_logits=False, loss_weights=weights,
                        **kw)
            out["loss"].backward(ops.const_one(out["loss"].device))
            ops.flush_wgrads()
            streams.join_all()
            torch.cuda.synchronize()
            got.append((out["loss"].detach().clone(), out["loss_acc"][:2].clone(), model.arena.grad.clone(), out.get("token_nll")))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][2], got[1][2])
    assert torch.equal(got[0][3], got[1][3]) and got[0][3].shape == (B, T) and not got[0][3].requires_grad
    assert got[2][3] is None and "token_nll" not in out
    assert torch.isfinite(got[0][2]).all() and got[0][2].abs().sum().item() > 0
    assert not torch.equal(got[0][0], got[2][0]) and not torch.equal(got[0][2], got[2][2]), "signed weights change loss and gradient"
    model.eval()
    with torch.no_grad():
        out = model(input_ids=src, attention_mask=src_mask, image_features=feats, labels=tgt, loss_weights=w, **kw)
        lg = model(input_ids=src, attention_mask=src_mask, image_features=feats, labels=tgt, loss_weights=w, output_logits=True, **kw)
        sc = model.score(input_ids=src, attention_mask=src_mask, labels=tgt, image_features=feats, **kw)
        assert torch.equal(out["token_nll"], -sc["token_logprobs"])
        assert (out["token_nll"][tgt == cfg.pad_token_id] == 0).all() and (out["token_nll"][tgt != cfg.pad_token_id] > 0).all()
        # loss_acc = {sum w l, N}; only the fused loss is weighted: the logits come back as always
        nll = out["token_nll"].double()
        want = (w.double()[:, None] * nll).sum().item() / (tgt != cfg.pad_token_id).sum().item()
        assert abs(out["loss"].item() - want) <= 1e-5 * (w.abs().double()[:, None] * nll).sum().item() / out["loss_acc"][1].item()
        assert torch.equal(lg["loss"], out["loss"]) and lg["logits"].shape[:2] == (B, T)
        with pytest.raises(ValueError, match="output_token_stats"):
            model(input_ids=src, attention_mask=src_mask, image_features=feats, labels=tgt, loss_weights=w, output_token_stats=True, **kw)
        with pytest.raises(ValueError, match="pass labels="):
            model(input_ids=src, attention_mask=src_mask, image_features=feats, decoder_input_ids=tgt, loss_weights=w, **kw)
        with pytest.raises(ValueError, match="float64"):
            model(input_ids=src, attention_mask=src_mask, image_features=feats, labels=tgt, loss_weights=w.double(), **kw)
        with pytest.raises(ValueError, match="norm='mean'"):
            model(input_ids=src, attention_mask=src_mask, image_features=feats, labels=tgt, loss_weights=w, loss_norm="mean", **kw)


def test_train_step_batch_key():
    """8: deterministic mode, one step from the same state: batch["loss_weights"] = ones leaves out4 and every weight torch.equal to
    the step without the key; random weights do not."""
    from vacnic_amd.training import TrainArgs, train_step
    cfg = small_cfg()
    args = TrainArgs(num_training_steps=20, warmup_rate=0.1, lr_bart=1e-4, deterministic=True)
    batch = _batch(cfg)
    B = batch["caption_ids"].shape[0]
    runs = []
    model, guide, opt = _fresh(cfg, with_guide=True, lr=args.lr_bart, num_warmup_steps=0)      # (no warm-up: the first update has lr > 0)
    saved = model.arena.flat32.clone()
    for weights in (None, torch.ones(B, device="cuda"), torch.tensor([2.0, -1.0], device="cuda")):
        _reset(model, opt, saved)
        out4 = train_step(model, guide, opt, batch if weights is None else dict(batch, loss_weights=weights), args).clone()
        torch.cuda.synchronize()
        runs.append((out4, model.arena.flat32.clone()))
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[1][0], runs[0][0]), (runs[1][0].tolist(), runs[0][0].tolist())
    assert torch.equal(runs[1][1], runs[0][1]), int((runs[1][1] != runs[0][1]).sum().item())
    assert not torch.equal(runs[2][0][:2], runs[0][0][:2]) and not torch.equal(runs[2][1], runs[0][1])
    assert torch.equal(runs[2][0][2:], runs[0][0][2:]), "SECLA and CoLaM do not see the weights"


def test_planned_step_recorded_with_the_key():
    """9: a plan recorded with batch["loss_weights"] replays with refreshed weights: three replays with three different weight
    tensors against three eager steps from the same state (the gate of the existing planned-vs-eager tests).  A batch without the
    key is refused."""
    from vacnic_amd import streams
    from vacnic_amd.training import PlannedTrainStep, TrainArgs, train_step
    cfg = small_cfg()
    args = TrainArgs(num_training_steps=20, warmup_rate=0.1, lr_bart=1e-4)
    base = _batch(cfg)
    ws = [torch.tensor(v, device="cuda") for v in ([1.0, 1.0], [2.0, -1.0], [-0.5, 0.25], [0.0, 3.0])]
    batches = [dict(base, loss_weights=w) for w in ws]
    streams.enable(True)
    try:
        runs, weights = [], []
        model, guide, opt = _fresh(cfg, with_guide=True, lr=args.lr_bart)
        saved = model.arena.flat32.clone()
        for planned in (False, True):
            _reset(model, opt, saved)
            if planned:
                step = PlannedTrainStep(model, guide, opt, args, batches[0], warmup=2)
                losses = [step(b).tolist() for b in batches[1:]]
                with pytest.raises(ValueError, match="recorded with batch"):
                    step(base)
                step.close()
            else:
                for _ in range(3):
                    train_step(model, guide, opt, batches[0], args)
                losses = [train_step(model, guide, opt, b, args).tolist() for b in batches[1:]]
            torch.cuda.synchronize()
            runs.append(np.array(losses))
            weights.append(model.arena.flat32.clone())
        print(f"eager {runs[0][:, 1].tolist()} planned {runs[1][:, 1].tolist()}")
        assert np.isfinite(runs[1]).all()
        np.testing.assert_allclose(runs[1], runs[0], rtol=2e-3, atol=1e-4)
        assert len({round(v, 4) for v in runs[1][:, 1].tolist()}) == 3, "three weight tensors, three different text losses"
        rel = ((weights[1] - weights[0]).norm() / weights[0].norm()).item()
        assert rel < 1e-4, rel
    finally:
        streams.enable(False)


# ================================================================================================ self-critical step
def parity_reward(samples, refs):
    """mean of the token ids modulo 97, scaled to [0, 1): a reward that depends on the sample alone and differs between any two
    random captions"""
    return [sum(t % 97 for t in s) / (97.0 * len(s)) for s in samples]


def _sample_and_score(model, batch, n, seed, max_length):
    """the captions self_critical_step will draw from this state and seed, as (labels [B n, T], -seq_logprob, tokens) and the same
    for the ground truth, scored teacher-forced with model.score"""
    from vacnic_amd.training import _model_inputs, sequences_to_labels
    cfg = model.config
    model.eval()
    with torch.no_grad():
        src, src_mask, feats, kw = _model_inputs(model, batch)
        seqs = model.generate(input_ids=src, attention_mask=src_mask, image_features=feats, add_ner_ffn=True, do_sample=True,
                              num_return_sequences=n, seed=seed, max_length=max_length, **kw)
        _, labels = sequences_to_labels(seqs, cfg.pad_token_id, cfg.eos_token_id, max_length - 1)
        rep = lambda t: t.repeat_interleave(n, dim=0)                                  # noqa: E731
        sc = model.score(input_ids=rep(src), attention_mask=rep(src_mask), labels=labels, image_features=rep(feats),
                         **{k: rep(v) for k, v in kw.items()})
        gt = model.score(input_ids=src, attention_mask=src_mask, labels=batch["caption_ids"], image_features=feats, **kw)
    model.train()
    return seqs, (-sc["seq_logprob"].double(), sc["seq_tokens"].double()), (-gt["seq_logprob"].double(), gt["seq_tokens"].double())


@pytest.mark.parametrize("ce_weight", [0.0, 0.5])
def test_self_critical_step_loss_and_reproducibility(ce_weight):
    """10a: the returned loss is sum_c A_c (-seq_logprob_c) (+ ce_weight sum_b -seq_logprob_gt_b) over the tokens of all rows,
    recomputed from model.score on the same samples, within LOSS_RTOL of the absolute mass.  10b: deterministic mode, the same
    state and seed twice: torch.equal weights."""
    from vacnic_amd.training import TrainArgs, group_advantages, self_critical_step
    cfg = small_cfg()
    args = TrainArgs(num_training_steps=20, lr_bart=1e-4, deterministic=True)
    batch = _batch(cfg)
    n, seed, ML = 2, 11, 9
    finals, outs = [], []
    model, _, opt = _fresh(cfg, lr=args.lr_bart, num_warmup_steps=0)
    saved = model.arena.flat32.clone()
    for run in range(2):
        _reset(model, opt, saved)
        seqs, (nll, tok), (gnll, gtok) = _sample_and_score(model, batch, n, seed, ML)
        if run == 0:
            adv = group_advantages(parity_reward(seqs.tolist(), None), n).double().cuda()
            terms = torch.cat([adv * nll, ce_weight * gnll]) if ce_weight > 0 else adv * nll
            tokens = (tok.sum() + (gtok.sum() if ce_weight > 0 else 0)).item()
            want, mass = terms.sum().item() / tokens, terms.abs().sum().item() / tokens
            plain = (nll.sum() / tok.sum()).item()
            print(f"advantages {adv.tolist()} want {want:.6f} mass {mass:.6f} plain NLL {plain:.6f}")
            assert adv.abs().min().item() > 0 and abs(want - plain) >= 10 * LOSS_RTOL * mass, "the weighted loss is not the plain one"
        out = self_critical_step(model, opt, batch, args, reward_fn=parity_reward, n_samples=n, ce_weight=ce_weight, seed=seed,
                                 max_length=ML).clone()
        torch.cuda.synchronize()
        outs.append(out); finals.append(model.arena.flat32.clone())
    loss, reward, adv2, logp = outs[0].tolist()
    print(f"step: loss {loss:.6f} (want {want:.6f}, bound {LOSS_RTOL * mass:.3e}) reward {reward:.4f} adv^2 {adv2:.5f} logp {logp:.4f}")
    assert abs(loss - want) <= LOSS_RTOL * mass, (loss, want, mass)
    assert abs(reward - float(np.mean(parity_reward(seqs.tolist(), None)))) <= 1e-6 and abs(adv2 - (adv ** 2).mean().item()) <= 1e-6
    assert abs(logp + plain) <= LOSS_RTOL * plain, "mean log-prob of the sampled tokens"
    assert torch.equal(outs[1], outs[0]) and torch.equal(finals[1], finals[0]), int((finals[1] != finals[0]).sum().item())
    assert model.training


def test_self_critical_step_moves_probability_to_the_rewarded_sample():
    """10c: one image, two samples, a reward that prefers sample 0 (advantages +0.5, -0.5), first optimizer step, weight decay 0,
    dropout 0: seq_logprob(sample 0) - seq_logprob(sample 1), scored with model.score, is larger after the step.  The first AdamW
    update is lr * sign(gradient) per element, so its inner product with the gradient is positive and the loss
    0.5 (NLL_0 - NLL_1) / tokens falls to first order.  lr = 1e-3: the synthetic weights have std 0.02 (a bf16 ulp of 2^-13 =
    1.2e-4 there, 4.9e-4 at |w| = 0.1), so the update survives the bf16 copy of nearly every element.
    Measured on an MI355X: the difference goes from -2.1653 to +95.7855 (a step of 1e-3 on every one of the model's elements at
    once is a large move; what is asserted is its direction).
    10d: a DistributedDataParallel wrapper is refused."""
    from vacnic_amd.ddp import DistributedDataParallel
    from vacnic_amd.training import TrainArgs, self_critical_step
    cfg = small_cfg()
    args = TrainArgs(num_training_steps=20, lr_bart=1e-3, weight_decay=0.0)
    batch = _batch(cfg, B=1)
    n, seed, ML = 2, 5, 9
    model, _, opt = _fresh(cfg, lr=args.lr_bart, weight_decay=0.0, num_warmup_steps=0)
    seqs, (nll0, _), _ = _sample_and_score(model, batch, n, seed, ML)
    assert not torch.equal(seqs[0], seqs[1]), "two different samples"
    before = (nll0[1] - nll0[0]).item()                              # = logprob(sample 0) - logprob(sample 1)
    out = self_critical_step(model, opt, batch, args, reward_fn=lambda s, r: [1.0, 0.0], n_samples=n, seed=seed, max_length=ML)
    # the ORIGINAL pair under the new weights
    from vacnic_amd.training import _model_inputs, sequences_to_labels
    with torch.no_grad():
        src, src_mask, feats, kw = _model_inputs(model, batch)
        _, labels = sequences_to_labels(seqs, cfg.pad_token_id, cfg.eos_token_id, ML - 1)
        rep = lambda t: t.repeat_interleave(n, dim=0)                                  # noqa: E731
        sc = model.score(input_ids=rep(src), attention_mask=rep(src_mask), labels=labels, image_features=rep(feats),
                         **{k: rep(v) for k, v in kw.items()})
    after = (sc["seq_logprob"][0] - sc["seq_logprob"][1]).item()
    print(f"logprob(sample 0) - logprob(sample 1): before {before:.4f} after {after:.4f} change {after - before:+.4f}; step {out.tolist()}")
    assert after > before, (before, after)
    assert abs(out[1].item() - 0.5) <= 1e-6 and abs(out[2].item() - 0.25) <= 1e-6
    wrapped = DistributedDataParallel.__new__(DistributedDataParallel)
    with pytest.raises(ValueError, match="one process"):
        self_critical_step(wrapped, opt, batch, args, n_samples=n)
