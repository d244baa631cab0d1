"""Loss kernels (csrc/loss.hip, the fused LM-head cross entropy of csrc/gemm.hip / gemm_kernel.h): every path edge against
float64 on the CPU.  References are torch float64 graphs or small numpy models written from the comments of the kernels (the
SECLA routing model "lowest index wins"); none is built from a kernel's output.  The unmarked tests check the host models, the
seed gaps and, for every value check, that a deliberately wrong reference (a "mutant") lies at least 10x the check's margin away.

Margins (none is taken from a kernel's output):
  * exact outputs (counts, SECLA `sim` on integer data, zero padding, untouched sentinels, masked positions): torch.equal.
  * fp32 outputs (lse, losses, cos, pooled vectors, l1 / l2, part_sum): the same graph is evaluated in fp32 on the CPU from
    the same inputs; the kernel may deviate from float64 by 8x the largest fp32 deviation at that shape (a different but
    legitimate summation order), floored at 1e-6 * max|ref|.
  * bf16 outputs (dlogits, dhs, dfaces): one rounding of an fp32 result: 2^-8 |ref| + atol, atol obtained as above.
  * both cross-entropy paths use __expf / __logf and get an allowance on top.  The compiler's header
    (lib/llvm/lib/clang/*/include/__clang_hip_math.h of the ROCm installation) defines __expf(x) = exp2_native(fl(log2e_f32 * x))
    and __logf(x) = __builtin_logf(x); the installation's documents give no ulp figure for either, so the model is derived:
      - the product fl(c x), c = fl(log2 e), carries two roundings: |dt| <= 2^-23 |x| log2(e), so exp2(t + dt) is off by the
        relative amount ln2 |dt| <= 2^-23 |x|; the native exp2 is taken as 1 ulp = 2^-23 relative.  __expf(x) is within
        2^-23 (1 + |x|) relative of exp(x), and __expf(0) = 1 exactly.
      - every term exp(z_j - gm) of a row is formed as a product of n_fac such factors (the first exponential, one rescale per
        later trip of the thread's walk, one per combine level) whose arguments telescope to z_j - gm, |z_j - gm| <= S, the span
        of the row's finite logits.  The sum is therefore within 2^-23 (S + n_fac) relative, and so is lse absolutely.
        n_fac = ceil(V / 256) + 2 for the materialised kernels (at most V / 256 trips per thread, the block combine), 72 for the
        fused path (64 columns per thread in the epilogue, 3 shuffle levels, the tile combine and its wave reduction).
      - log: 2^-22 |lse - max| (the precise logf is better than that; a native log2 times fl(ln 2) would meet it).
      A_lse = 2^-23 (S + n_fac) + 2^-22 max|lse - max|.  The mean loss gets A_lse, loss_sum gets count * A_lse, and
      dlogits_j = (exp(z_j - lse) - ...) g gets |g| softmax_j (2^-23 (1 + S + ln V) + A_lse), element by element: the
      exponential's error is relative, so it scales with the float64 softmax of that element.
    SECLA uses expf / logf and gets no allowance.
  * no margin is looser than the check of the same quantity in test_kernels_gpu.py / test_label_smoothing_gpu.py: fused
    row_lse is also held to rtol 1e-4 + atol 2e-3 and every mean loss to 2e-3 relative (the bound is the smaller of the two).
  * decisions that hinge on a comparison: SECLA data are integers times a power of two (every `sim` is exact in fp32, so the
    arg-max routing is the same in every precision); the CoLaM hinge side is asserted in float64 to be at least 1000x the fp32
    margin of cos away from the margin.
Every check prints `LOSSCHK <what> <shape> bound=<margin> err=<observed>`: bound and err are those of the element that uses the
largest share of its bound (for a bf16 output the bound includes 2^-8 |ref| of that element), `margin` is the absolute part,
`maxerr` the largest error anywhere.  profiles/loss_misc_tests.txt holds one run of them.

Measured on the MI355X in that run (largest share of its bound that any element uses): CE row_lse 0.05 (margins up to 1.4e-5),
CE loss 0.09, fused row_lse 0.07 (2.6e-5), fused loss 0.22, part_sum totals 0.17, CoLaM cos 0.12, pooled 0.01, loss 0.57 (the
1e-6 |ref| floor), SECLA l1 / l2 0.04, loss 0.11, combine_losses 0.07, dh 0.62, dE 0.75; the bf16 outputs reach 0.98 - 0.99:
2^-8 |ref| is exactly half a bf16 ulp at the bottom of a binade, so a correct rounding comes that close.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
NEG_INF = float("-inf")


# -------------------------------------------------------------------------------------------- plumbing
@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


def cpu_randn(*shape, seed, scale=1.0, dtype=BF16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def cpu_randint(lo, hi, shape, seed):
    return torch.randint(lo, hi, shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def host(t):
    return None if t is None else t.detach().to("cpu")


def t64(v):
    return torch.as_tensor(v, dtype=F64)


def f32_margin(ref64, ref32):
    """8x the deviation of the fp32 evaluation from float64 at this shape, floored at 1e-6 * max|ref|."""
    ref64, ref32 = t64(ref64), t64(ref32)
    dev = (ref32 - ref64).abs().max().item()
    return max(8.0 * dev, 1e-6 * ref64.abs().max().item())


def bound_of(ref64, ref32, bf16=False, extra=0.0, cap=None):
    """(scalar margin, per-element bound).  cap = (rtol, atol) of an existing check of the same quantity: never looser than it."""
    ref64 = t64(ref64)
    extra = t64(extra)                                          # a scalar, or one allowance per element
    base = f32_margin(ref64, ref32)
    margin = base + extra.max().item()
    bound = torch.full_like(ref64, base) + extra + (ref64.abs() * 2.0 ** -8 if bf16 else 0.0)
    if cap is not None:
        bound = torch.minimum(bound, cap[0] * ref64.abs() + cap[1])
    return margin, bound


def check(what, got, ref64, ref32, bf16=False, extra=0.0, cap=None):
    ref64 = t64(ref64)
    got = host(got).to(F64).reshape(ref64.shape)
    margin, bound = bound_of(ref64, ref32, bf16, extra, cap)
    err = (got - ref64).abs()
    used = torch.where(err > 0, err / bound, torch.zeros_like(err)).reshape(-1)          # share of its bound that an element uses
    k = int(torch.nan_to_num(used, nan=float("inf")).argmax())                           # bound / err: those of the worst element
    print(f"LOSSCHK {what} {tuple(ref64.shape)} bound={bound.reshape(-1)[k].item():.3e} err={err.reshape(-1)[k].item():.3e} "
          f"margin={margin:.3e} maxerr={err.max().item():.3e} refmax={ref64.abs().max().item():.3e} used={used[k].item():.3f}")
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    bad = (err > bound).sum().item()
    assert bad == 0, f"{what}: {bad}/{err.numel()} off, max err {err.max().item():.4g}, margin {margin:.4g}"


def check_equal(what, got, want):
    got, want = host(got), host(want)
    diff = (got.to(F64) - want.to(F64)).abs().max().item() if got.numel() else 0.0
    print(f"LOSSCHK {what} {tuple(want.shape)} bound=0.000e+00 err={diff:.3e}")
    assert got.shape == want.shape and torch.equal(got, want), f"{what}: not equal (max diff {diff})"


def assert_sensitive(what, ref64, ref32, mutant64, bf16=False, extra=0.0, cap=None):
    """the wrong reference is at least 10x the check's bound away in some element: a kernel that computed it would fail."""
    ref64, mutant64 = t64(ref64), t64(mutant64).reshape(t64(ref64).shape)
    _, bound = bound_of(ref64, ref32, bf16, extra, cap)
    ratio = ((mutant64 - ref64).abs() / bound).max().item()
    assert ratio >= 10.0, f"{what}: the mutant is only {ratio:.2f}x the margin away"


# ------------------------------------------------------------------------------- cross entropy: reference
def ce_formula(z, tgt, ignore, eps, g=1.0):
    """row_loss = (1 - eps) (lse - z_t) + eps (lse - mean_j z_j) over rows whose target is in [0, V) and != ignore (loss.hip);
    dz = d (g * loss_sum / count) / dz by autograd.  z: [R, V] of the dtype to evaluate in."""
    R, V = z.shape
    z = z.detach().clone().requires_grad_(True)
    lse = torch.logsumexp(z, -1)
    valid = (tgt != ignore) & (tgt >= 0) & (tgt < V)
    zt = z.gather(1, tgt.clamp(0, V - 1)[:, None])[:, 0]
    zt = torch.where(valid, zt, torch.zeros_like(zt))                 # (an ignored row may aim at a -inf logit)
    row = lse - zt
    if eps:
        row = (1.0 - eps) * row + eps * (lse - z.mean(-1))
    row = torch.where(valid, row, torch.zeros_like(row))
    count = int(valid.sum())
    loss_sum = row.sum()
    if count:
        (loss_sum / count * g).backward()
        dz = z.grad
    else:
        dz = torch.zeros_like(z)
    return dict(lse=lse.detach(), row=row.detach(), loss_sum=loss_sum.detach(), count=count,
                loss=(loss_sum / count).detach() if count else None, dz=dz, zsum=z.detach().sum(-1))


def span_of(z64):
    """largest span of a row's finite logits, and the largest lse - max."""
    fin = torch.isfinite(z64)
    hi = torch.where(fin, z64, torch.full_like(z64, NEG_INF)).max(-1).values
    lo = torch.where(fin, z64, torch.full_like(z64, float("inf"))).min(-1).values
    return (hi - lo).max().item(), (torch.logsumexp(z64, -1) - hi).abs().max().item()


def ce_allowances(z64, V, n_fac, g, count):
    S, lmax = span_of(z64)
    a_lse = 2.0 ** -23 * (S + n_fac) + 2.0 ** -22 * lmax
    a_dz = abs(g) / max(count, 1) * (2.0 ** -23 * (1.0 + S + math.log(V)) + a_lse) * torch.softmax(z64, -1)
    return a_lse, a_dz


def round_up(v, m):
    return (v + m - 1) // m * m


PAD_FILL = 8192.0                      # large, finite, exact in bf16: a pad column that leaks into a row dominates its lse
_CE = {}


def ce_case(V, R, f32, eps, ignore=1, layout="pad", kind="plain", g=1.0):
    """inputs on the CPU + float64 / fp32 references.  layout: 'pad' (ldl > V, aligned rows), 'odd' (fp32, odd ldl: alternate
    rows miss 16-byte alignment), 'view' (fp32, a [:, 1:] view: misaligned base).  kind: 'plain', 'ignored' (every row ignored),
    'range' (targets outside [0, V): ignored by the materialised kernels), 'ninf' (-inf logits)."""
    key = (V, R, f32, eps, ignore, layout, kind, g)
    if key in _CE:
        return _CE[key]
    dt = F32 if f32 else BF16
    off = 1 if layout == "view" else 0
    if not f32:
        ldl = round_up(V, 8) + 8
    elif layout == "odd":
        ldl = (V + 6) | 1
    else:
        ldl = round_up(V, 4) + 8
    buf = torch.full((R, ldl), PAD_FILL, dtype=dt)
    z = cpu_randn(R, V, seed=1000 * V + R + (7 if f32 else 0), scale=2.0, dtype=dt)
    ig = ignore if ignore != "last" else V - 1
    base = [0, V - 1, 7 % V, 8 % V, ig]
    tgt = torch.tensor([base[i % 5] for i in range(R)]) if R > 1 else torch.tensor([V - 1])
    if kind == "ignored":
        tgt = torch.full((R,), ig)
    elif kind == "range":
        tgt = torch.tensor([V + 3, -5, V, 0, V - 1][:R])
    elif kind == "ninf":
        # an aligned group of 8 (both vectors of thread 0's first fp32 trip) all -inf before anything finite in thread 0's
        # walk (thread 0 meets finite values afterwards: its second trip at V = 2056, the scalar tail at V = 2047; on a misaligned
        # fp32 row column 256), the second column of the scalar tail, scattered ones; row 4 is ignored and aims at a -inf logit
        cols = [c for c in list(range(0, 8)) + list(range(1024, 1032)) + [V - (V - 1) % 8, 300, 1500] if c < V - 1]
        z[:, cols] = NEG_INF
        z[1, :] = NEG_INF; z[1, V - 1] = 0.5                        # a row with a single finite logit, at the very end
        tgt = torch.tensor([V - 1, V - 1, min(9, V - 1), V - 1, 1][:R])
        assert ig == 1 and torch.isinf(z[4, 1]) and torch.isfinite(z[torch.arange(4), tgt[:4]]).all()
    buf[:, off:off + V] = z
    z64 = z.to(F64)
    r64, r32 = ce_formula(z64, tgt, ig, eps, g), ce_formula(z.to(F32), tgt, ig, eps, g)
    a_lse, a_dz = ce_allowances(z64, V, math.ceil(V / 256) + 2, g, r64["count"])
    c = dict(V=V, R=R, f32=f32, eps=eps, ignore=ig, ldl=ldl, off=off, buf=buf, z=z, tgt=tgt, r64=r64, r32=r32, a_lse=a_lse, a_dz=a_dz, g=g)
    _CE[key] = c
    return c


LOSS_CAP = (2e-3, 0.0)                 # the gate of the existing cross-entropy tests
FUSED_LSE_CAP = (1e-4, 2e-3)           # test_lmhead_ce_fused_matches_materialised_logits


def ce_run(K, c, grad_out=None, grad_scale=1.0, ldd_extra=8):
    """forward + backward of the materialised pair on the case; dlogits rows are wider than the logits rows (ldd > ldl)."""
    buf = c["buf"].cuda()
    logits = buf[:, c["off"]:] if c["off"] else buf
    tgt = c["tgt"].cuda()
    lse, acc = K.ce_fwd(logits, tgt, c["V"], ignore_index=c["ignore"], label_smoothing=c["eps"])
    ldd = round_up(c["ldl"] + ldd_extra, 8)
    dl = torch.full((c["R"], ldd), 7.0, device="cuda", dtype=BF16)
    go = None if grad_out is None else torch.tensor(grad_out, device="cuda", dtype=F32)
    K.ce_bwd(logits, tgt, c["V"], lse, acc, dl, grad_out=go, grad_scale=grad_scale, ignore_index=c["ignore"], label_smoothing=c["eps"])
    torch.cuda.synchronize()
    return lse, acc, dl


def ce_compare(what, c, lse, acc, dl, lse_cap=None):
    r64, r32, V = c["r64"], c["r32"], c["V"]
    check(f"{what} row_lse", lse, r64["lse"], r32["lse"], extra=c["a_lse"], cap=lse_cap)
    acc = host(acc)
    assert acc[1].item() == r64["count"], f"{what}: count {acc[1].item()} != {r64['count']}"
    print(f"LOSSCHK {what} count () bound=0.000e+00 err={abs(acc[1].item() - r64['count']):.3e}")
    if r64["count"]:
        check(f"{what} loss", acc[0] / acc[1], r64["loss"], r32["loss"], extra=c["a_lse"], cap=LOSS_CAP)
    else:
        assert acc[0].item() == 0.0
    if dl is not None:
        check(f"{what} dlogits", dl[:, :V], r64["dz"], r32["dz"], bf16=True, extra=c["a_dz"])
        assert (host(dl)[:, V:] == 0).all(), f"{what}: dlogits padding is not zero"


CE_SIZES = [1, 7, 8, 9, 255, 256, 257, 2047, 2056]


# ---------------------------------------------------------------------- cross entropy: unmarked host checks
def test_ce_formula_is_torch_cross_entropy():
    """the formula written from the kernel's comment against torch's own cross_entropy, for targets inside its domain."""
    for V, eps, ig in [(9, 0.0, 1), (257, 0.1, -100), (257, 0.1, 0), (300, 0.3, 299)]:
        z = cpu_randn(6, V, seed=V, scale=2.0, dtype=F64)
        tgt = torch.tensor([0, V - 1, 7, 8, ig, 5])
        r = ce_formula(z, tgt, ig, eps, g=1.7)
        zz = z.clone().requires_grad_(True)
        ref = F.cross_entropy(zz, tgt, ignore_index=ig, label_smoothing=eps)
        (ref * 1.7).backward()
        assert abs(r["loss"].item() - ref.item()) < 1e-12 and (r["dz"] - zz.grad).abs().max().item() < 1e-13
        assert r["count"] == int((tgt != ig).sum())


def test_ce_ninf_reference_is_finite():
    for f32 in (False, True):
        for V in (7, 2047, 2056):
            c = ce_case(V, 5, f32, 0.0, kind="ninf")
            r = c["r64"]
            assert torch.isfinite(r["lse"]).all() and torch.isfinite(r["loss"]) and torch.isfinite(r["dz"]).all()
            assert r["count"] == 4 and (r["dz"][4] == 0).all()
            assert abs(r["lse"][1].item() - 0.5) < 1e-12                     # the row with one finite logit
            zz = c["z"].to(F64).requires_grad_(True)                          # torch agrees on -inf logits
            ref = F.cross_entropy(zz, c["tgt"], ignore_index=1)
            ref.backward()
            assert abs(ref.item() - r["loss"].item()) < 1e-12 and (zz.grad - r["dz"]).abs().max().item() < 1e-13


def _ce_mutants(z64, tgt, ig, eps, g, V, pad=None):
    """wrong references: last column dropped, pad columns included, target off by one, the ignored rows counted, eps / V omitted."""
    R = z64.shape[0]
    m = {}
    if V > 1:
        d = ce_formula(z64[:, :V - 1], tgt.clamp(max=V - 2), ig, eps, g)
        m["last column dropped"] = dict(lse=d["lse"], loss=d["loss"], dz=F.pad(d["dz"], (0, 1)))
        t1 = torch.where((tgt != ig), (tgt + 1) % V, tgt)
        m["target off by one"] = {k: ce_formula(z64, t1, ig, eps, g)[k] for k in ("loss", "dz")}
    if pad is not None:
        d = ce_formula(torch.cat([z64, pad], 1), tgt, ig, eps, g)
        m["pad columns included"] = dict(lse=d["lse"], loss=d["loss"], dz=d["dz"][:, :V])
    if (tgt == ig).any() and 0 <= ig < V:
        d = ce_formula(z64, tgt, V + 99, eps, g)
        m["ignore_index row counted"] = dict(loss=d["loss"], dz=d["dz"])
    if eps:
        valid = ((tgt != ig) & (tgt >= 0) & (tgt < V)).to(F64)[:, None]
        cnt = max(int(valid.sum()), 1)
        m["eps/V term omitted"] = dict(dz=ce_formula(z64, tgt, ig, eps, g)["dz"] + eps / V * valid * g / cnt)
    return m


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("V", [8, 257, 2056])
def test_ce_mutants_are_caught(V, f32):
    for eps in (0.0, 0.1):
        c = ce_case(V, 5, f32, eps)
        r64, r32 = c["r64"], c["r32"]
        muts = _ce_mutants(c["z"].to(F64), c["tgt"], c["ignore"], eps, 1.0, V, pad=torch.full((5, 3), PAD_FILL, dtype=F64))
        assert set(muts) >= {"last column dropped", "pad columns included", "target off by one", "ignore_index row counted"}
        for name, m in muts.items():
            if "lse" in m:
                assert_sensitive(name, r64["lse"], r32["lse"], m["lse"], extra=c["a_lse"])
            if "loss" in m:
                assert_sensitive(name, r64["loss"], r32["loss"], m["loss"], extra=c["a_lse"], cap=LOSS_CAP)
            assert_sensitive(name, r64["dz"], r32["dz"], m["dz"], bf16=True, extra=c["a_dz"])


def test_ce_margins_are_no_looser_than_the_existing_checks():
    """materialised: loss 2e-3 relative, dlogits rtol 2e-2 + atol 1e-5 at g / count = 1 / count (test_cross_entropy)."""
    for f32 in (False, True):
        for V in CE_SIZES:
            for eps in (0.0, 0.1):
                c = ce_case(V, 5, f32, eps)
                r64, r32 = c["r64"], c["r32"]
                _, b = bound_of(r64["dz"], r32["dz"], bf16=True, extra=c["a_dz"])
                assert (b <= 2e-2 * r64["dz"].abs() + 1e-5).all()
                assert c["a_lse"] < 2e-4 and f32_margin(r64["lse"], r32["lse"]) < 1e-4


# -------------------------------------------------------------------------- cross entropy: GPU, materialised
@gpu
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("V", CE_SIZES)
def test_ce_sizes(K, V, f32, eps):
    """V = 1 (lse = z, zero gradient), the 8-wide chunk edges, one chunk per thread (2047: 255 chunks and a scalar tail of 7),
    a second trip for thread 0 (2056); pad columns at 8192 must stay out; dlogits rows wider than the logits rows."""
    c = ce_case(V, 5, f32, eps)
    ce_compare(f"ce V={V} R=5 f32={f32} eps={eps}", c, *ce_run(K, c))
    c1 = ce_case(V, 1, f32, eps)
    ce_compare(f"ce V={V} R=1 f32={f32} eps={eps}", c1, *ce_run(K, c1))


@gpu
@pytest.mark.parametrize("f32", [False, True])
def test_ce_grad_scaling(K, f32):
    """grad_out as a device scalar and grad_scale != 1: g = 0.75 * 2.5."""
    c = ce_case(257, 5, f32, 0.1, g=0.75 * 2.5)
    ce_compare(f"ce V=257 f32={f32} grad_out=0.75 grad_scale=2.5", c, *ce_run(K, c, grad_out=0.75, grad_scale=2.5))


@gpu
@pytest.mark.parametrize("layout", ["odd", "view"])
@pytest.mark.parametrize("V", [255, 256, 257])
def test_ce_fp32_misaligned_rows(K, V, layout):
    """fp32 rows that miss 16-byte alignment take the scalar walk: every second row with an odd ldl, every row of a [:, 1:] view."""
    for eps in (0.0, 0.1):
        c = ce_case(V, 5, True, eps, layout=layout)
        if layout == "odd":
            assert c["ldl"] % 2 == 1 and (c["ldl"] == 263 or V != 257)
        ce_compare(f"ce V={V} fp32 {layout} ldl={c['ldl']} eps={eps}", c, *ce_run(K, c))


@gpu
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("ignore", [1, -100, 0, "last"])
def test_ce_ignore_index(K, ignore, f32):
    c = ce_case(257, 5, f32, 0.1, ignore=ignore)
    assert c["r64"]["count"] == (4 if ignore in (1, -100) else 3)
    ce_compare(f"ce V=257 f32={f32} ignore={ignore}", c, *ce_run(K, c))
    c0 = ce_case(257, 5, f32, 0.1, ignore=ignore, kind="ignored")
    lse, acc, dl = ce_run(K, c0)
    ce_compare(f"ce V=257 f32={f32} ignore={ignore} all rows ignored", c0, lse, acc, None)
    assert host(acc).tolist() == [0.0, 0.0] and (host(dl) == 0).all(), "every row ignored: count 0 and no gradient"


@gpu
@pytest.mark.parametrize("f32", [False, True])
def test_ce_out_of_range_targets_are_ignored(K, f32):
    """the materialised kernels' rule: a target outside [0, V) is an ignored row (the fused path leaves it undefined)."""
    c = ce_case(257, 5, f32, 0.0, ignore=-100, kind="range")
    assert c["r64"]["count"] == 2
    lse, acc, dl = ce_run(K, c)
    ce_compare(f"ce V=257 f32={f32} out-of-range targets", c, lse, acc, dl)
    assert (host(dl)[:3] == 0).all()


@gpu
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("V", [7, 2047, 2056])
def test_ce_neg_inf_logits(K, V, f32):
    """rows with some -inf logits: torch's finite lse, loss and gradient.  Before the guard in ce_fwd_body a thread that met -inf
    while its running max was still -inf computed exp(-inf - -inf) = NaN, which reached row_lse."""
    c = ce_case(V, 5, f32, 0.0, kind="ninf")
    lse, acc, dl = ce_run(K, c)
    ce_compare(f"ce V={V} f32={f32} -inf logits", c, lse, acc, dl)
    assert (host(dl)[4] == 0).all(), "the ignored row aims at a -inf logit and carries no gradient"
    if f32 and V > 7:                                            # the scalar walk of misaligned rows: column 0 is -inf, column 256 finite
        c = ce_case(V, 5, True, 0.0, layout="odd", kind="ninf")
        ce_compare(f"ce V={V} fp32 odd ldl -inf logits", c, *ce_run(K, c))


@gpu
def test_ce_bf16_refuses_bad_rows(K):
    buf = torch.zeros(5, 272, device="cuda", dtype=BF16)
    tgt = torch.zeros(5, dtype=torch.int64, device="cuda")
    K.ce_fwd(buf[:, :260], tgt, 257)                              # fine: ldl = 272, aligned base
    with pytest.raises(ValueError, match="16-byte aligned"):
        K.ce_fwd(buf.view(-1)[:5 * 268].view(5, 268), tgt, 257)   # ldl = 268: not a multiple of 8
    with pytest.raises(ValueError, match="16-byte aligned"):
        K.ce_fwd(buf[:, 1:], tgt, 257)                            # base 2 bytes off
    with pytest.raises(ValueError, match="bad V/ldl"):
        K.ce_fwd(buf[:, :200], tgt, 300)                          # (ldl = 272 < V)


# ------------------------------------------------------------------------------ fused LM-head cross entropy
FUSED_NFAC = 72
FUSED_V, FUSED_R = [255, 256, 257, 264, 513], [1, 255, 257]
_FUSED = {}


def fused_case(V, R, d, eps, with_bias, ignore, g=1.0):
    """h [R, d], E [round_up(V, 32), d] with zero pad rows (the convention of the existing fused tests); targets on both sides
    of every 256-column tile edge, at 0 and V - 1, some equal to ignore; all others inside [0, V): the fused path's domain."""
    key = (V, R, d, eps, with_bias, ignore, g)
    if key in _FUSED:
        return _FUSED[key]
    Vp = round_up(V, 32)
    h = cpu_randn(R, d, seed=V * 7 + R)
    E = torch.zeros(Vp, d, dtype=BF16)
    E[:V] = cpu_randn(V, d, seed=V * 11 + R + 1, scale=0.3)
    bias = (cpu_randn(V, seed=5, scale=0.5, dtype=F32) + 0.7) if with_bias else None
    tgt = cpu_randint(0, V, (R,), seed=V + R)
    special = [t for t in (0, V - 1, 255, 256, 511, 512) if t < V]
    if R == 1:
        tgt[0] = V - 1
    else:
        for i, t in enumerate(special):
            tgt[3 * i + 2] = t
        tgt[7::11] = ignore
    assert ((tgt == ignore) | ((tgt >= 0) & (tgt < V))).all()

    def logits(dt):
        z = h.to(dt) @ E[:V].to(dt).t()
        return z if bias is None else z + bias.to(dt)
    z64, z32 = logits(F64), logits(F32)
    r64, r32 = ce_formula(z64, tgt, ignore, eps, g), ce_formula(z32, tgt, ignore, eps, g)
    a_lse, a_dz = ce_allowances(z64, V, FUSED_NFAC, g, r64["count"])
    c = dict(V=V, R=R, d=d, eps=eps, ignore=ignore, Vp=Vp, h=h, E=E, bias=bias, tgt=tgt, z64=z64, r64=r64, r32=r32, a_lse=a_lse,
             a_dz=a_dz, g=g)
    _FUSED[key] = c
    return c


def fused_fwd(K, c):
    V, R = c["V"], c["R"]
    dev = {k: (None if c[k] is None else c[k].cuda()) for k in ("h", "E", "bias", "tgt")}
    ps = torch.full((R, (V + 255) // 256), float("nan"), device="cuda") if c["eps"] else None
    lse, acc = K.lmhead_ce_fwd(dev["h"], dev["E"], dev["tgt"], V, ignore_index=c["ignore"], label_smoothing=c["eps"], bias=dev["bias"],
                               part_sum=ps)
    return dev, lse, acc, ps


def fused_dlogits(K, c, dev, lse, acc, col0, ncols, grad_out=None, grad_scale=1.0, sentinel=7.0):
    V, R = c["V"], c["R"]
    go = None if grad_out is None else torch.tensor(grad_out, device="cuda", dtype=F32)
    rowp = K.lmhead_ce_rowp(lse, dev["tgt"], acc, grad_out=go, grad_scale=grad_scale, ignore_index=c["ignore"],
                            label_smoothing=c["eps"], V=V)
    assert rowp.shape == (R, 4 if c["eps"] else 2)
    n8 = round_up(ncols, 8)
    dl = torch.full((R, n8 + 16), sentinel, device="cuda", dtype=BF16)
    K.lmhead_ce_dlogits(dev["h"], dev["E"], dev["tgt"], V, rowp, dl, col0, ncols, ignore_index=c["ignore"], label_smoothing=c["eps"],
                        bias=dev["bias"])
    torch.cuda.synchronize()
    return dl


def fused_compare_dl(what, c, dl, col0, ncols, sentinel=7.0):
    r64, r32 = c["r64"], c["r32"]
    n8 = round_up(ncols, 8)
    sl = slice(col0, col0 + ncols)
    check(f"{what} dlogits[{col0}:{col0 + ncols}]", dl[:, :ncols], r64["dz"][:, sl], r32["dz"][:, sl], bf16=True, extra=c["a_dz"][:, sl])
    dl = host(dl)
    assert (dl[:, ncols:n8] == 0).all(), f"{what}: pad columns up to round_up(ncols, 8) must be zero"
    assert (dl[:, n8:] == sentinel).all(), f"{what}: columns beyond round_up(ncols, 8) were written"


def test_fused_mutants_are_caught():
    for V, R in [(257, 255), (513, 257)]:
        for eps in (0.0, 0.1):
            c = fused_case(V, R, 64, eps, True, 1)
            r64, r32 = c["r64"], c["r32"]
            Ep = c["E"][V:V + 3].to(F64) + 1.0                     # what non-zero pad rows of E would add
            pad = c["h"].to(F64) @ Ep.t()
            muts = _ce_mutants(c["z64"], c["tgt"], 1, eps, 1.0, V, pad=pad)
            assert set(muts) >= {"last column dropped", "pad columns included", "target off by one", "ignore_index row counted"}
            assert eps == 0.0 or "eps/V term omitted" in muts
            for name, m in muts.items():
                if "lse" in m:
                    assert_sensitive(name, r64["lse"], r32["lse"], m["lse"], extra=c["a_lse"], cap=FUSED_LSE_CAP)
                if "loss" in m:
                    assert_sensitive(name, r64["loss"], r32["loss"], m["loss"], extra=c["a_lse"], cap=LOSS_CAP)
                assert_sensitive(name, r64["dz"], r32["dz"], m["dz"], bf16=True, extra=c["a_dz"])
            # the bias left out of the row sums behind the smoothed loss
            assert_sensitive("bias left out of part_sum", r64["zsum"], r32["zsum"], r64["zsum"] - c["bias"].to(F64).sum())


@gpu
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("R", FUSED_R)
@pytest.mark.parametrize("V", FUSED_V)
def test_fused_ce_tile_edges(K, V, R, eps, with_bias):
    """V on both sides of the 256-column tile and of the 8-column group, R on both sides of the 256-row tile, d = 64: row_lse per
    row, count, loss (with eps > 0 it is driven by part_sum, whose row totals are checked as well) and every dlogits column."""
    ignore = 1 if (V + R) % 2 else -100
    c = fused_case(V, R, 64, eps, with_bias, ignore)
    what = f"fused V={V} R={R} eps={eps} bias={with_bias} ignore={ignore}"
    dev, lse, acc, ps = fused_fwd(K, c)
    ce_compare(what, c, lse, acc, None, lse_cap=FUSED_LSE_CAP)
    if eps:
        check(f"{what} part_sum row totals", host(ps).to(F64).sum(1), c["r64"]["zsum"], c["r32"]["zsum"])
    dl = fused_dlogits(K, c, dev, lse, acc, 0, V)
    fused_compare_dl(what, c, dl, 0, V)
    ign = c["tgt"] == ignore
    assert (host(dl)[ign][:, :V] == 0).all(), "ignored rows carry no gradient"


@gpu
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_fused_ce_d72_and_grad_scaling(K, eps):
    """d = 72 (K no multiple of 32); grad_out as a device scalar and grad_scale != 1."""
    c = fused_case(257, 37, 72, eps, True, -100, g=0.75 * 2.5)
    what = f"fused V=257 R=37 d=72 eps={eps}"
    dev, lse, acc, ps = fused_fwd(K, c)
    ce_compare(what, c, lse, acc, None, lse_cap=FUSED_LSE_CAP)
    fused_compare_dl(what, c, fused_dlogits(K, c, dev, lse, acc, 0, 257, grad_out=0.75, grad_scale=2.5), 0, 257)


@gpu
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("col0,ncols", [(8, 250), (104, 301), (256, 257)])
def test_fused_dlogits_chunks(K, col0, ncols, eps):
    """chunks that start off the 256-column grid and are no multiple of 8 wide; targets on the chunk's first and last column and
    one column outside either end; pad columns zero, everything behind them untouched."""
    V, R = 513, 37
    c = dict(fused_case(V, R, 64, eps, True, 1))
    tgt = c["tgt"].clone()
    tgt[20:24] = torch.tensor([col0 - 1, col0, col0 + ncols - 1, min(col0 + ncols, V - 1)])
    z64 = c["z64"]
    c.update(tgt=tgt, r64=ce_formula(z64, tgt, 1, eps), r32=ce_formula(z64.to(F32), tgt, 1, eps))
    c["a_lse"], c["a_dz"] = ce_allowances(z64, V, FUSED_NFAC, 1.0, c["r64"]["count"])
    dev, lse, acc, _ = fused_fwd(K, c)
    dl = fused_dlogits(K, c, dev, lse, acc, col0, ncols)
    fused_compare_dl(f"fused V=513 R=37 eps={eps} chunk", c, dl, col0, ncols)


@gpu
@pytest.mark.parametrize("V,R", [(257, 255), (513, 257)])
def test_fused_matches_materialised(K, V, R):
    """the two paths on the same float64-derived logits (the materialised one reads them rounded to fp32, 2^-24 |z| per logit):
    row_lse within the sum of the two margins."""
    c = fused_case(V, R, 64, 0.1, True, 1)
    _, lse_f, acc_f, _ = fused_fwd(K, c)
    z32 = c["z64"].to(F32)
    ldl = round_up(V, 4)
    lg = torch.zeros(R, ldl); lg[:, :V] = z32
    lse_m, acc_m = K.ce_fwd(lg.cuda(), c["tgt"].cuda(), V, ignore_index=1, label_smoothing=0.1)
    torch.cuda.synchronize()
    m64, m32 = ce_formula(z32.to(F64), c["tgt"], 1, 0.1), ce_formula(z32, c["tgt"], 1, 0.1)
    a_m, _ = ce_allowances(z32.to(F64), V, math.ceil(V / 256) + 2, 1.0, m64["count"])
    bound = ((f32_margin(c["r64"]["lse"], c["r32"]["lse"]) + c["a_lse"]) + (f32_margin(m64["lse"], m32["lse"]) + a_m)
             + 2.0 ** -24 * c["z64"].abs().max().item())
    err = (host(lse_f).to(F64) - host(lse_m).to(F64)).abs().max().item()
    print(f"LOSSCHK fused-vs-materialised V={V} R={R} row_lse ({R},) bound={bound:.3e} err={err:.3e}")
    assert err <= bound
    assert host(acc_f)[1].item() == host(acc_m)[1].item() == c["r64"]["count"]
    lf, lm = (host(acc_f)[0] / host(acc_f)[1]).item(), (host(acc_m)[0] / host(acc_m)[1]).item()
    print(f"LOSSCHK fused-vs-materialised V={V} R={R} loss () bound={bound:.3e} err={abs(lf - lm):.3e}")
    assert abs(lf - lm) <= bound


@gpu
@pytest.mark.parametrize("V,R", [(257, 255), (513, 257)])
def test_fused_autograd_dh_dE(K, V, R):
    """ops.lm_head_ce: loss, dh and dE against float64 autograd.  dh = bf16(sum_j dl_j E_j) and dE = sum_r dl_r h_r are formed
    from the bf16-rounded dlogits: each product carries that rounding (2^-8 |dl| |E| resp. 2^-8 |dl| |h|, summed), dh one more
    of its own; both are also held to the gates of the existing fused test."""
    from vacnic_amd import ops
    eps, d = 0.1, 64
    c = fused_case(V, R, d, eps, False, 1)
    h64 = c["h"].to(F64).requires_grad_(True); E64 = c["E"][:V].to(F64).requires_grad_(True)
    F.cross_entropy(h64 @ E64.t(), c["tgt"], ignore_index=1, label_smoothing=eps).backward()
    h32 = c["h"].to(F32).requires_grad_(True); E32 = c["E"][:V].to(F32).requires_grad_(True)
    F.cross_entropy(h32 @ E32.t(), c["tgt"], ignore_index=1, label_smoothing=eps).backward()
    dl_abs = c["r64"]["dz"].abs()
    egrad = torch.zeros(c["Vp"], d, device="cuda")
    hh = c["h"].cuda().requires_grad_(True)
    anchor = torch.zeros(1, device="cuda", requires_grad=True)
    loss, _ = ops.lm_head_ce(hh, anchor, c["E"].cuda(), egrad, c["tgt"].cuda(), V, 1, label_smoothing=eps)
    loss.backward()
    torch.cuda.synchronize()
    what = f"lm_head_ce V={V} R={R}"
    check(f"{what} loss", loss, c["r64"]["loss"], c["r32"]["loss"], extra=c["a_lse"], cap=LOSS_CAP)
    a_dh = (dl_abs + c["a_dz"]) @ c["E"][:V].to(F64).abs() * 2.0 ** -8 + c["a_dz"] @ c["E"][:V].to(F64).abs()
    check(f"{what} dh", hh.grad, h64.grad, h32.grad, bf16=True, extra=a_dh, cap=(3e-2, 2e-2 * h64.grad.abs().max().item()))
    a_dE = (dl_abs + c["a_dz"]).t() @ c["h"].to(F64).abs() * 2.0 ** -8 + c["a_dz"].t() @ c["h"].to(F64).abs()
    check(f"{what} dE", egrad[:V], E64.grad, E32.grad, extra=a_dE, cap=(3e-2, 2e-2 * E64.grad.abs().max().item()))
    assert (host(egrad)[V:] == 0).all()


# --------------------------------------------------------------------------------------------------- CoLaM
COLAM_SHAPES = [(1, 1, 8), (3, 7, 8), (4, 9, 520), (2, 1024, 64), (3, 17, 2056)]
_COLAM = {}


def colam_ref(hs, hg, mask, margin, g, dt):
    """pooled = nan_to_num(sum_t mask h / sum_t mask, nan=1) (an all-masked sample pools to ones and takes no gradient),
    cos = <a, b> / (|a| |b|), loss = mean_b max(0, margin - cos); dhs = d (g loss) / d hs."""
    a = hs.to(dt).requires_grad_(True); b = hg.to(dt)
    m = mask.to(dt)[..., None]; cnt = mask.sum(1).to(dt)[:, None]

    def pool(h):
        return torch.where(cnt > 0, (h * m).sum(1) / cnt.clamp(min=1), torch.ones_like(cnt))
    ps, pg = pool(a), pool(b)
    cos = (ps * pg).sum(1) / (ps.norm(dim=1) * pg.norm(dim=1))
    loss = (margin - cos).clamp(min=0).mean()
    (loss * g).backward()
    return dict(ps=ps.detach(), pg=pg.detach(), cos=cos.detach(), loss=loss.detach(), dhs=a.grad)


def colam_case(B, T, D):
    if (B, T, D) in _COLAM:
        return _COLAM[(B, T, D)]
    hs = cpu_randn(B, T, D, seed=B * 100 + T)
    hg = (hs.float() * 0.6 + cpu_randn(B, T, D, seed=B * 100 + T + 1, dtype=F32) * 0.8).to(BF16)
    kinds = {1: ["full"], 2: ["none", "full"]}.get(B, ["none", "single", "full", "ragged"][:B])
    mask = torch.zeros(B, T, dtype=torch.uint8)
    for b, kind in enumerate(kinds):
        if kind == "full":
            mask[b] = 1
        elif kind == "single":
            mask[b, T - 2] = 1
        elif kind == "ragged":
            mask[b, 1::2] = 1
    cos64 = colam_ref(hs, hg, mask, 0.0, 1.0, F64)["cos"]
    cos32 = colam_ref(hs, hg, mask, 0.0, 1.0, F32)["cos"]
    cm = f32_margin(cos64, cos32)
    live = torch.tensor([k != "none" for k in kinds])
    srt = (cos64[live] if live.sum() > 1 else cos64).sort().values
    margins = [1.5, -1.5]                                 # above and below every sample's cos
    if B > 1:                                             # and between two of them (two that take a gradient, where there are
                                                          # two): the middle of the widest gap
        gaps = srt[1:] - srt[:-1]
        k = int(gaps.argmax())
        margins.append(float(np.float32((srt[k] + srt[k + 1]).item() / 2)))
    c = dict(B=B, T=T, D=D, hs=hs, hg=hg, mask=mask, kinds=kinds, margins=margins, cos64=cos64, cos_margin=cm)
    _COLAM[(B, T, D)] = c
    return c


@pytest.mark.parametrize("B,T,D", COLAM_SHAPES)
def test_colam_hinge_sides_are_decided(B, T, D):
    """every |margin - cos| is at least 1000x the fp32 margin of cos, and each sample has a margin on either side of its cos."""
    c = colam_case(B, T, D)
    for mg in c["margins"]:
        gap = (mg - c["cos64"]).abs().min().item()
        assert gap >= 1000 * c["cos_margin"], (mg, gap, c["cos_margin"])
    assert (c["cos64"] < max(c["margins"])).all() and (c["cos64"] > min(c["margins"])).all()
    if B > 1:
        side = c["margins"][2] > c["cos64"]
        assert side.any() and not side.all()
    for b, kind in enumerate(c["kinds"]):
        if kind == "none":
            assert abs(c["cos64"][b].item() - 1.0) < 1e-12


def test_colam_mutants_are_caught():
    c = colam_case(4, 9, 520)
    hs, hg, mask = c["hs"], c["hg"], c["mask"]
    mg, g = c["margins"][0], 1.25
    r64, r32 = colam_ref(hs, hg, mask, mg, g, F64), colam_ref(hs, hg, mask, mg, g, F32)
    full = torch.ones_like(mask); full[0] = 0
    ign = colam_ref(hs, hg, full, mg, g, F64)                                     # mask ignored in the pool
    cnt = mask.sum(1).to(F64)[:, None]
    scale = torch.where(cnt > 0, cnt / mask.shape[1], torch.ones_like(cnt))       # mean over T instead of the mask count
    mut = {"mask ignored in the pool": dict(ps=ign["ps"], pg=ign["pg"], cos=ign["cos"], loss=ign["loss"], dhs=ign["dhs"]),
           "mean over T": dict(ps=r64["ps"] * scale, pg=r64["pg"] * scale, dhs=r64["dhs"] * scale[:, None])}
    for name, m in mut.items():
        for key, v in m.items():
            assert_sensitive(f"{name} {key}", r64[key], r32[key], v, bf16=key == "dhs")
    # the hinge taken on the wrong side
    mid = c["margins"][2]
    a64, a32 = colam_ref(hs, hg, mask, mid, g, F64), colam_ref(hs, hg, mask, mid, g, F32)
    assert_sensitive("hinge always active", a64["dhs"], a32["dhs"], r64["dhs"], bf16=True)


@gpu
@pytest.mark.parametrize("B,T,D", COLAM_SHAPES)
def test_colam(K, B, T, D):
    """T = 1 and T % 8 != 0 (the clamped rows of the 8-token batches), T = 1024 (the LDS limit), D = 2056 (thread 0 owns two
    chunks); an all-masked sample (cos = 1, pooled = 1, loss term max(0, margin - 1), zero gradient), a single token, a full mask."""
    c = colam_case(B, T, D)
    hs, hg, mask = c["hs"].cuda(), c["hg"].cuda(), c["mask"].cuda()
    for i, mg in enumerate(c["margins"]):
        go, gs = (None, 1.0) if i == 0 else (0.75, 2.5)
        g = 1.0 if go is None else go * gs
        r64, r32 = colam_ref(c["hs"], c["hg"], c["mask"], mg, g, F64), colam_ref(c["hs"], c["hg"], c["mask"], mg, g, F32)
        loss, cos, ps, pg = K.colam_fwd(hs, hg, mask, mg)
        dhs = K.colam_bwd(cos, ps, pg, mask, (B, T, D), mg, None if go is None else torch.tensor(go, device="cuda"), gs)
        torch.cuda.synchronize()
        what = f"colam B={B} T={T} D={D} margin={mg:.4f}"
        for key, got in (("cos", cos), ("ps", ps), ("pg", pg), ("loss", loss)):
            check(f"{what} {key}", got, r64[key], r32[key])
        check(f"{what} dhs", dhs, r64["dhs"], r32["dhs"], bf16=True)
        dh = host(dhs)
        assert (dh[c["mask"] == 0] == 0).all(), "masked positions of dhs must be exactly zero"
        for b, kind in enumerate(c["kinds"]):
            if kind == "none":
                assert (host(ps)[b] == 1).all() and (host(pg)[b] == 1).all() and (dh[b] == 0).all()
        if mg < -1:
            assert (dh == 0).all() and host(loss).item() == 0.0


@gpu
def test_colam_refusals(K):
    m = torch.ones(2, 1025, dtype=torch.uint8, device="cuda")
    h = torch.ones(2, 1025, 8, device="cuda", dtype=BF16)
    with pytest.raises(ValueError, match="T <= 1024"):
        K.colam_fwd(h, h, m, 0.5)
    h = torch.ones(2, 4, 12, device="cuda", dtype=BF16)
    with pytest.raises(ValueError, match="D % 8 == 0"):
        K.colam_fwd(h, h, m[:, :4].contiguous(), 0.5)


# --------------------------------------------------------------------------------------------------- SECLA
SECLA_SHAPES = [(1, 1, 1, 8), (2, 3, 1, 8), (5, 1, 3, 520), (3, 7, 2, 64), (8, 4, 6, 1024)]
_SECLA = {}


def _log_softmax_rows(x):
    m = x.max(1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(1, keepdims=True))


def secla_model(faces, names, g=1.0, dt=np.float64, last=False):
    """numpy model of loss.hip's SECLA: sim[i][n][j][f] = <names[i][n], faces[j][f]>; l1[i][j] = mean_n max_f sim[i][n][j][f];
    l2[i][j] = mean_f max_n sim[j][n][i][f]; loss = CE(l1, arange) + CE(l2, arange); the gradient is routed through the arg-max
    entries, the LOWEST index among tied maxima (last=True: the highest, a mutant); dfaces[j][f] = sum_{i,n} wsim[i][n][j][f] names[i][n]."""
    faces, names = np.asarray(faces, dtype=dt), np.asarray(names, dtype=dt)
    B, Fn, D = faces.shape
    N = names.shape[1]
    sim = np.einsum("ind,jfd->injf", names, faces).astype(dt)
    l1 = (sim.max(3).sum(1) / dt(N)).astype(dt)                               # [i][j]
    l2 = (sim.max(1).sum(2) / dt(Fn)).T.astype(dt)                            # sim.max(1): [i][j][f] -> sum_f -> [i][j] = l2[j][i]
    ls1, ls2 = _log_softmax_rows(l1), _log_softmax_rows(l2)
    loss = -(np.trace(ls1) + np.trace(ls2)) / dt(B)

    def first_argmax(a, axis):
        if not last:
            return a.argmax(axis)
        return a.shape[axis] - 1 - np.flip(a, axis).argmax(axis)
    eye = np.eye(B, dtype=dt)
    w = np.zeros_like(sim)
    am1 = first_argmax(sim, 3)                                                # [i][n][j]
    t1 = dt(g) / dt(B) * (np.exp(ls1) - eye) / dt(N)                          # [i][j]
    ii, nn, jj = np.meshgrid(np.arange(B), np.arange(N), np.arange(B), indexing="ij")
    np.add.at(w, (ii, nn, jj, am1), np.broadcast_to(t1[:, None, :], am1.shape))
    am2 = first_argmax(sim, 1)                                                # [i][j][f]
    t2 = dt(g) / dt(B) * (np.exp(ls2).T - eye) / dt(Fn)                       # [i][j] = softmax(l2[j])[i] - [i == j]
    ii, jj, ff = np.meshgrid(np.arange(B), np.arange(B), np.arange(Fn), indexing="ij")
    np.add.at(w, (ii, am2, jj, ff), np.broadcast_to(t2[:, :, None], am2.shape))
    dfaces = np.einsum("injf,ind->jfd", w, names).astype(dt)
    return dict(sim=sim, l1=l1, l2=l2, loss=np.asarray(loss, dtype=dt), wsim=w, dfaces=dfaces)


def secla_case(B, Fn, N, D, dense=False):
    """integers times a power of two: every sim is exact in fp32 (|sim| <= 2 D 2^-k), so ties and the routing are the same in
    every precision.  Duplicated faces and names put ties on both arg-max axes.  dense: D = 8, F = 2, face (j, 1) = face (j, 0),
    so face (j, 0) wins the arg-max over f of every (i, n) and its column holds B * N non-zero weights."""
    key = (B, Fn, N, D, dense)
    if key in _SECLA:
        return _SECLA[key]
    scale = 2.0 ** -(int(math.log2(D)) // 2 + (2 if dense else 0))
    faces = cpu_randint(-2, 3, (B, Fn, D), seed=B * 31 + D).to(BF16)
    names = cpu_randint(-1, 2, (B, N, D), seed=B * 37 + D + 1).to(F32) * scale
    if dense:
        faces[:, 1] = faces[:, 0]
    else:
        if Fn > 2:
            faces[:, Fn - 1] = faces[:, 1]                      # padded faces are identical rows
        if N > 1:
            names[:, N - 1] = names[:, 0]
        if B > 2:
            faces[2] = faces[0]
    f64, n64 = faces.to(F64).numpy(), names.to(F64).numpy()
    c = dict(B=B, F=Fn, N=N, D=D, faces=faces, names=names, f64=f64, n64=n64)
    _SECLA[key] = c
    return c


def test_secla_model_is_torch_autograd_without_ties():
    """the routing model against torch autograd of the BatchSoftmax graph (test_kernels_gpu.py::test_secla) on random float64
    data, where no two sims tie."""
    B, Fn, N, D = 4, 3, 5, 16
    faces = cpu_randn(B, Fn, D, seed=1, dtype=F64); names = cpu_randn(B, N, D, seed=2, dtype=F64)
    ff = faces.clone().requires_grad_(True)

    def batch_softmax(m):
        logits = m.max(-1).values.sum(-1) / m.shape[2]
        return F.cross_entropy(logits, torch.arange(m.shape[0]))
    m1 = torch.matmul(names.unsqueeze(1), ff.permute(0, 2, 1)); m2 = torch.matmul(ff.unsqueeze(1), names.permute(0, 2, 1))
    ref = batch_softmax(m1) + batch_softmax(m2)
    (ref * 1.7).backward()
    r = secla_model(faces.numpy(), names.numpy(), g=1.7)
    assert abs(r["loss"] - ref.item()) < 1e-12
    assert np.abs(r["dfaces"] - ff.grad.numpy()).max() < 1e-13
    assert np.abs(r["dfaces"] - secla_model(faces.numpy(), names.numpy(), g=1.7, last=True)["dfaces"]).max() == 0    # no ties


@pytest.mark.parametrize("B,Fn,N,D", SECLA_SHAPES)
def test_secla_cases_are_exact_and_hold_ties(B, Fn, N, D):
    c = secla_case(B, Fn, N, D)
    r64, r32 = secla_model(c["f64"], c["n64"]), secla_model(c["f64"], c["n64"], dt=np.float32)
    assert np.array_equal(r64["sim"], r32["sim"].astype(np.float64)), "sim is not exact in fp32"
    assert np.array_equal(r64["wsim"] != 0, r32["wsim"] != 0)
    if B * Fn * N > 1:
        s = r64["sim"]
        assert ((s == s.max(3, keepdims=True)).sum(3) > 1).any() or Fn == 1
        assert ((s == s.max(1, keepdims=True)).sum(1) > 1).any() or N == 1


def test_secla_mutants_are_caught():
    c = secla_case(8, 4, 6, 1024)
    r64, r32 = secla_model(c["f64"], c["n64"], g=2.0), secla_model(c["f64"], c["n64"], g=2.0, dt=np.float32)
    last = secla_model(c["f64"], c["n64"], g=2.0, last=True)
    assert_sensitive("tie routed to the last index", r64["dfaces"], r32["dfaces"], last["dfaces"], bf16=True)
    assert_sensitive("l1 / l2 swapped", r64["l1"], r32["l1"], r64["l2"])
    assert_sensitive("l1 / l2 swapped", r64["l2"], r32["l2"], r64["l1"])
    assert_sensitive("1/N vs 1/F swapped", r64["l1"], r32["l1"], r64["l1"] * c["N"] / c["F"])
    assert_sensitive("1/N vs 1/F swapped", r64["l2"], r32["l2"], r64["l2"] * c["F"] / c["N"])
    assert_sensitive("loss of one direction only", r64["loss"], r32["loss"], r64["loss"] / 2)
    d = secla_case(32, 2, 32, 8, dense=True)
    r = secla_model(d["f64"], d["n64"])
    assert_sensitive("dense column cut at 1024 rows", r["dfaces"], secla_model(d["f64"], d["n64"], dt=np.float32)["dfaces"],
                     r["dfaces"] * 0.5, bf16=True)


@pytest.mark.parametrize("B,nnz", [(32, 1024), (33, 1056)])
def test_secla_dense_columns_hold_b_times_n_weights(B, nnz):
    c = secla_case(B, 2, 32, 8, dense=True)
    for dt in (np.float64, np.float32):
        w = secla_model(c["f64"], c["n64"], dt=dt)["wsim"].reshape(B * 32, B * 2)
        cols = (w != 0).sum(0)
        assert (cols[0::2] == nnz).all(), cols[:6]                  # face (j, 0): every (i, n)
        assert (cols[1::2] <= B).all() and (cols[1::2] > 0).all()   # face (j, 1): the arg-max over n of every i only


def secla_run_and_compare(K, c, what, go, gs):
    B, Fn, N, D = c["B"], c["F"], c["N"], c["D"]
    g = 1.0 if go is None else go * gs
    r64, r32 = secla_model(c["f64"], c["n64"], g=g), secla_model(c["f64"], c["n64"], g=g, dt=np.float32)
    faces, names = c["faces"].cuda(), c["names"].cuda()
    loss, sim, l1, l2 = K.secla_fwd(faces, names)
    df = K.secla_bwd(faces, names, sim, l1, l2, None if go is None else torch.tensor(go, device="cuda"), gs)
    torch.cuda.synchronize()
    check_equal(f"{what} sim", sim, torch.from_numpy(r64["sim"]).to(F32))
    for key, got in (("l1", l1), ("l2", l2), ("loss", loss)):
        check(f"{what} {key}", got, r64[key], r32[key])
    check(f"{what} dfaces", df, r64["dfaces"], r32["dfaces"], bf16=True)


@gpu
@pytest.mark.parametrize("B,Fn,N,D", SECLA_SHAPES)
def test_secla(K, B, Fn, N, D):
    """B * F off the 16-face groups of the sim kernel, D = 520 (lane 0 alone in a second trip), ties on both arg-max axes."""
    c = secla_case(B, Fn, N, D)
    secla_run_and_compare(K, c, f"secla B={B} F={Fn} N={N} D={D}", None, 1.0)
    secla_run_and_compare(K, c, f"secla B={B} F={Fn} N={N} D={D} grad_out=0.75 grad_scale=2.5", 0.75, 2.5)


@gpu
@pytest.mark.parametrize("B", [32, 33])
def test_secla_dense_column(K, B):
    """B * N = 1024: the last size the compaction holds; 1056: the dense walk of secla_dfaces_kernel."""
    c = secla_case(B, 2, 32, 8, dense=True)
    secla_run_and_compare(K, c, f"secla dense B={B} F=2 N=32 D=8 (B*N={B * 32})", None, 1.0)


# ------------------------------------------------------------------------------------------ combine_losses
def combine_ref(ce_sum, count, secla, colam, ws, wc, dt):
    v = [torch.tensor(x, dtype=dt) for x in (ce_sum, count, 0.0 if secla is None else secla, 0.0 if colam is None else colam)]
    txt = v[0] / v[1]
    return torch.stack([txt + torch.tensor(ws, dtype=dt) * v[2] + torch.tensor(wc, dtype=dt) * v[3], txt, v[2], v[3]])


def test_combine_mutants_are_caught():
    r64, r32 = combine_ref(1234.5, 321.0, 0.7, 1.9, 0.3, 2.5, F64), combine_ref(1234.5, 321.0, 0.7, 1.9, 0.3, 2.5, F32)
    assert_sensitive("weights swapped", r64, r32, combine_ref(1234.5, 321.0, 0.7, 1.9, 2.5, 0.3, F64))
    assert_sensitive("weights taken as 1", r64, r32, combine_ref(1234.5, 321.0, 0.7, 1.9, 1.0, 1.0, F64))


@gpu
@pytest.mark.parametrize("secla,colam", [(0.7, 1.9), (None, 1.9), (0.7, None), (None, None)])
def test_combine_losses(K, secla, colam):
    acc = torch.tensor([1234.5, 321.0], device="cuda")
    s = None if secla is None else torch.tensor(secla, device="cuda")
    c = None if colam is None else torch.tensor(colam, device="cuda")
    out = K.combine_losses(acc.data_ptr(), acc.data_ptr() + 4, s, c, 0.3, 2.5, "cuda")
    torch.cuda.synchronize()
    check(f"combine_losses secla={secla} colam={colam}", out, combine_ref(1234.5, 321.0, secla, colam, 0.3, 2.5, F64),
          combine_ref(1234.5, 321.0, secla, colam, 0.3, 2.5, F32))
    acc0 = torch.zeros(2, device="cuda")                     # no valid target: 0 / 0 is NaN, like torch's mean over nothing
    out = host(K.combine_losses(acc0.data_ptr(), acc0.data_ptr() + 4, s, c, 0.3, 2.5, "cuda"))
    assert torch.isnan(out[:2]).all()
    assert out[2].item() == np.float32(secla or 0.0) and out[3].item() == np.float32(colam or 0.0)
