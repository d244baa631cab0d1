"""GEMM family (csrc/gemm.hip, gemm_kernel.h): every dispatch edge against float64 on the CPU.  Inputs are built on the CPU,
references are computed on the CPU in float64 from the logical operands; nothing is taken from a kernel's output.  The unmarked
tests run without a GPU: the dispatch plan (vacnic_gemm_plan: the launch path's own decision code) proves that the shapes used
below take the paths they are named after, every reference is shown to differ from its wrong variants ("mutants"), and no bound
is looser than the older check of the same quantity.

Exact regime (most checks).  Operands, bias, residual and the initial accumulator are small integers (exact in bf16), alpha is a
power of two.  Every product and every partial sum, in any order, is then an integer multiple of alpha below 2^24 * alpha, i.e.
exact in fp32 (`assert_exact_regime` checks sum_k |x||w| + |bias| + |residual| + |acc| < 2^24 on the reference).  fp32 outputs,
atomic and fix-up split-K, xsum and wgrad_group must equal the float64 result bit for bit (bound=0 in the log); bf16 outputs must
equal its round-to-nearest-even.  The bf16 transposed epilogue of the 256-row tiles rounds the bias-added value to bf16 BEFORE it
adds a residual, multiplies by act' or saves the pre-activation; in the checks that carry such an operand the pre-activation is an
integer of magnitude <= 256 (resp. a multiple of 1/8 of magnitude <= 32), which bf16 holds exactly, so both epilogues must give
RNE(u + residual); `assert u.abs().max() <= 256` precedes those comparisons.

Activation paths.  Pre-activations are exact multiples of 1/8 (alpha = 0.125, |u| <= 32), so the only errors are the activation
formula and the roundings to bf16:  |got - ref64| <= 2^-8 |ref| (+ 2^-8 |act(u)| where a residual is added to an already rounded
value) + allowance, ref64 = the true activation in float64 (erf-GELU, tanh, x sigmoid(1.702 x)).  Allowance, from common.h and
the compiler's __clang_hip_math.h (__expf(x) = exp2_native(fl(log2e x)), within 2^-23 (1 + |x|) relative of exp(x), as derived in
test_loss_gpu.py; fast_rcp = v_rcp_f32, taken as 1 ulp = 2^-23 relative):
  * formula: erf_abs is Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7, so gelu_fwd carries 0.5 |x| 1.5e-7 and gelu_bwd 0.5 * 1.5e-7;
    tanh_fast and the quick-GELU are exact identities.
  * native operations: every intermediate of act / act' (t, e, poly, er, e2, s, x pdf(x), 1.702 x s (1 - s)) is at most
    max(1, |x|) in magnitude and is produced by at most 8 operations (v_exp, v_rcp, fp32 multiply-adds), each within
    2^-23 (1 + |arg|) relative, |arg| <= max(x^2 / 2, 2 |x|, 1.702 |x|) <= (1 + |x|)^2 / 2 + 1.  So
        A_fwd(x) = 8 * 2^-23 * (1 + |x|)^2 * max(|act(x)|, 2^-6)       (relative to the result, with an absolute floor for the tails)
        A_bwd(x) = 8 * 2^-23 * (1 + |x|)^2                              (act' is O(1))
    and a backward element gets |g| A_bwd(d).  At |x| = 6 these are 4.7e-5: about 1 % of the bf16 rounding term.
  * what is not derived (the fp32 evaluation order of the polynomial and the final products) is measured as the project's rule
    says: 8x the deviation of THE SAME formula evaluated in fp32 on the CPU (numpy float32) from its float64 evaluation at that
    shape.  Never from the kernel.
  * no bound is looser than the older check of the same quantity in test_kernels_gpu.py (forward 1e-2 |ref| + 1e-2, backward
    2e-2 |ref| + 2e-2): the bound is the smaller of the two, and test_bounds_are_not_looser_than_the_older_checks asserts that the
    cap never binds on the data used here.

gemv_ln.  Reference 1 is the bit identity with add_ln_fwd + skinny GEMM.  Reference 2 follows the kernel comment in float64:
LayerNorm in float64, rounded to bf16, dot in float64.  Margin: the LayerNorm rule of test_norm_gpu.py (8x the deviation of the
same pipeline in fp32 torch on the CPU from float64, floored at 1e-6 max|ref|), plus, because the kernel's fp32 LayerNorm may
round a normalised value to the OTHER bf16 neighbour when the float64 value lies within the LayerNorm margin of a rounding
boundary, sum_k near[m,k] ulp_bf16(h[m,k]) |w[n,k]| for exactly those elements; bf16 outputs get 2^-8 |ref| on top.

Canaries: every output buffer (out, preact, xsum, the fp32 accumulator, dW, dbias) is allocated with 8 extra rows and, where
ldo > N, extra columns, all filled with 0.3125 (exact in bf16, not a multiple of 1/8); they must be untouched after every launch,
read-only operands must be unchanged, and the arrival counters of the fix-up are zero after every launch.

Every check prints `GEMMCHK <what> <shape> bound=<margin> err=<observed>`; profiles/gemm_tests.txt holds one MI355X run.

Measured on the MI355X in that run: 2256 of the 2542 checks are exact (bound=0).  Largest share of its bound that any element uses:
bf16 outputs behind an activation 0.98 - 0.99 (2^-8 |ref| is exactly half a bf16 ulp at the bottom of a binade, so a correct
rounding comes that close), gemv_ln ln_out 0.993, fix-up + gelu 0.84, fused dropout + gelu 0.84.

What the suite found (eight gaps read off the code before it was written):
  1. row split x fused activation dropout: CONFIRMED.  Without the rule "no row split while drop_p != 0" in gemm_dispatch,
     test_fused_dropout_at_the_row_split_shape fails: the dgrad under the cost model differs from the host mask in 23789 of
     16908288 elements, the first at (4096, 5) = m_main.  Fixed on the host (the DR tiles are 256 x 256 / 64 x 128 anyway).
  2. test_gemm_row_split_dispatch did not split: CONFIRMED by test_plan_row_split_shapes; moved to 8224 x 2048 x 512.
  3. atomic split-K dropped act / preact / dact_src / residual: CONFIRMED by reading; now VACNIC_UNSUPPORTED
     (test_refusals_decided_on_the_host, test_atomic_split_refuses_epilogue_operands).
  4. K % 8 != 0, 5. garbage in the pad columns of K-strided operands, 6. a split above ceil(K / 64), 7. alpha with bias in all five
     epilogues: REFUTED (test_k_schedule_per_loop, test_tile_edges, test_split_k, test_epilogues_exact, test_skinny pass unchanged).
  8. alignment of out / preact / dact_src / residual: CONFIRMED by reading (16-byte row accesses whenever ldo % 8 == 0, 8-byte
     bf16 stores of the register epilogue when ldo % 4 == 0, 16-byte fp32 stores when ldo % 4 == 0); now VACNIC_MISALIGNED, and
     a stride that rules the vector accesses out takes the element-wise path (test_misaligned_epilogue_operands_are_refused_or_routed).
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from test_norm_gpu import flat_keep, drop_threshold, inv_keep_of, mix_seed, philox4x32_10  # noqa: F401  (host Philox model)

gpu = pytest.mark.gpu
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
CANARY = 0.3125
TILE = {64: (64, 128), 128: (128, 128), 256: (256, 256), 258: (256, 256), 260: (256, 256), 261: (128, 128), 262: (256, 256),
        264: (256, 128)}
HINTS = sorted(TILE)
LAYOUTS = ("NN", "NT", "TN", "TT")          # X then W: N = K-contiguous, T = K-strided
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the shape of the row-split tests: the smallest tail the cost model cuts off at N = 4096 (test_plan_row_split_shapes)
SPLIT_SHAPE = (4128, 4096, 512)
SPLIT_MAIN = 4096


def layouts_of(hint):
    return ("NN",) if hint == 258 else LAYOUTS          # the 8-phase loop exists for the forward layout only


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


def plan(**kw):
    from vacnic_amd import kernels
    M, N, K_ = kw.pop("M"), kw.pop("N"), kw.pop("K")
    return kernels.gemm_plan(M, N, K_, **kw)


# ------------------------------------------------------------------------------------------------ data
def round8(n):
    return (n + 7) // 8 * 8


def ints(shape, lo, hi, seed):
    """seeded integers in [lo, hi] as float64: position-dependent, so a misplaced fragment shows"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(F64)


def garbage(shape, seed):
    """finite, non-zero, bf16-exact values for padding that a kernel may read but must not use"""
    g = torch.Generator(device="cpu").manual_seed(seed + 7919)
    v = torch.randint(3, 10, tuple(shape), generator=g).to(F64)
    return v * (torch.randint(0, 2, tuple(shape), generator=g).to(F64) * 2 - 1)


def pack(logical, kstrided, ld_extra=0, kpad="garbage", seed=0):
    """the storage of a logical [R, K] operand: K-contiguous [R][ld] (pad columns [K, round8(K)): zero or garbage; everything
    beyond: garbage) or K-strided [K][ld] (pad columns [R, ld): garbage).  Returns (bf16 buffer, ld)."""
    R, Kd = logical.shape
    if kstrided:
        ld = round8(R) + ld_extra
        buf = garbage((Kd, ld), seed)
        buf[:, :R] = logical.t()
    else:
        ld = round8(Kd) + ld_extra
        buf = garbage((R, ld), seed)
        buf[:, :Kd] = logical
        if kpad == "zero":
            buf[:, Kd:round8(Kd)] = 0
    return buf.to(BF16), ld


def rne(t):
    """float64 -> nearest-even bf16 -> float64 (the values here are exact in fp32, so the fp32 step rounds nothing)"""
    t32 = t.to(F32)
    assert torch.equal(t32.to(F64), t), "reference not exact in fp32"
    return t32.to(BF16).to(F64)


def assert_exact_regime(X, W, alpha=1.0, bias=None, residual=None, acc0=None):
    top = (X.abs() @ W.abs().t()).max().item()
    top += 0 if bias is None else bias.abs().max().item() / abs(alpha)
    top += 0 if residual is None else residual.abs().max().item() / abs(alpha)
    top += 0 if acc0 is None else acc0.abs().max().item() / abs(alpha)
    assert top < 2 ** 24 and math.log2(abs(alpha)) == int(math.log2(abs(alpha))), "not in the exact regime"


def gemm_ref(X, W, alpha=1.0, bias=None):
    """u[m][n] = alpha sum_k X[m][k] W[n][k] + bias[n] in float64"""
    u = alpha * (X @ W.t())
    return u if bias is None else u + bias


# the wrong variants every reference is held against (test_mutants_*)
def mut_last_k_dropped(X, W, alpha=1.0, bias=None):
    return gemm_ref(X[:, :-1], W[:, :-1], alpha, bias)


def mut_pad_column_included(X, W, xpad, wpad, alpha=1.0, bias=None):
    return gemm_ref(torch.cat([X, xpad], 1), torch.cat([W, wpad], 1), alpha, bias)


def mut_bias_scaled(X, W, alpha, bias):
    return alpha * (X @ W.t() + bias)


def mut_slice1_twice(X, W, kps, alpha=1.0, bias=None):
    return gemm_ref(X, W, alpha, bias) + alpha * (X[:, kps:2 * kps] @ W[:, kps:2 * kps].t())


def keep_mask(M, N, seed, counter, thr):
    return torch.from_numpy(flat_keep(M * N, mix_seed(seed, counter), thr).reshape(M, N))


def mut_mask_restarted(keep, m_main):
    m = keep.clone()
    m[m_main:] = keep[:keep.shape[0] - m_main]
    return m


# ------------------------------------------------------------------------------------------- activations
ACTS = ("gelu", "tanh", "quick_gelu")
EXIST_FWD, EXIST_BWD = (1e-2, 1e-2), (2e-2, 2e-2)          # (rtol, atol) of the older checks in test_kernels_gpu.py
EXIST_RES = (1e-2, 2e-2)                                   # ... of an activation followed by a residual (test_gemm_row_split_dispatch)


def act_true(name, u, deriv=False):
    u = u.to(F64)
    if name is None:
        return torch.ones_like(u) if deriv else u
    if name == "gelu":
        cdf = 0.5 * (1 + torch.erf(u / math.sqrt(2)))
        return cdf + u * torch.exp(-u * u / 2) / math.sqrt(2 * math.pi) if deriv else u * cdf
    if name == "tanh":
        return 1 - torch.tanh(u) ** 2 if deriv else torch.tanh(u)
    s = torch.sigmoid(1.702 * u)
    return s + 1.702 * u * s * (1 - s) if deriv else u * s


def act_formula(name, u, dt, deriv=False):
    """the formulas of common.h (erf_abs / gelu_fwd / gelu_bwd / tanh_fast / quick-GELU) evaluated in numpy dtype `dt`"""
    c = lambda v: np.asarray(v, dtype=dt)                       # noqa: E731
    x = np.asarray(u.numpy(), dtype=dt)
    one = c(1)
    if name == "gelu":
        au = np.abs(x) * c(0.70710678118654752)
        t = one / (one + c(0.3275911) * au)
        e = np.exp(-au * au)
        poly = t * (c(0.254829592) + t * (c(-0.284496736) + t * (c(1.421413741) + t * (c(-1.453152027) + t * c(1.061405429)))))
        er = np.copysign(one - poly * e, x)
        r = c(0.5) * (one + er) + x * c(0.3989422804014327) * e if deriv else c(0.5) * x * (one + er)
    elif name == "tanh":
        e2 = np.exp(c(-2) * np.abs(x))
        t = np.copysign((one - e2) * (one / (one + e2)), x)
        r = one - t * t if deriv else t
    else:
        s = one / (one + np.exp(c(-1.702) * x))
        r = s + c(1.702) * x * s * (one - s) if deriv else x * s
    return torch.from_numpy(np.asarray(r, dtype=np.float64))


def act_allow(name, u, deriv=False):
    """(per-element derived allowance, scalar measured fp32 margin) of act(u) / act'(u): module docstring"""
    if name is None:
        return torch.zeros_like(u), 0.0
    native = 8 * 2.0 ** -23 * (1 + u.abs()) ** 2
    if not deriv:
        native = native * torch.clamp(act_true(name, u).abs(), min=2.0 ** -6)
    formula = 0.0
    if name == "gelu":
        formula = 0.5 * 1.5e-7 * (torch.ones_like(u) if deriv else u.abs())
    measured = 8.0 * (act_formula(name, u, np.float32, deriv) - act_formula(name, u, np.float64, deriv)).abs().max().item()
    return native + formula, measured


def act_bound(name, u, ref, scale=None, deriv=False, extra_round=None):
    """per-element bound of a bf16 output ref = [scale *] act(u) [+ ...]: 2^-8 |ref| + allowance, never above the older check"""
    allow, measured = act_allow(name, u, deriv)
    s = 1.0 if scale is None else scale.abs()
    bound = 2.0 ** -8 * ref.abs() + s * (allow + measured)
    if extra_round is not None:
        bound = bound + 2.0 ** -8 * extra_round.abs()
    rt, at = EXIST_BWD if deriv else EXIST_RES if extra_round is not None else EXIST_FWD
    cap = rt * ref.abs() + at
    return torch.minimum(bound, cap), bool((bound <= cap).all())


# ------------------------------------------------------------------------------------------- the checks
def chk_equal(what, got, want):
    got, want = got.to(F64), want.to(F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs().max().item() if got.numel() else 0.0
    print(f"GEMMCHK {what} {tuple(want.shape)} bound=0.000e+00 err={err:.3e}")
    assert torch.equal(got, want), f"{what}: {(got != want).sum().item()}/{want.numel()} differ, max {err:.4g}, first at " \
                                   f"{tuple((got != want).nonzero()[0].tolist())}"


def chk_bound(what, got, ref, bound):
    got = got.to(F64)
    err = (got - ref).abs()
    used = torch.where(err > 0, err / bound, torch.zeros_like(err)).reshape(-1)
    k = int(torch.nan_to_num(used, nan=float("inf")).argmax())
    print(f"GEMMCHK {what} {tuple(ref.shape)} bound={bound.reshape(-1)[k].item():.3e} err={err.reshape(-1)[k].item():.3e} "
          f"maxerr={err.max().item():.3e} refmax={ref.abs().max().item():.3e} used={used[k].item():.3f}")
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    bad = (err > bound).sum().item()
    assert bad == 0, f"{what}: {bad}/{err.numel()} off, max err {err.max().item():.4g}"


def canary_ok(what, buf, M, N):
    """rows [M, M + 8) and columns [N, ld) still hold the canary"""
    b = buf.to(F64)
    assert bool((b[M:] == CANARY).all()), f"{what}: rows [M, M+8) were written"
    if b.dim() == 2:
        assert bool((b[:M, N:] == CANARY).all()), f"{what}: columns [N, ld) were written"


def run_gemm(K, X, W, layout="NN", hint=-1, *, bias=None, alpha=1.0, act=None, want_preact=False, dact=None, residual=None,
             out_mode=0, acc0=None, ldo_extra=0, ld_extra=(0, 0), kpad=("zero", "garbage"), split_k=1, fixup=False, xsum0=None,
             drop=None, seed=0):
    """one launch on logical operands X [M, K], W [N, K] (float64 holding bf16-exact values); returns the host copies of the
    outputs after checking every canary, every read-only operand and the fix-up counters."""
    M, Kd = X.shape
    N = W.shape[0]
    xk, wk = layout[0] == "T", layout[1] == "T"
    xb, ldx = pack(X, xk, ld_extra[0], kpad[0], seed + 1)
    wb, ldw = pack(W, wk, ld_extra[1], kpad[1], seed + 2)
    ldo = N + ldo_extra

    def obuf(dtype, init=None):
        t = torch.full((M + 8, ldo), CANARY, dtype=dtype)
        if init is not None:
            t[:M, :N] = init.to(dtype)
        return t
    odt = BF16 if out_mode == 0 else F32
    out = obuf(odt, acc0 if out_mode == 2 else torch.zeros(M, N, dtype=F64) + 0.4375)
    pre = obuf(BF16, torch.zeros(M, N, dtype=F64) + 0.4375) if want_preact else None
    dsrc = obuf(BF16, dact) if dact is not None else None
    res = obuf(BF16, residual) if residual is not None else None
    xs = None
    if xsum0 is not None:
        xs = torch.full((M + 8,), CANARY, dtype=F32)
        xs[:M] = xsum0.to(F32)
    dev = lambda t: None if t is None else t.cuda()            # noqa: E731
    d = dict(xb=dev(xb), wb=dev(wb), bias=dev(None if bias is None else bias.to(F32)), out=dev(out), pre=dev(pre), dsrc=dev(dsrc),
             res=dev(res), xs=dev(xs))
    dr = None
    if drop is not None:
        p, dseed, counter = drop
        dr = (p, dseed, None if counter is None else torch.tensor([counter], dtype=torch.int64, device="cuda"))
    K.gemm(d["xb"], d["wb"], M, N, Kd, bias=d["bias"], out=d["out"], ldx=ldx, ldw=ldw, ldo=ldo, x_kstrided=xk, w_kstrided=wk, act=act,
           out_mode=out_mode, split_k=split_k, alpha=alpha, preact=d["pre"], dact_src=d["dsrc"], residual=d["res"], tile_hint=hint,
           xsum=d["xs"], fixup=fixup, drop=dr)
    torch.cuda.synchronize()
    got = {k: None if v is None else v.cpu() for k, v in d.items()}
    what = f"{layout} hint {hint} {M}x{N}x{Kd}"
    canary_ok(what + " out", got["out"], M, N)
    r = {"out": got["out"][:M, :N]}
    if pre is not None:
        canary_ok(what + " preact", got["pre"], M, N)
        r["preact"] = got["pre"][:M, :N]
    if xs is not None:
        canary_ok(what + " xsum", got["xs"], M, 0)
        r["xsum"] = got["xs"][:M]
    for name, src in (("xb", xb), ("wb", wb), ("dsrc", dsrc), ("res", res)):
        assert src is None or torch.equal(got[name], src), f"{what}: read-only operand {name} changed"
    if fixup:
        for _, cnt in K._FIX.values():
            assert int(cnt.count_nonzero()) == 0, f"{what}: arrival counters not zero after the launch"
    return r


# ===================================================================================== unmarked: the plan
def test_plan_row_split_shapes():
    """the shapes of the row-split tests really split: m_main = 4096 on 256-row tiles (8-phase loop in the forward layout,
    ping-pong with a K-strided operand), a 32-row tail on the 64-row tiles — and never with fused dropout."""
    M, N, K_ = SPLIT_SHAPE
    for kw, main_hint in ((dict(), 258), (dict(bias=True, act="quick_gelu", preact=True, residual=True), 258),
                          (dict(act="gelu", dact_src=True), 258), (dict(w_kstrided=True, act="gelu", dact_src=True), 256),
                          (dict(x_kstrided=True, out_mode=1), 256),
                          (dict(x_kstrided=True, w_kstrided=True, out_mode=2, xsum=True), 256)):
        p = plan(M=M, N=N, K=K_, **kw)
        assert [l["rows"] for l in p] == [SPLIT_MAIN, M - SPLIT_MAIN] and [l["tile_hint"] for l in p] == [main_hint, 64], (kw, p)
    p = plan(M=M, N=N, K=2048, split_k=2, fixup=True, out_mode=1)              # fix-up split-K across the row split
    assert [(l["rows"], l["tile_hint"], l["k_slices"], l["fixup"]) for l in p] == [(SPLIT_MAIN, 258, 2, True), (32, 64, 2, True)], p
    p = plan(M=8224, N=2048, K=512, bias=True, act="quick_gelu", preact=True, residual=True)     # test_gemm_row_split_dispatch
    assert [(l["rows"], l["tile_hint"]) for l in p] == [(8192, 258), (32, 64)], p
    assert len(plan(M=8224, N=1024, K=128)) == 1, "the shape that test used before does not split"
    for kw in (dict(act="gelu"), dict(act="gelu", preact=True), dict(w_kstrided=True, act="gelu", dact_src=True)):
        p = plan(M=M, N=N, K=K_, drop_p=0.1, **kw)
        assert len(p) == 1 and p[0]["rows"] == M and p[0]["tile_hint"] == 256, ("fused dropout must not split rows", kw, p)


def test_plan_8phase_and_loops():
    for M, N, K_ in ((4096, 4096, 512), (16384, 4096, 1024), SPLIT_SHAPE):
        assert plan(M=M, N=N, K=K_)[0]["tile_hint"] == 258
        assert plan(M=M, N=N, K=K_, w_kstrided=True)[0]["tile_hint"] == 256
        assert plan(M=M, N=N, K=K_, x_kstrided=True)[0]["tile_hint"] == 256
        assert plan(M=M, N=N, K=K_, act="gelu", drop_p=0.1)[0]["tile_hint"] == 256
    for hint in HINTS:                                            # a forced hint is the kernel that runs
        for lay in layouts_of(hint):
            p = plan(M=304, N=304, K=72, tile_hint=hint, x_kstrided=lay[0] == "T", w_kstrided=lay[1] == "T")
            assert len(p) == 1 and p[0]["tile_hint"] == hint
    with pytest.raises(Exception, match="8-phase loop"):
        plan(M=304, N=304, K=72, tile_hint=258, w_kstrided=True)
    # fused dropout has 256 x 256, 256 x 128 and 64 x 128 instances only: 128 runs the 64-row tiles
    assert [plan(M=300, N=512, K=72, tile_hint=h, act="gelu", drop_p=0.1)[0]["tile_hint"] for h in (64, 128, 256, 264)] == [64, 64, 256, 264]


def test_plan_skinny_conditions():
    assert plan(M=8, N=1001, K=512)[0] == dict(rows=8, tile_hint=8, k_slices=1, fixup=False, epilogue="skinny")
    assert plan(M=1, N=4, K=8, bias=True, act="gelu", out_mode=1)[0]["tile_hint"] == 8
    for kw in (dict(M=9, N=64, K=512), dict(M=8, N=64, K=100, ldx=104, ldw=104), dict(M=8, N=64, K=512, residual=True),
               dict(M=8, N=64, K=512, preact=True), dict(M=8, N=64, K=512, act="gelu", dact_src=True),
               dict(M=8, N=64, K=512, split_k=2, out_mode=2), dict(M=8, N=64, K=512, w_kstrided=True)):
        assert plan(**kw)[0]["tile_hint"] != 8, kw
    for kw in (dict(M=9, N=64, K=512), dict(M=8, N=64, K=100, ldx=104, ldw=104), dict(M=8, N=64, K=512, residual=True),
               dict(M=8, N=64, K=512, split_k=2, out_mode=2)):
        with pytest.raises(Exception, match="skinny kernel needs"):
            plan(tile_hint=8, **kw)
    assert plan(M=8, N=64, K=32, split_k=2, out_mode=2, tile_hint=8)[0]["tile_hint"] == 8      # one 64-wide slice: no split


def test_plan_epilogue_families():
    sh = dict(M=260, N=264, K=72)
    for hint in HINTS:
        big = TILE[hint][0] == 256
        fam = lambda **kw: plan(**{**sh, "tile_hint": hint, **kw})[0]["epilogue"]                  # noqa: E731
        assert fam() == fam(bias=True, act="gelu") == ("bf16_transposed" if big else "direct")
        for one in ("preact", "residual", "dact_src"):
            assert fam(**{one: True}) == ("bf16_transposed" if big else "f32_staged"), (hint, one)
        for two in (("preact", "residual"), ("dact_src", "residual"), ("preact", "dact_src"), ("preact", "dact_src", "residual")):
            assert fam(**{k: True for k in two}) == "f32_staged", (hint, two)
        assert fam(out_mode=1) == fam(out_mode=2) == "f32_staged"
        assert fam(ldo=268) == ("f32_staged" if big else "direct") and fam(ldo=266) == "f32_staged"
        assert plan(tile_hint=hint, M=260, N=261, K=72, ldo=264)[0]["epilogue"] == ("f32_staged" if big else "direct")
        if hint != 258:
            assert fam(out_mode=2, split_k=2, K=128) == "atomic" and fam(out_mode=2, split_k=2, K=128, fixup=True) == "f32_staged"
        assert fam(out_mode=2, split_k=2, K=64) == "f32_staged"                                   # one slice: the plain path
    assert plan(M=300, N=512, K=72, tile_hint=256, act="gelu", drop_p=0.1)[0]["epilogue"] == "f32_staged"
    assert plan(M=300, N=512, K=72, tile_hint=256, act="gelu", preact=True, drop_p=0.1)[0]["epilogue"] == "bf16_transposed"


def test_plan_k_slices():
    for K_, split, z in ((128, 2, 2), (128, 3, 2), (128, 8, 2), (200, 2, 2), (200, 3, 2), (200, 8, 4), (520, 2, 2), (520, 3, 3),
                         (520, 8, 5), (64, 2, 1), (72, 8, 2)):
        for fix in (False, True):
            p = plan(M=260, N=264, K=K_, split_k=split, out_mode=2, fixup=fix, tile_hint=128)[0]
            assert p["k_slices"] == z and p["fixup"] == (fix and z > 1), (K_, split, fix, p)


def test_plan_every_tuned_key():
    tuned = json.load(open(os.path.join(ROOT, "vacnic_amd", "gemm_tuned.json")))
    assert len(tuned) >= 10
    for key, t in tuned.items():
        xk, wk, M, N, K_, om, pre = (int(v) for v in key.split(","))
        fix = len(t) > 4 and bool(t[4])
        p = plan(M=M, N=N, K=K_, x_kstrided=bool(xk), w_kstrided=bool(wk), ldx=round8(M if xk else K_), ldw=round8(N if wk else K_), out_mode=om, preact=bool(pre), tile_hint=t[0] or -1,
                 split_k=t[1] if (fix or om == 2) else 1, fixup=fix, xsum=bool(xk and wk))
        assert p[0]["tile_hint"] == (t[0] or p[0]["tile_hint"]), (key, t, p)


def test_refusals_decided_on_the_host():
    """gap 3: K slices that meet in atomics carry alpha and bias only.  gap 8: out / preact / dact_src / residual must be aligned
    wherever the epilogues access rows in 16-byte (8-byte) pieces; a stride that rules those out takes the element-wise path."""
    sh = dict(M=260, N=264, K=128)
    for kw in (dict(act="gelu"), dict(preact=True), dict(act="gelu", dact_src=True), dict(residual=True)):
        with pytest.raises(Exception, match="atomics carries alpha and bias only"):
            plan(split_k=2, out_mode=2, tile_hint=128, **sh, **kw)
        assert plan(split_k=2, out_mode=2, tile_hint=128, fixup=True, **sh, **kw)[0]["fixup"]
    assert plan(split_k=2, out_mode=2, tile_hint=128, bias=True, alpha=0.5, **sh)[0]["epilogue"] == "atomic"
    base = 1 << 20
    for hint in HINTS:
        for name in ("out", "preact", "dact_src", "residual"):
            extra = {} if name == "out" else {name: True}
            for off in (2, 8):
                with pytest.raises(ValueError, match="aligned"):
                    plan(tile_hint=hint, ptrs={name: base + off}, **sh, **extra)
            # rows that are not 16-byte multiples are accessed element by element: any (element-aligned) base will do
            assert plan(tile_hint=hint, ldo=266, ptrs={name: base + 2}, **sh, **extra)
        with pytest.raises(ValueError, match="8-byte aligned"):
            plan(tile_hint=hint, ldo=268, ptrs={"out": base + 4}, **sh)
        assert plan(tile_hint=hint, ldo=268, ptrs={"out": base + 8}, **sh)
        for off in (4, 8):
            with pytest.raises(ValueError, match="fp32 out"):
                plan(tile_hint=hint, out_mode=1, ptrs={"out": base + off}, **sh)
        assert plan(tile_hint=hint, out_mode=1, ldo=266, ptrs={"out": base + 4}, **sh)
    assert plan(M=8, N=1001, K=512, ptrs={"out": base + 2})[0]["tile_hint"] == 8        # the skinny kernel stores single elements


# ================================================================================== unmarked: the mutants
def _epi_case(seed=0, M=260, N=264, K_=72):
    X, W = ints((M, K_), -2, 2, seed + 1), ints((N, K_), -1, 1, seed + 2)
    return X, W, ints((N,), -8, 8, seed + 3), ints((M, N), -100, 100, seed + 4)


def test_mutants_exact_regime():
    """every wrong variant differs from the reference in at least one element (an exact check then fails)"""
    X, W, bias, res = _epi_case()
    ref = gemm_ref(X, W, 0.5, bias)
    assert_exact_regime(X, W, 0.5, bias, res)
    assert not torch.equal(ref, mut_last_k_dropped(X, W, 0.5, bias))
    assert not torch.equal(ref, mut_bias_scaled(X, W, 0.5, bias))
    assert not torch.equal(rne(ref), rne(mut_last_k_dropped(X, W, 0.5, bias))) and not torch.equal(rne(ref), rne(mut_bias_scaled(X, W, 0.5, bias)))
    for K_ in (100, 996):                                               # K % 8 != 0: the pad columns the tests fill with garbage
        Xk, Wk = ints((64, K_), -4, 4, 5), ints((128, K_), -4, 4, 6)
        xp, wp = garbage((64, round8(K_) - K_), 1), garbage((128, round8(K_) - K_), 2)
        assert not torch.equal(gemm_ref(Xk, Wk), mut_pad_column_included(Xk, Wk, xp, wp))
        assert torch.equal(gemm_ref(Xk, Wk), mut_pad_column_included(Xk, Wk, xp * 0, wp)), "zero on one side is enough"
    for K_, split in ((128, 2), (200, 3), (520, 8)):
        kps = (-(-K_ // split) + 63) // 64 * 64
        Xk, Wk = ints((64, K_), -4, 4, 7), ints((128, K_), -4, 4, 8)
        assert not torch.equal(gemm_ref(Xk, Wk, 0.5, bias[:128]), mut_slice1_twice(Xk, Wk, kps, 0.5, bias[:128]))
    # K-strided operands, M % 8 != 0: the pad columns of dY must reach neither out nor xsum
    M, Mp = 67, 72
    dY = ints((M, 40), -4, 4, 9)
    padded = torch.cat([dY, garbage((Mp - M, 40), 3)], 0)
    xs, xs_mut = torch.full((M + 8,), CANARY, dtype=F64), torch.full((M + 8,), CANARY, dtype=F64)
    xs[:M] = dY.sum(1)
    xs_mut[:Mp] = padded.sum(1)                                         # xsum over round_up(M, 8) rows
    assert not torch.equal(xs, xs_mut) and bool((xs_mut[M:Mp] != CANARY).all())
    # the activation-dropout mask with the row index restarted at the tail launch
    Ms, Ns, _ = SPLIT_SHAPE
    thr = drop_threshold(0.1)
    keep = keep_mask(Ms, 256, 777, 5, thr)
    mut = mut_mask_restarted(keep, SPLIT_MAIN)
    assert torch.equal(mut[:SPLIT_MAIN], keep[:SPLIT_MAIN]) and not torch.equal(mut[SPLIT_MAIN:], keep[SPLIT_MAIN:])
    assert (mut[SPLIT_MAIN:] != keep[SPLIT_MAIN:]).float().mean().item() > 0.1


def _act_case(seed=0, M=260, N=264, K_=72):
    X, W = ints((M, K_), -2, 2, seed + 1), ints((N, K_), -2, 2, seed + 2)
    bias = ints((N,), -8, 8, seed + 3) * 0.125
    u = gemm_ref(X, W, 0.125, bias)
    assert u.abs().max().item() <= 32, "pre-activations must be bf16-exact multiples of 1/8"
    return X, W, bias, u


@pytest.mark.parametrize("act", ACTS)
def test_mutants_activation_bounds(act):
    """for the tolerance checks a wrong variant lies at least 10x the bound away in some element"""
    X, W, bias, u = _act_case()
    ref = act_true(act, u)
    bound, _ = act_bound(act, u, ref)
    for name, mu in (("last k dropped", mut_last_k_dropped(X, W, 0.125, bias)), ("bias scaled by alpha", mut_bias_scaled(X, W, 0.125, bias)),
                     ("slice 1 twice", u + 0.125 * (X[:, 64:] @ W[:, 64:].t()))):
        ratio = torch.nan_to_num((act_true(act, mu) - ref).abs() / bound).max().item()
        assert ratio >= 10, f"{act} {name}: only {ratio:.2f}x the bound away"
    g = gemm_ref(ints((260, 40), -2, 2, 11), ints((264, 40), -2, 2, 12), 0.125)
    refb = g * act_true(act, u, deriv=True)
    boundb, _ = act_bound(act, u, refb, scale=g, deriv=True)
    gm = mut_last_k_dropped(ints((260, 40), -2, 2, 11), ints((264, 40), -2, 2, 12), 0.125)
    assert torch.nan_to_num((gm * act_true(act, u, deriv=True) - refb).abs() / boundb).max().item() >= 10
    assert torch.nan_to_num((g * act_true(act, u + 0.125, deriv=True) - refb).abs() / boundb).max().item() >= 10, "act' of a neighbouring element"


@pytest.mark.parametrize("act", ACTS)
def test_bounds_are_not_looser_than_the_older_checks(act):
    _, _, _, u = _act_case()
    ref = act_true(act, u)
    bound, inside = act_bound(act, u, ref)
    assert inside and bool((bound <= EXIST_FWD[0] * ref.abs() + EXIST_FWD[1]).all())
    res = ints(u.shape, -100, 100, 4)
    bound, _ = act_bound(act, u, ref + res, extra_round=ref)
    assert bool((bound <= EXIST_RES[0] * (ref + res).abs() + EXIST_RES[1]).all())
    # two correct roundings (half an ulp each) and the allowance stay inside that older check, so the cap rejects no correct kernel
    allow, measured = act_allow(act, u)
    assert bool((2.0 ** -9 * (1 + 2.0 ** -8) * (ref.abs() + (ref + res).abs()) + allow + measured <= EXIST_RES[0] * (ref + res).abs() + EXIST_RES[1]).all())
    g = gemm_ref(ints((260, 40), -2, 2, 11), ints((264, 40), -2, 2, 12), 0.125)
    refb = g * act_true(act, u, deriv=True)
    bound, inside = act_bound(act, u, refb, scale=g, deriv=True)
    assert inside and bool((bound <= EXIST_BWD[0] * refb.abs() + EXIST_BWD[1]).all())
    # the formulas of common.h themselves stay inside their allowance in float64 (formula term) and fp32 (measured term)
    allow, measured = act_allow(act, u)
    assert bool(((act_formula(act, u, np.float64) - ref).abs() <= allow).all())
    assert bool(((act_formula(act, u, np.float32) - ref).abs() <= allow + measured).all())
    allow, measured = act_allow(act, u, deriv=True)
    assert bool(((act_formula(act, u, np.float64, True) - act_true(act, u, True)).abs() <= allow).all())


# ======================================================================================== GPU: K schedule
@gpu
@pytest.mark.parametrize("hint", HINTS)
def test_k_schedule_per_loop(K, hint):
    """one tile, K at every prologue / drain edge of the loop: 1 to 5+ stages of the 32-wide 4-slot ring, 1 to 3 tiles of the
    64-wide loops, odd and even tile counts of the 8-phase loop; K % 8 != 0 with zero padding on one side, garbage on the other."""
    BM, BN = TILE[hint]
    for lay in layouts_of(hint):
        for K_ in (8, 24, 32, 64, 72, 96, 128, 160, 192, 200, 320):
            X, W = ints((BM, K_), -4, 4, K_), ints((BN, K_), -4, 4, K_ + 1)
            assert_exact_regime(X, W)
            r = run_gemm(K, X, W, lay, hint, out_mode=1, seed=K_)
            chk_equal(f"kloop {lay} hint {hint} K={K_}", r["out"], gemm_ref(X, W))
        for K_ in (100, 996):
            X, W = ints((BM, K_), -4, 4, K_), ints((BN, K_), -4, 4, K_ + 1)
            for kpad in (("zero", "garbage"), ("garbage", "zero")) if lay == "NN" else (("garbage", "garbage"),):
                # a K-strided operand has no K padding: its rows past K are out of range and read as zero
                r = run_gemm(K, X, W, lay, hint, out_mode=1, kpad=kpad, seed=K_)
                chk_equal(f"kloop {lay} hint {hint} K={K_} pad x={kpad[0]} w={kpad[1]}", r["out"], gemm_ref(X, W))


# ========================================================================================= GPU: tile edges
@gpu
@pytest.mark.parametrize("hint", HINTS)
def test_tile_edges(K, hint):
    """partial tiles in both directions, tile counts 1, 2, 3, 6, 7 and 9 (XCD remap with nt < 8 and nt % 8 != 0), odd N and ldo
    (element-wise stores), K-strided operands whose pad columns hold garbage"""
    BM, BN = TILE[hint]
    K_ = 72
    cases = [(M, N) for M in (BM - 1, BM, BM + 1, 2 * BM + 5) for N in (BN - 1, BN, BN + 1, BN + 8, 2 * BN + 12)] + [(6 * BM + 5, BN)]
    for M, N in cases:
        X, W, bias = ints((M, K_), -4, 4, M), ints((N, K_), -4, 4, N), ints((N,), -8, 8, 3)
        ref = gemm_ref(X, W, 1.0, bias)
        chk_equal(f"edges NN hint {hint} f32", run_gemm(K, X, W, "NN", hint, bias=bias, out_mode=1)["out"], ref)
        if N % 2 == 0 or M == BM + 1:
            chk_equal(f"edges NN hint {hint} bf16", run_gemm(K, X, W, "NN", hint, bias=bias)["out"], rne(ref))
    if hint == 258:
        return
    for M, N in ((BM + 3, BN + 5), (BM - 1, 2 * BN + 12), (2 * BM + 5, BN - 3)):
        X, W = ints((M, K_), -4, 4, M), ints((N, K_), -4, 4, N)
        ref = gemm_ref(X, W)
        acc0, xs0 = ints((M, N), -50, 50, 5), ints((M,), -50, 50, 6)
        chk_equal(f"edges NT hint {hint}", run_gemm(K, X, W, "NT", hint)["out"], rne(ref))
        chk_equal(f"edges TN hint {hint}", run_gemm(K, X, W, "TN", hint, out_mode=1, ld_extra=(8, 0))["out"], ref)
        r = run_gemm(K, X, W, "TT", hint, out_mode=2, acc0=acc0, xsum0=xs0, ld_extra=(0, 16))
        chk_equal(f"edges TT hint {hint}", r["out"], acc0 + ref)
        chk_equal(f"edges TT hint {hint} xsum", r["xsum"], xs0 + X.sum(1))


# =========================================================================================== GPU: epilogues
EXACT_EPI = [
    dict(), dict(bias=1), dict(bias=1, alpha=0.5), dict(bias=1, alpha=0.5, out_mode=1), dict(bias=1, alpha=0.5, out_mode=2),
    dict(bias=1, ldo_extra=8), dict(bias=1, ldo_extra=4), dict(bias=1, ldo_extra=2), dict(bias=1, out_mode=1, ldo_extra=8),
    dict(bias=1, out_mode=2, ldo_extra=2),
    dict(bias=1, preact=1), dict(bias=1, residual=1), dict(bias=1, dact=1), dict(bias=1, alpha=0.5, residual=1, ldo_extra=8),
    dict(bias=1, preact=1, residual=1), dict(bias=1, dact=1, residual=1), dict(bias=1, preact=1, dact=1, residual=1),
    dict(bias=1, preact=1, residual=1, out_mode=1), dict(bias=1, residual=1, out_mode=2), dict(bias=1, preact=1, ldo_extra=2),
]


@gpu
@pytest.mark.parametrize("hint", HINTS)
def test_epilogues_exact(K, hint):
    """every epilogue family on 260 x 264 x 72 (a partial tile in both directions) and on N = 261 (ragged rows: bf16 output falls
    off the transposed epilogue, fp32 output with ldo % 4 != 0 takes the element-wise stores).  Pre-activations are integers (or
    halves) of magnitude <= 256, so the epilogues that round to bf16 before adding the residual agree with those that do not."""
    for N in (264, 261):
        X, W, bias, res = _epi_case(N=N)
        M = X.shape[0]
        dsrc = ints((M, N), -3, 3, 9)                           # with act = none, act'(.) = 1 whatever the source holds
        acc0 = ints((M, N), -1000, 1000, 10)
        for i, c in enumerate(EXACT_EPI):
            alpha, om = c.get("alpha", 1.0), c.get("out_mode", 0)
            if N == 261 and c.get("ldo_extra", 0) == 8:
                c = dict(c, ldo_extra=3)                        # N = 261: ldo 264 (16-byte rows, ragged last chunk)
            b = bias if c.get("bias") else None
            u = gemm_ref(X, W, alpha, b)
            assert_exact_regime(X, W, alpha, b, res, acc0)
            assert u.abs().max().item() <= 256, "pre-activation must be exact in bf16"
            v = u + (res if c.get("residual") else 0) + (acc0 if om == 2 else 0)
            r = run_gemm(K, X, W, "NN", hint, bias=b, alpha=alpha, want_preact=bool(c.get("preact")), dact=dsrc if c.get("dact") else None,
                         residual=res if c.get("residual") else None, out_mode=om, acc0=acc0, ldo_extra=c.get("ldo_extra", 0), seed=i)
            what = f"epi hint {hint} N={N} " + ",".join(f"{k}={v_}" for k, v_ in c.items())
            chk_equal(what + " out", r["out"], rne(v) if om == 0 else v)
            if c.get("preact"):
                chk_equal(what + " preact", r["preact"], u)


@gpu
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("hint", HINTS)
def test_epilogues_activation(K, hint, act):
    """activation and activation-backward epilogues: pre-activations are exact multiples of 1/8, bound = 2^-8 |ref| + allowance"""
    X, W, bias, u = _act_case()
    M, N = u.shape
    ref = act_true(act, u)
    res = ints((M, N), -100, 100, 4)
    for c in (dict(), dict(preact=1), dict(ldo_extra=8), dict(out_mode=1), dict(residual=1), dict(preact=1, residual=1)):
        om = c.get("out_mode", 0)
        r = run_gemm(K, X, W, "NN", hint, bias=bias, alpha=0.125, act=act, want_preact=bool(c.get("preact")),
                     residual=res if c.get("residual") else None, out_mode=om, ldo_extra=c.get("ldo_extra", 0))
        want = ref + (res if c.get("residual") else 0)
        bound, _ = act_bound(act, u, want, extra_round=ref if c.get("residual") else None)
        if om == 1:
            bound = bound - 2.0 ** -8 * want.abs() + 2.0 ** -22 * want.abs()          # fp32 output: no bf16 rounding
        what = f"act {act} hint {hint} " + ",".join(f"{k}={v}" for k, v in c.items())
        chk_bound(what + " out", r["out"], want, bound)
        if c.get("preact"):
            chk_equal(what + " preact", r["preact"], u)
    # backward: out = (alpha dY W) * act'(dact_src) in the dgrad layout; g is a multiple of 1/8 of magnitude <= 32
    dY, W2 = ints((M, 40), -2, 2, 11), ints((N, 40), -2, 2, 12)
    g = gemm_ref(dY, W2, 0.125)
    assert g.abs().max().item() <= 32
    refb = g * act_true(act, u, deriv=True)
    bound, _ = act_bound(act, u, refb, scale=g, deriv=True)
    for lay in ("NT",) if hint != 258 else ("NN",):
        for c in (dict(), dict(residual=1)):
            r = run_gemm(K, dY, W2, lay, hint, alpha=0.125, act=act, dact=u, residual=res if c.get("residual") else None)
            want = refb + (res if c.get("residual") else 0)
            b2 = bound + (2.0 ** -8 * (want.abs() + refb.abs()) if c.get("residual") else 0)
            chk_bound(f"act' {act} {lay} hint {hint} {c}", r["out"], want, b2)


# ============================================================================================= GPU: split-K
@gpu
@pytest.mark.parametrize("hint", HINTS)
def test_split_k(K, hint):
    """atomic and ordered fix-up split-K: exact, hence independent of the arrival order; bias once, alpha on every slice; a
    request above ceil(K / 64) and a single slice with a workspace; xsum beside both; two launches bitwise equal"""
    M, N = 260, 264
    bias = ints((N,), -8, 8, 3)
    for lay in layouts_of(hint):
        for K_, splits in ((64, (2,)), (128, (2, 3, 8)), (200, (2, 3, 8)), (520, (2, 3, 8))):
            X, W = ints((M, K_), -2, 2, K_), ints((N, K_), -1, 1, K_ + 1)
            acc0, xs0 = ints((M, N), -1000, 1000, 10), ints((M,), -50, 50, 6)
            u = gemm_ref(X, W, 0.5, bias)
            assert_exact_regime(X, W, 0.5, bias, None, acc0)
            xs = xs0 if lay == "TT" else None
            for split in splits:
                for fix in (False, True):
                    r = run_gemm(K, X, W, lay, hint, bias=bias, alpha=0.5, out_mode=2, acc0=acc0, split_k=split, fixup=fix, xsum0=xs)
                    what = f"split {lay} hint {hint} K={K_} split={split} {'fixup' if fix else 'atomic'}"
                    chk_equal(what, r["out"], acc0 + u)
                    if xs is not None:
                        chk_equal(what + " xsum", r["xsum"], xs0 + X.sum(1))
                    r2 = run_gemm(K, X, W, lay, hint, bias=bias, alpha=0.5, out_mode=2, acc0=acc0, split_k=split, fixup=fix, xsum0=xs)
                    assert torch.equal(r["out"], r2["out"]), what + ": two launches differ"
    # the fix-up runs the whole epilogue once: bf16 output, residual, saved pre-activation, activation
    lay = "NN"
    Xa, Wa, ba, ua = _act_case(K_=200)
    res = ints((M, N), -100, 100, 4)
    for split in (2, 3, 8):
        X, W = ints((M, 200), -2, 2, 1), ints((N, 200), -1, 1, 2)
        u = gemm_ref(X, W, 0.5, bias)
        assert u.abs().max().item() <= 256
        r = run_gemm(K, X, W, lay, hint, bias=bias, alpha=0.5, residual=res, want_preact=True, split_k=split, fixup=True)
        chk_equal(f"fixup hint {hint} split={split} bf16 + residual", r["out"], rne(u + res))
        chk_equal(f"fixup hint {hint} split={split} preact", r["preact"], u)
        r = run_gemm(K, Xa, Wa, lay, hint, bias=ba, alpha=0.125, act="gelu", split_k=split, fixup=True)
        ref = act_true("gelu", ua)
        chk_bound(f"fixup hint {hint} split={split} gelu", r["out"], ref, act_bound("gelu", ua, ref)[0])


@gpu
def test_atomic_split_refuses_epilogue_operands(K):
    """gap 3: the atomics branch would drop act / preact / dact_src / residual silently; it is refused on the host instead"""
    from vacnic_amd._lib import VacnicError
    X, W = ints((64, 128), -2, 2, 1), ints((128, 128), -1, 1, 2)
    z = torch.zeros(64, 128, dtype=F64)
    for kw in (dict(act="gelu"), dict(want_preact=True), dict(act="gelu", dact=z), dict(residual=z)):
        with pytest.raises(VacnicError, match="atomics carries alpha and bias only"):
            run_gemm(K, X, W, "NN", 64, out_mode=2, acc0=z, split_k=2, **kw)


# ============================================================================================ GPU: row split
def _split_rows():
    M = SPLIT_SHAPE[0]
    rows = list(range(0, 8)) + list(range(SPLIT_MAIN - 16, M)) + list(range(8, SPLIT_MAIN - 16, 389))
    return torch.tensor(sorted(set(rows)))


@gpu
def test_row_split_operands(K):
    """the cost model cuts rows [4096, 4128) off into a launch of its own: every row-indexed operand (out, preact, residual,
    dact_src, K-strided X, xsum) must be offset consistently.  References for a band on both sides of m_main, the first and
    last rows and a strided sample."""
    M, N, K_ = SPLIT_SHAPE
    sel = _split_rows()
    X, W = ints((M, K_), -1, 1, 1), ints((N, K_), -1, 1, 2)
    bias, res = ints((N,), -8, 8, 3), ints((M, N), -100, 100, 4)
    u = gemm_ref(X[sel], W, 1.0, bias)
    assert_exact_regime(X[sel], W, 1.0, bias, res)
    assert u.abs().max().item() <= 256
    r = run_gemm(K, X, W, "NN", -1, bias=bias, want_preact=True, residual=res)
    chk_equal("rowsplit NN preact", r["preact"][sel], u)
    chk_equal("rowsplit NN out + residual", r["out"][sel], rne(u + res[sel]))
    # activation + saved pre-activation + residual (the ViT block), then the dgrad that reads it back
    ua = gemm_ref(X[sel], W, 0.125, bias * 0.125)
    r = run_gemm(K, X, W, "NN", -1, bias=bias * 0.125, alpha=0.125, act="quick_gelu", want_preact=True, residual=res)
    ref = act_true("quick_gelu", ua)
    chk_equal("rowsplit NN act preact", r["preact"][sel], ua)
    chk_bound("rowsplit NN act out", r["out"][sel], ref + res[sel], act_bound("quick_gelu", ua, ref + res[sel], extra_round=ref)[0])
    dsrc = ints((M, N), -24, 24, 7) * 0.125
    g = gemm_ref(X[sel], W, 0.125)
    assert g.abs().max().item() <= 32
    refb = g * act_true("gelu", dsrc[sel], deriv=True)
    for lay in ("NN", "NT"):
        r = run_gemm(K, X, W, lay, -1, alpha=0.125, act="gelu", dact=dsrc)
        chk_bound(f"rowsplit {lay} dact", r["out"][sel], refb, act_bound("gelu", dsrc[sel], refb, scale=g, deriv=True)[0])
    r = run_gemm(K, X, W, "TN", -1, out_mode=1)
    chk_equal("rowsplit TN f32", r["out"][sel], gemm_ref(X[sel], W))
    acc0, xs0 = ints((M, N), -1000, 1000, 10), ints((M,), -50, 50, 6)
    r = run_gemm(K, X, W, "TT", -1, out_mode=2, acc0=acc0, xsum0=xs0)
    chk_equal("rowsplit TT acc", r["out"][sel], acc0[sel] + gemm_ref(X[sel], W))
    chk_equal("rowsplit TT xsum", r["xsum"], xs0 + X.sum(1))
    X2, W2 = ints((M, 2048), -1, 1, 11), ints((N, 2048), -1, 1, 12)      # K = 2048: the longest reduction at which split 2 still cuts the rows
    r = run_gemm(K, X2, W2, "NN", -1, bias=bias, out_mode=1, split_k=2, fixup=True)
    chk_equal("rowsplit NN fixup split 2", r["out"][sel], gemm_ref(X2[sel], W2, 1.0, bias))


# =========================================================================================== GPU: dropout
def _drop_check(what, got, u, keep, thr):
    """dropped positions are exact zeros; kept ones are RNE_bf16(fl32(u * 256 / (256 - thr))) (u exact in bf16 and non-zero)"""
    want = torch.where(keep, (u.to(F32) * np.float32(inv_keep_of(thr))).to(BF16).to(F64), torch.zeros_like(u))
    assert bool((u != 0).all())
    chk_equal(what + " mask", got.to(F64) == 0, ~keep)
    chk_equal(what + " values", got, want)


@gpu
@pytest.mark.parametrize("hint", [64, 128, 256, 264])
def test_fused_dropout_masks_and_values(K, hint):
    """the zeros of the output are exactly the host mask flat_keep(M * N, mix_seed(seed, counter), thr) of the contiguous [M, N]
    array; kept values are the reference times 256 / (256 - thr).  One tile plus a ragged edge; forward with and without a saved
    pre-activation, dgrad with dact_src.  act = none makes the values exact (act' = 1)."""
    BM, BN = TILE[hint]
    M, N, K_ = BM + 5, BN + 16, 72
    p, seed, counter = 0.1, 777, 5
    thr = drop_threshold(p)
    keep = keep_mask(M, N, seed, counter, thr)
    X, W = ints((M, K_), -1, 1, 1), ints((N, K_), -1, 1, 2)
    bias = ints((N,), -8, 8, 3) + 0.5                                    # u is a half-integer: never zero
    u = gemm_ref(X, W, 1.0, bias)
    assert u.abs().max().item() < 128 and bool((rne(u) == u).all())
    r = run_gemm(K, X, W, "NN", hint, bias=bias, want_preact=True, drop=(p, seed, counter))
    chk_equal(f"drop hint {hint} preact is not dropped", r["preact"], u)
    _drop_check(f"drop hint {hint} fwd with preact", r["out"], u, keep, thr)
    r = run_gemm(K, X, W, "NN", hint, bias=bias, drop=(p, seed, counter))
    _drop_check(f"drop hint {hint} fwd", r["out"], u, keep, thr)
    r = run_gemm(K, X, W, "NT", hint, bias=bias, dact=u, drop=(p, seed, counter))
    _drop_check(f"drop hint {hint} dgrad", r["out"], u, keep, thr)
    r = run_gemm(K, X, W, "NN", hint, bias=bias, drop=(p, seed ^ mix_seed(0, counter), None))        # no device counter: the seed alone
    _drop_check(f"drop hint {hint} host seed", r["out"], u, keep, thr)
    ua = u * 0.125
    r = run_gemm(K, X, W, "NN", hint, bias=bias * 0.125, alpha=0.125, act="gelu", want_preact=True, drop=(p, seed, counter))
    inv = inv_keep_of(thr)
    ref = act_true("gelu", ua) * keep * inv
    chk_bound(f"drop hint {hint} gelu", r["out"], ref, act_bound("gelu", ua, ref, scale=keep * inv)[0] + 2.0 ** -22 * ref.abs())
    assert bool((r["out"][~keep] == 0).all())


@gpu
def test_fused_dropout_at_the_row_split_shape(K):
    """gap 1: at a shape whose plain launch splits rows, the mask is still the one of the contiguous [M, N] array in the rows of
    the would-be tail, and the forward with a forced hint and the dgrad under the cost model apply the same mask"""
    M, N, K_ = SPLIT_SHAPE
    p, seed, counter = 0.1, 4242, 3
    thr = drop_threshold(p)
    keep = keep_mask(M, N, seed, counter, thr)
    sel = _split_rows()
    X, W = ints((M, K_), -1, 1, 1), ints((N, K_), -1, 1, 2)
    bias = ints((N,), -8, 8, 3) + 0.5
    u = gemm_ref(X[sel], W, 1.0, bias)
    assert u.abs().max().item() < 128 and bool((rne(u) == u).all())
    fwd = run_gemm(K, X, W, "NN", 256, bias=bias, want_preact=True, drop=(p, seed, counter))
    dgr = run_gemm(K, X, W, "NT", -1, bias=bias, dact=torch.zeros(M, N, dtype=F64), drop=(p, seed, counter))
    cm = run_gemm(K, X, W, "NN", -1, bias=bias, drop=(p, seed, counter))
    for what, r in (("fwd hint 256", fwd), ("dgrad cost model", dgr), ("fwd cost model", cm)):
        chk_equal(f"drop rowsplit {what} mask", r["out"].to(F64) == 0, ~keep)            # u is a half-integer: never zero
        _drop_check(f"drop rowsplit {what} rows", r["out"][sel], u, keep[sel], thr)
    chk_equal("drop rowsplit forward == dgrad", fwd["out"], dgr["out"])


# ============================================================================================ GPU: skinny
@gpu
@pytest.mark.parametrize("K_", [8, 504, 512, 2048, 2056])
def test_skinny(K, K_):
    """the W-streaming kernel (hint 8 and the automatic choice): one and four waves per column group, ragged N, strided X and
    out, every out_mode, exact in the integer regime"""
    i = 0
    for M in (1, 5, 8):
        for N in (1, 4, 1001, 1003):
            X, W, bias = ints((M, K_), -4, 4, M + N), ints((N, K_), -4, 4, N), ints((N,), -8, 8, 3)
            acc0 = ints((M, N), -1000, 1000, 10)
            assert_exact_regime(X, W, 0.5, bias, None, acc0)
            for hint in (8, -1):
                om = i % 3
                i += 1
                assert plan(M=M, N=N, K=K_, ldx=K_ + 8, ldo=N + 3, bias=True, out_mode=om, tile_hint=hint)[0]["tile_hint"] == 8
                r = run_gemm(K, X, W, "NN", hint, bias=bias, alpha=0.5, out_mode=om, acc0=acc0, ldo_extra=3, ld_extra=(8, 16))
                v = gemm_ref(X, W, 0.5, bias) + (acc0 if om == 2 else 0)
                chk_equal(f"skinny M={M} N={N} K={K_} hint {hint} out_mode {om}", r["out"], rne(v) if om == 0 else v)
    X, W = ints((5, K_), -2, 2, 1), ints((1003, K_), -2, 2, 2)
    bias = ints((1003,), -8, 8, 3) * 0.125
    u = gemm_ref(X, W, 2.0 ** -5 if K_ > 512 else 0.125, bias)
    for act in ACTS:
        r = run_gemm(K, X, W, "NN", 8, bias=bias, alpha=2.0 ** -5 if K_ > 512 else 0.125, act=act)
        ref = act_true(act, u)
        chk_bound(f"skinny act {act} K={K_}", r["out"], ref, act_bound(act, u, ref)[0])


@gpu
def test_small_m_off_the_skinny_kernel(K):
    """M <= 8 with K % 8 != 0 or with a residual takes the tile path and is still right"""
    for M in (1, 5, 8):
        X, W, bias = ints((M, 100), -4, 4, M), ints((1003, 100), -4, 4, 2), ints((1003,), -8, 8, 3)
        assert plan(M=M, N=1003, K=100, ldx=104, ldw=104, bias=True, out_mode=1)[0]["tile_hint"] == 64
        chk_equal(f"small M={M} K=100", run_gemm(K, X, W, "NN", -1, bias=bias, out_mode=1)["out"], gemm_ref(X, W, 1.0, bias))
        X, W, res = ints((M, 72), -2, 2, M), ints((1003, 72), -1, 1, 2), ints((M, 1003), -100, 100, 4)
        u = gemm_ref(X, W, 1.0, bias)
        assert plan(M=M, N=1003, K=72, bias=True, residual=True)[0]["tile_hint"] == 64 and u.abs().max().item() <= 256
        chk_equal(f"small M={M} residual", run_gemm(K, X, W, "NN", -1, bias=bias, residual=res)["out"], rne(u + res))


# ============================================================================================ GPU: gemv_ln
def _ln_pipeline(x, res, g, b, w, bias, dt, eps=1e-5):
    """the kernel comment's arithmetic in dtype dt: LayerNorm(x + res), rounded to bf16, dot"""
    h = (x + res).to(dt)
    mean = h.mean(1, keepdim=True)
    var = ((h - mean) ** 2).mean(1, keepdim=True)
    y = (h - mean) / torch.sqrt(var + eps) * g.to(dt) + b.to(dt)
    y16 = y.to(F32).to(BF16).to(dt)
    return y, y16, y16 @ w.to(dt).t() + (0 if bias is None else bias.to(dt))


def _bf16_ulp(v):
    return 2.0 ** (torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -126))) - 7)


@gpu
@pytest.mark.parametrize("M", [1, 8])
@pytest.mark.parametrize("K_", [8, 512, 520, 1024])
def test_gemv_ln(K, K_, M):
    N, ldw, ldo = 1003, K_ + 8, 1008
    gen = torch.Generator(device="cpu").manual_seed(K_ + M)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=gen) * sc                          # noqa: E731
    x, res, w = rn(M, K_).to(BF16), rn(M, K_).to(BF16), rn(N, K_, sc=0.05).to(BF16)
    g, b, bias = rn(K_, sc=0.5) + 1.0, rn(K_, sc=0.1), rn(N)
    wbuf = garbage((N, ldw), 1).to(BF16)
    wbuf[:, :K_] = w
    y64, y16, z64 = _ln_pipeline(x.to(F64), res.to(F64), g, b, w, bias, F64)
    y32, _, z32 = _ln_pipeline(x.to(F32), res.to(F32), g, b, w, bias, F32)
    m_ln = max(8.0 * (y32.to(F64) - y64).abs().max().item(), 1e-6 * y64.abs().max().item())
    # float64 values within the LayerNorm margin of a bf16 rounding boundary may legitimately round the other way
    ulp = _bf16_ulp(y64)
    near = ((y64 - y16).abs() - ulp / 2).abs() <= m_ln
    flip = (near.to(F64) * ulp) @ w.to(F64).abs().t()
    m_dot = max(8.0 * (z32.to(F64) - z64).abs().max().item(), 1e-6 * z64.abs().max().item())
    d = dict(x=x.cuda(), res=res.cuda(), g=g.cuda(), b=b.cuda(), w=wbuf.cuda(), bias=bias.cuda())
    for om, with_ln in ((0, True), (1, True), (1, False)):
        odt = BF16 if om == 0 else F32
        got = torch.full((M + 8, ldo), CANARY, dtype=odt).cuda()
        hn = torch.full((M + 8, K_), CANARY, dtype=BF16).cuda() if with_ln else None
        K.gemv_ln(d["x"], d["res"], d["g"], d["b"], d["w"], M, N, K_, bias=d["bias"], out=got, ln_out=hn, ldw=ldw, ldo=ldo, out_mode=om)
        # reference 1: bit identity with add_ln_fwd + skinny GEMM
        h_ref, _, _ = K.add_ln_fwd(d["x"].view(M, 1, K_), d["res"].view(M, 1, K_), d["g"], d["b"], need_stats=False)
        want = torch.full((M + 8, ldo), CANARY, dtype=odt).cuda()
        K.gemm(h_ref.view(M, K_), d["w"], M, N, K_, bias=d["bias"], out=want, ldw=ldw, ldo=ldo, out_mode=om, tile_hint=8)
        torch.cuda.synchronize()
        what = f"gemv_ln M={M} K={K_} out_mode {om} ln_out={with_ln}"
        chk_equal(what + " vs add_ln + skinny", got.cpu(), want.cpu())
        canary_ok(what, got.cpu(), M, N)
        # reference 2: float64
        bound = m_dot + flip + (2.0 ** -8 * z64.abs() if om == 0 else 0)
        chk_bound(what + " vs float64", got.cpu()[:M, :N], z64, bound)
        if with_ln:
            chk_equal(what + " ln_out vs add_ln", hn.cpu()[:M], h_ref.view(M, K_).cpu())
            canary_ok(what + " ln_out", hn.cpu(), M, K_)
            chk_bound(what + " ln_out vs float64", hn.cpu()[:M], y64, 2.0 ** -8 * y64.abs() + m_ln)
    ua = z64
    got = K.gemv_ln(d["x"], d["res"], d["g"], d["b"], d["w"], M, N, K_, bias=d["bias"], ldw=ldw, act="gelu")
    ref = act_true("gelu", ua)
    allow, measured = act_allow("gelu", ua)
    chk_bound(f"gemv_ln M={M} K={K_} gelu", got.cpu(), ref, 2.0 ** -8 * ref.abs() + allow + measured + 1.2 * (m_dot + flip))   # |gelu'| <= 1.13


@gpu
def test_gemv_ln_refusals(K):
    from vacnic_amd._lib import VacnicError
    t = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device="cuda")                      # noqa: E731
    with pytest.raises(VacnicError, match="K <= 1024"):
        K.gemv_ln(t(4, 1032), t(4, 1032), t(1032, dt=F32), t(1032, dt=F32), t(16, 1032), 4, 16, 1032)
    with pytest.raises(VacnicError, match="M <= 8"):
        K.gemv_ln(t(9, 512), t(9, 512), t(512, dt=F32), t(512, dt=F32), t(16, 512), 9, 16, 512)
    with pytest.raises(ValueError, match="out_mode"):
        K.gemv_ln(t(4, 512), t(4, 512), t(512, dt=F32), t(512, dt=F32), t(16, 512), 4, 16, 512, out=t(4, 16, dt=F32), out_mode=2)


# ========================================================================================= GPU: wgrad_group
@gpu
@pytest.mark.parametrize("M", [8, 72, 200])
def test_wgrad_group_small(K, M):
    """jobs whose N or K crosses 1024 (two units per side), with and without a bias gradient (only the first column block of
    units may add it), strided dy / x, a non-zero initial dW, more than 16 units in one call (the flush at GROUP_MAX_UNITS);
    exact and bitwise repeatable"""
    shapes = [(1032, 1040, True), (1032, 1032, False), (1032, 1032, True), (1032, 1032, True), (1032, 1032, False), (1032, 1032, True),
              (67, 1029, True), (1029, 67, False), (128, 128, True)]
    host, jobs = [], []
    for i, (N, K_, has_b) in enumerate(shapes):
        dy, x = ints((M, N), -4, 4, 10 + i), ints((M, K_), -4, 4, 30 + i)
        dyb, _ = pack(dy, False, 8 * (i % 2), "garbage", i)
        xb, _ = pack(x, False, 16 * (i % 3 == 0), "garbage", i + 50)
        lddw = (K_ + 3) // 4 * 4 + 4
        dw0, db0 = ints((N, K_), -1000, 1000, 50 + i), ints((N,), -1000, 1000, 70 + i)
        dwb = torch.full((N + 8, lddw), CANARY, dtype=F32)
        dwb[:N, :K_] = dw0.to(F32)
        dbb = torch.full((N + 8,), CANARY, dtype=F32)
        dbb[:N] = db0.to(F32)
        host.append((dy, x, dw0, db0, dwb, dbb, has_b))
        d_dy, d_x, d_dw, d_db = dyb.cuda(), xb.cuda(), dwb.cuda(), dbb.cuda()
        jobs.append((d_dy[:, :N], d_x[:, :K_], d_dw[:N, :K_], d_db[:N] if has_b else None, d_dw, d_db))
    runs = []
    for _ in range(2):
        for (dy, x, dw0, db0, dwb, dbb, has_b), j in zip(host, jobs):
            j[4].copy_(dwb)
            j[5].copy_(dbb)
        K.wgrad_group([j[:4] for j in jobs])
        torch.cuda.synchronize()
        runs.append([(j[4].cpu(), j[5].cpu()) for j in jobs])
    for i, ((dy, x, dw0, db0, dwb, dbb, has_b), (gw, gb)) in enumerate(zip(host, runs[0])):
        N, K_ = dw0.shape
        what = f"wgrad_group M={M} job {i} {N}x{K_}"
        chk_equal(what + " dW", gw[:N, :K_], dw0 + dy.t() @ x)
        canary_ok(what + " dW", gw, N, K_)
        chk_equal(what + " dbias", gb[:N], db0 + dy.sum(0) if has_b else db0)
        canary_ok(what + " dbias", gb, N, 0)
        assert torch.equal(gw, runs[1][i][0]) and torch.equal(gb, runs[1][i][1]), what + ": not bitwise repeatable"


# =========================================================================================== GPU: alignment
@gpu
def test_misaligned_epilogue_operands_are_refused_or_routed(K):
    """gap 8: a base address the 16-byte epilogue accesses cannot take is refused before any launch; with a row stride that rules
    those accesses out, the same base goes through the element-wise path and the result is right"""
    M, N, K_ = 70, 136, 72
    X, W, bias = ints((M, K_), -2, 2, 1), ints((N, K_), -1, 1, 2), ints((N,), -8, 8, 3)
    xb, wb, bd = pack(X, False)[0].cuda(), pack(W, False)[0].cuda(), bias.to(F32).cuda()
    res = ints((M, N), -100, 100, 4)
    for hint in (64, 256):
        for off in (1, 4):
            flat = torch.full(((M + 8) * (N + 8) + 8,), CANARY, dtype=BF16).cuda()
            with pytest.raises(ValueError, match="aligned"):
                K.gemm(xb, wb, M, N, K_, bias=bd, out=flat[off:], ldo=N, tile_hint=hint)
            with pytest.raises(ValueError, match="aligned"):
                K.gemm(xb, wb, M, N, K_, bias=bd, out=flat, residual=flat[off:], ldo=N, tile_hint=hint)
            torch.cuda.synchronize()
            assert bool((flat == CANARY).all()), "a refused call must not launch"
        # ldo = N + 1: rows are not 16-byte multiples, every access is element-wise, an odd base is fine
        ldo = N + 1
        flat = torch.full(((M + 8) * ldo + 8,), CANARY, dtype=BF16).cuda()
        rflat = torch.full(((M + 8) * ldo + 8,), CANARY, dtype=BF16)
        rflat[1:1 + M * ldo].view(M, ldo)[:, :N] = res.to(BF16)
        K.gemm(xb, wb, M, N, K_, bias=bd, out=flat[1:], residual=rflat.cuda()[1:], ldo=ldo, tile_hint=hint)
        torch.cuda.synchronize()
        got = flat.cpu()
        body = got[1:1 + (M + 8) * ldo].view(M + 8, ldo)
        chk_equal(f"routed hint {hint} odd base", body[:M, :N], rne(gemm_ref(X, W, 1.0, bias) + res))
        canary_ok(f"routed hint {hint}", body, M, N)
        assert got[0].item() == CANARY
