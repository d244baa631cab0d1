"""The 8-phase counted-wait K loop of the 256 x 256 GEMM tile (tile_hint 258, forward layout) on the MI355X: bitwise against the
same call on the ping-pong loop (tile_hint 256) — both issue the same MFMAs per accumulator in the same k order — and against an
fp32 product of the bf16 inputs with the tolerances tests/test_kernels_gpu.py uses for this tile.  The shapes are the smallest
at which the schedule can go wrong: prologue and drain only, one iteration, an odd K-tile count, zero-filled K, partial tiles."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

NEW, OLD = 258, 256
ACTS = {"gelu": torch.nn.functional.gelu, "tanh": torch.tanh, "quick_gelu": lambda t: t * torch.sigmoid(1.702 * t)}


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


def rnd(*shape, scale=1.0, dtype=torch.bfloat16, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to("cuda").to(dtype)


def close(a, b, rtol, atol, what=""):
    a = a.float(); b = b.float()
    err = (a - b).abs()
    bound = atol + rtol * b.abs()
    bad = (err > bound).sum().item()
    assert bad == 0, f"{what}: {bad}/{a.numel()} off; max err {err.max().item():.4g} (ref max {b.abs().max().item():.4g})"


def same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape
    n = (a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32) != b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)).sum().item()
    assert n == 0, f"{what}: {n}/{a.numel()} elements differ bitwise between the 8-phase and the ping-pong loop"


def forward_case(K, M, N, K_):
    # K_ not a multiple of 8 rides in rows padded to a multiple of 8 (ldx / ldw), as everywhere in the package
    ld = (K_ + 7) // 8 * 8
    xb = torch.zeros(M, ld, device="cuda", dtype=torch.bfloat16); wb = torch.zeros(N, ld, device="cuda", dtype=torch.bfloat16)
    xb[:, :K_] = rnd(M, K_, seed=1); wb[:, :K_] = rnd(N, K_, scale=0.1, seed=2)
    b = rnd(N, dtype=torch.float32, seed=3)
    new = K.gemm(xb, wb, M, N, K_, ldx=ld, ldw=ld, bias=b, tile_hint=NEW)
    old = K.gemm(xb, wb, M, N, K_, ldx=ld, ldw=ld, bias=b, tile_hint=OLD)
    same_bits(new, old, f"{M}x{N}x{K_}")
    close(new, xb.float() @ wb.float().t() + b, 1e-2, 2e-2 * math.sqrt(K_ / 64), f"{M}x{N}x{K_} vs fp32")


@pytest.mark.parametrize("K_", [64, 128, 192, 200, 1024])
def test_k_schedule(K, K_):
    """one K-tile (prologue + drain), one full iteration, an odd tile count, K no multiple of 32 or 64, several iterations"""
    forward_case(K, 256, 256, K_)


@pytest.mark.parametrize("M,N", [(257, 264), (513, 1288)])
def test_partial_tiles(K, M, N):
    """partial tiles in both directions; 3 x 6 = 18 tiles: more than 8, not a multiple of 8 (the XCD tile order)"""
    forward_case(K, M, N, 192)


@pytest.mark.parametrize("act", ["gelu", "tanh", "quick_gelu"])
def test_epilogues(K, act):
    """every epilogue behind the new loop at M = 512, N = 256, K = 128: bias with each activation, residual, saved
    pre-activation, activation-backward source, fp32 output, accumulate — bitwise against the ping-pong loop, and against fp32
    with the tolerances of test_gemm_epilogues_bf16_staged_256_row_tiles."""
    M, N, K_ = 512, 256, 128
    x = rnd(M, K_, seed=1); w = rnd(N, K_, scale=0.1, seed=2); b = rnd(N, dtype=torch.float32, seed=3); res = rnd(M, N, seed=4)
    f = ACTS[act]
    u = x.float() @ w.float().t() + b

    def both(**kw):
        new = K.gemm(x, w, M, N, K_, tile_hint=NEW, **kw)
        old = K.gemm(x, w, M, N, K_, tile_hint=OLD, **kw)
        same_bits(new, old, f"{act} {sorted(kw)}")
        return new

    close(both(bias=b, act=act), f(u), 1e-2, 1e-2, "bias + act")
    close(both(bias=b, act=act, residual=res), f(u) + res.float(), 1e-2, 2e-2, "act + residual")
    pre_new = torch.empty(M, N, device="cuda", dtype=torch.bfloat16); pre_old = torch.empty_like(pre_new)
    o_new = K.gemm(x, w, M, N, K_, bias=b, act=act, preact=pre_new, tile_hint=NEW)
    o_old = K.gemm(x, w, M, N, K_, bias=b, act=act, preact=pre_old, tile_hint=OLD)
    same_bits(o_new, o_old, "saved pre-activation: output"); same_bits(pre_new, pre_old, "saved pre-activation")
    close(pre_new, u, 1e-2, 1e-2, "preact")
    close(o_new, f(pre_new.float()), 1e-2, 1e-2, "act on the saved pre-activation")
    du = both(act=act, dact_src=pre_new)
    uu = pre_new.float().requires_grad_(True)
    f(uu).backward(x.float() @ w.float().t())
    close(du, uu.grad, 2e-2, 2e-2, "activation backward")
    close(both(bias=b, out_mode=1), u, 1e-2, 1e-2, "fp32 output")
    a_new = torch.full((M, N), 2.0, device="cuda"); a_old = a_new.clone()
    K.gemm(x, w, M, N, K_, out=a_new, out_mode=2, tile_hint=NEW)
    K.gemm(x, w, M, N, K_, out=a_old, out_mode=2, tile_hint=OLD)
    same_bits(a_new, a_old, "accumulate")
    close(a_new, 2.0 + u - b, 2e-3, 2e-2 * math.sqrt(K_ / 64), "accumulate vs fp32")


@pytest.mark.parametrize("K_", [64, 192, 1024])
def test_identity_times_asymmetric(K, K_):
    """a mis-placed fragment shows: X = identity padded to [256, K], W asymmetric with distinct rows and columns
    (small integers, exact in bf16) -> out[m][n] = W[n][m] for m < K and 0 below, exactly"""
    M = N = 256
    x = torch.zeros(M, K_, device="cuda", dtype=torch.bfloat16)
    d = min(M, K_)
    x[torch.arange(d), torch.arange(d)] = 1.0
    n = torch.arange(N, device="cuda").view(N, 1); k = torch.arange(K_, device="cuda").view(1, K_)
    w = ((n * 7 + k * 13 + (n * k) % 5) % 251 - 125).to(torch.bfloat16)
    out = K.gemm(x, w, M, N, K_, tile_hint=NEW)
    want = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
    want[:d] = w[:, :d].t()
    assert torch.equal(out, want), f"{(out != want).sum().item()} elements of W's slice misplaced"


def test_repeat_stability(K):
    """ten launches of 512 x 512 x 1024 on random data, all bitwise equal (a read placed ahead of its wait shows as a rare
    wrong tile)"""
    M, N, K_ = 512, 512, 1024
    x = rnd(M, K_, seed=1); w = rnd(N, K_, scale=0.1, seed=2)
    first = K.gemm(x, w, M, N, K_, tile_hint=NEW)
    same_bits(first, K.gemm(x, w, M, N, K_, tile_hint=OLD), "512x512x1024")
    for i in range(9):
        same_bits(K.gemm(x, w, M, N, K_, tile_hint=NEW), first, f"launch {i + 2}")


def test_strided_layouts_are_refused(K):
    """the 8-phase loop is built for the forward layout; asking for it with a K-strided operand is an error, not a fall-back"""
    x = rnd(256, 256, seed=1); w = rnd(256, 256, seed=2)
    with pytest.raises(Exception):
        K.gemm(x, w, 256, 256, 256, w_kstrided=True, tile_hint=NEW)
