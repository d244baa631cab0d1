"""vacnic_attn_bwd on the MI355X: the whole-row store path of dQ / dK / dV (16-byte aligned gradients leave through LDS as
128-byte row segments, unaligned ones as the accumulator layout's 8-byte pieces) and the one-kernel backward for Tq <= 64.

What must be exact is asserted as exact: the two store paths are bitwise equal, nothing outside the gradient views is written,
two calls on the same inputs are bitwise equal.  The one-kernel backward is compared with the three-launch path on a problem
padded to Tq' = 65 with queries whose dO is zero (they add nothing to any gradient), and with torch autograd in float64."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

FMIN = torch.finfo(torch.float32).min
SCALE = 0.125


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


def rnd(*shape, scale=1.0, dtype=torch.bfloat16, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to("cuda").to(dtype)


def close(a, b, rtol, atol, what=""):
    a = a.double(); b = b.double()
    err = (a - b).abs()
    bad = (err > atol + rtol * b.abs()).sum().item()
    assert bad == 0, f"{what}: {bad}/{a.numel()} off; max err {err.max().item():.4g} (ref max {b.abs().max().item():.4g})"


def close_order(a, b, what):
    """|a - b| <= 2^-7 |b| + 2^-9 max|b| on every element: two bf16 spacings plus a floor for near-zero elements, for two bf16
    roundings of fp32 sums that differ only in summation order."""
    a = a.double(); b = b.double()
    err = (a - b).abs()
    bound = 2.0 ** -7 * b.abs() + 2.0 ** -9 * b.abs().max()
    worst = (err / bound).max().item()
    print(f"{what}: max |a-b| {err.max().item():.4g}, max|b| {b.abs().max().item():.4g}, worst err/bound {worst:.3f}")
    bad = (err > bound).sum().item()
    assert bad == 0, f"{what}: {bad}/{a.numel()} beyond 2^-7|b| + 2^-9 max|b|; worst err/bound {worst:.3f}"


def len_mask(B, Tk, seed=3, single=None, empty=None):
    """uint8 [B, Tk] key mask of valid prefixes; batch row `single` keeps one key, batch row `empty` none."""
    lens = torch.randint(max(1, Tk // 4), Tk + 1, (B,), generator=torch.Generator().manual_seed(seed))
    if single is not None:
        lens[single] = 1
    if empty is not None:
        lens[empty] = 0
    return (torch.arange(Tk)[None, :] < lens[:, None]).to(torch.uint8).cuda()


def ref64(q, k, v, dout, H, key_mask, causal, M=None):
    """torch autograd in float64 on the bf16 inputs: additive finfo(float32).min masks (a fully masked row softmaxes uniformly,
    as in float32: the scores are absorbed), optional dropout factors M [B, H, Tq, Tk] applied after the softmax."""
    B, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    qa, ka, va = (t.double().reshape(B, -1, H, 64).transpose(1, 2).detach().clone().requires_grad_(True) for t in (q, k, v))
    s = qa @ ka.transpose(-1, -2) * SCALE
    if key_mask is not None:
        s = s + ((1.0 - key_mask.double()) * FMIN)[:, None, None, :]
    if causal:
        s = s + torch.full((Tq, Tk), FMIN, device=q.device, dtype=torch.float64).triu(1)
    p = torch.softmax(s, -1)
    if M is not None:
        p = p * M.to(p.device).double()
    out = p @ va
    out.backward(dout.double().reshape(B, Tq, H, 64).transpose(1, 2))
    back = lambda g: g.transpose(1, 2).reshape(B, -1, H * 64)
    return back(out.detach()), back(qa.grad), back(ka.grad), back(va.grad)


def offset_view(B, T, d, fill=None):
    """[B, T, d] bf16 view whose base sits 4 elements into a larger buffer: 8-byte aligned only."""
    buf = torch.empty(B * T * d + 8, device="cuda", dtype=torch.bfloat16)
    if fill is not None:
        buf.fill_(fill)
    v = buf[4:4 + B * T * d].view(B, T, d)
    assert v.data_ptr() % 16 == 8
    return v


def bwd_with_delta(K, q, k, v, out, dout, lse, dq, dk, dv, B, H, Tq, Tk, key_mask=None, causal=False, p_drop=0.0, seed=0):
    """K.attn_bwd with the delta buffer handed back."""
    delta = torch.empty((B, H, Tq), device=q.device, dtype=torch.float32)
    p = K._p
    K.call_struct("vacnic_attn_bwd", stream=K._stream(), q=p(q), k=p(k), v=p(v), out=p(out), dout=p(dout), lse=p(lse),
                  delta=p(delta), dq=p(dq), dk=p(dk), dv=p(dv), key_mask=p(key_mask), B=B, H=H, Tq=Tq, Tk=Tk,
                  ldq=q.stride(1), ldk=k.stride(1), ldv=v.stride(1), ldo=out.stride(1),
                  bsq=q.stride(0), bsk=k.stride(0), bsv=v.stride(0), bso=out.stride(0),
                  lddq=dq.stride(1), lddk=dk.stride(1), lddv=dv.stride(1),
                  bsdq=dq.stride(0), bsdk=dk.stride(0), bsdv=dv.stride(0), causal=int(causal), scale=SCALE, p_drop=p_drop, seed=seed,
                  seed_dev=p(None))
    return delta


# ------------------------------------------------------------------------------------------------ part A: whole-row stores
# B, H, Tq, Tk, masked.  Tq > 128: the dK/dV kernel and the dQ kernel, not the one-kernel backward.
ROW_SHAPES = [
    (1, 2, 129, 129, False),      # one row into the second 128-block and into the third 64-tile
    (2, 2, 200, 84, True),        # Tk < 128: the last wave of the dK/dV workgroup is all padding
    (1, 1, 257, 257, False),
]


@pytest.fixture(scope="module")
def row_problem(K):
    """(shape, p_drop) -> inputs, forward results and the gradients through aligned views, computed once."""
    cache = {}

    def get(shape, p_drop):
        if (shape, p_drop) not in cache:
            B, H, Tq, Tk, masked = shape
            d = H * 64
            q = rnd(B, Tq, d, seed=1); k = rnd(B, Tk, d, seed=2); v = rnd(B, Tk, d, seed=3); dout = rnd(B, Tq, d, seed=4)
            km = len_mask(B, Tk) if masked else None
            kw = dict(key_mask=km, causal=False, scale=SCALE, p_drop=p_drop, seed=11)
            out, lse = K.attn_fwd(q, k, v, B, H, Tq, Tk, **kw)
            dq = torch.empty_like(q); dk = torch.empty_like(k); dv = torch.empty_like(v)
            assert all(t.data_ptr() % 16 == 0 for t in (dq, dk, dv))
            K.attn_bwd(q, k, v, out, dout, lse, dq, dk, dv, B, H, Tq, Tk, **kw)
            cache[(shape, p_drop)] = (q, k, v, dout, km, kw, out, lse, dq, dk, dv)
        return cache[(shape, p_drop)]
    return get


@pytest.mark.parametrize("p_drop", [0.0, 0.25])
@pytest.mark.parametrize("shape", ROW_SHAPES)
def test_row_stores_bitwise_equal_to_piece_stores(K, row_problem, shape, p_drop):
    B, H, Tq, Tk, _ = shape
    d = H * 64
    q, k, v, dout, km, kw, out, lse, dq, dk, dv = row_problem(shape, p_drop)
    dq8 = offset_view(B, Tq, d); dk8 = offset_view(B, Tk, d); dv8 = offset_view(B, Tk, d)
    K.attn_bwd(q, k, v, out, dout, lse, dq8, dk8, dv8, B, H, Tq, Tk, **kw)
    assert torch.equal(dq, dq8), "dq"
    assert torch.equal(dk, dk8), "dk"
    assert torch.equal(dv, dv8), "dv"


# the three shapes above, and two that take the one-kernel backward (its own row stores of dK / dV per tile and of dQ)
@pytest.mark.parametrize("shape", ROW_SHAPES + [(1, 2, 33, 129, True), (2, 2, 64, 64, False)])
def test_row_stores_write_nothing_else_and_match_float64(K, shape):
    B, H, Tq, Tk, masked = shape
    d = H * 64
    SENT = -77.0
    q = rnd(B, Tq, d, seed=1); k = rnd(B, Tk, d, seed=2); v = rnd(B, Tk, d, seed=3); dout = rnd(B, Tq, d, seed=4)
    km = len_mask(B, Tk) if masked else None
    out, lse = K.attn_fwd(q, k, v, B, H, Tq, Tk, key_mask=km, scale=SCALE)
    dqb = torch.full((B, Tq + 3, 3 * d), SENT, device="cuda", dtype=torch.bfloat16)
    dkvb = torch.full((B, Tk + 3, 2 * d), SENT, device="cuda", dtype=torch.bfloat16)
    dq = dqb[:, :Tq, d:2 * d]; dk = dkvb[:, :Tk, :d]; dv = dkvb[:, :Tk, d:]
    assert all(t.data_ptr() % 16 == 0 for t in (dq, dk, dv))
    K.attn_bwd(q, k, v, out, dout, lse, dq, dk, dv, B, H, Tq, Tk, key_mask=km, scale=SCALE)
    assert (dqb[:, Tq:] == SENT).all() and (dqb[:, :, :d] == SENT).all() and (dqb[:, :, 2 * d:] == SENT).all(), "dq buffer"
    assert (dkvb[:, Tk:] == SENT).all(), "dk / dv buffer"
    _, rq, rk, rv = ref64(q, k, v, dout, H, km, False)
    s = max(1.0, math.sqrt(Tk / 64))
    close(dq, rq, 3e-2, 3e-2 * s, "dq"); close(dk, rk, 3e-2, 3e-2 * s, "dk"); close(dv, rv, 3e-2, 3e-2 * s, "dv")


# ------------------------------------------------------------------------------------- part B: one kernel for Tq <= 64
# B, H, Tq, Tk, mask ("causal" / "keys" / "keys1": key mask with one batch row keeping a single key / None), p_drop
SHORT_CASES = [
    (2, 2, 64, 64, "causal", 0.0),
    (2, 3, 20, 44, "keys", 0.0),          # second query block empty, Tk < 64
    (1, 2, 33, 129, "keys", 0.0),         # one row into the second query block, one key into the second 128-tile
    (2, 2, 64, 512, "keys1", 0.0),
    (1, 2, 1, 70, None, 0.0),
    # the dropout mask index depends on Tq for (b, h) > 0: B = H = 1
    (1, 1, 64, 64, "causal", 0.25),
    (1, 1, 40, 200, "keys", 0.25),
]


@pytest.mark.parametrize("B,H,Tq,Tk,mask,p_drop", SHORT_CASES)
def test_short_kernel_against_three_launches(K, B, H, Tq, Tk, mask, p_drop):
    """Tq' = 65: the Tq queries, dummy queries up to 64 and one more, all dummies with dO = 0 (so dP = delta = dS = 0 for them).
    attn_bwd at Tq' takes the delta sweep + dK/dV + dQ launches, at Tq the one kernel, on the same data."""
    d = H * 64
    Tq2 = 65
    q2 = rnd(B, Tq2, d, seed=1); k = rnd(B, Tk, d, seed=2); v = rnd(B, Tk, d, seed=3)
    dout2 = rnd(B, Tq2, d, seed=4); dout2[:, Tq:] = 0
    causal = mask == "causal"
    km = None
    if mask in ("keys", "keys1"):
        km = len_mask(B, Tk, single=1 if mask == "keys1" else None)
    kw = dict(key_mask=km, causal=causal, scale=SCALE, p_drop=p_drop, seed=5)
    out2, lse2 = K.attn_fwd(q2, k, v, B, H, Tq2, Tk, **kw)
    dq2 = torch.empty_like(q2); dk2 = torch.empty_like(k); dv2 = torch.empty_like(v)
    K.attn_bwd(q2, k, v, out2, dout2, lse2, dq2, dk2, dv2, B, H, Tq2, Tk, **kw)
    # the first Tq rows of that forward are the Tq run's
    q = q2[:, :Tq]; out = out2[:, :Tq]; dout = dout2[:, :Tq]; lse = lse2[:, :, :Tq].contiguous()
    dq = torch.empty(B, Tq, d, device="cuda", dtype=torch.bfloat16); dk = torch.empty_like(k); dv = torch.empty_like(v)
    K.attn_bwd(q, k, v, out, dout, lse, dq, dk, dv, B, H, Tq, Tk, **kw)
    close_order(dq, dq2[:, :Tq], "dq"); close_order(dk, dk2, "dk"); close_order(dv, dv2, "dv")


def _recover_attn_mask(K, q, k, B, H, Tq, Tk, p, seed, key_mask=None, causal=False):
    """(P o M / (1 - p_q)) of the kernel itself: with V = a one-hot window of 64 keys the output row of head h IS the dropped
    probability row restricted to that window."""
    pm = torch.zeros(B, H, Tq, Tk)
    for w0 in range(0, Tk, 64):
        v = torch.zeros(B, Tk, H * 64, device="cuda", dtype=torch.bfloat16)
        n = min(64, Tk - w0)
        for h in range(H):
            v[:, w0:w0 + n, h * 64:h * 64 + n] = torch.eye(n, device="cuda", dtype=torch.bfloat16)
        o, _ = K.attn_fwd(q, k, v, B, H, Tq, Tk, key_mask=key_mask, causal=causal, p_drop=p, seed=seed)
        pm[:, :, :, w0:w0 + n] = o.float().view(B, Tq, H, 64).permute(0, 2, 1, 3)[..., :n].cpu()
    return pm


@pytest.mark.parametrize("Tq,Tk", [(64, 300), (20, 44)])
def test_short_kernel_dropout_against_autograd(K, Tq, Tk):
    """Dropout at B, H > 1: the mask read off the forward (one-hot values), then torch autograd with that mask."""
    B, H, p, seed = 2, 2, 0.25, 777
    q = rnd(B, Tq, H * 64, scale=0.7, seed=1); k = rnd(B, Tk, H * 64, scale=0.7, seed=2); v = rnd(B, Tk, H * 64, seed=3)
    km = torch.ones(B, Tk, dtype=torch.uint8); km[1, Tk - 7:] = 0; km = km.cuda()
    pm = _recover_attn_mask(K, q, k, B, H, Tq, Tk, p, seed, key_mask=km)
    qf, kf = (t.float().cpu().view(B, -1, H, 64).transpose(1, 2) for t in (q, k))
    sc = qf @ kf.transpose(-1, -2) * SCALE + (1 - km.cpu().float())[:, None, None, :] * FMIN
    P = torch.softmax(sc, -1)
    big = P > 1e-3                                            # where a dropped entry is distinguishable from a tiny probability
    keep = pm > 0
    p_q = round(p * 256) / 256
    M = torch.where(keep | ~big, torch.full_like(P, 1 / (1 - p_q)), torch.zeros_like(P))
    out, lse = K.attn_fwd(q, k, v, B, H, Tq, Tk, key_mask=km, p_drop=p, seed=seed)
    dout = rnd(B, Tq, H * 64, seed=9)
    _, rq, rk, rv = ref64(q, k, v, dout, H, km, False, M=M)
    dq = torch.empty_like(q); dk = torch.empty_like(k); dv = torch.empty_like(v)
    K.attn_bwd(q, k, v, out, dout, lse, dq, dk, dv, B, H, Tq, Tk, key_mask=km, p_drop=p, seed=seed)
    for name, got, ref in (("dq", dq, rq), ("dk", dk, rk), ("dv", dv, rv)):
        e = ((got.double() - ref).norm() / ref.norm()).item()
        print(f"{name}: relative norm error {e:.4g}")
        assert e < 2e-2, (name, e)


def test_short_kernel_fully_masked_batch_row(K):
    """Every key of batch row 0 masked: the softmax is uniform over the keys, and so are the gradients' probabilities."""
    B, H, Tq, Tk = 2, 2, 40, 70
    d = H * 64
    q = rnd(B, Tq, d, seed=1); k = rnd(B, Tk, d, seed=2); v = rnd(B, Tk, d, seed=3); dout = rnd(B, Tq, d, seed=4)
    km = len_mask(B, Tk, empty=0)
    assert km[0].sum().item() == 0 and km[1].sum().item() > 0
    out, lse = K.attn_fwd(q, k, v, B, H, Tq, Tk, key_mask=km, scale=SCALE)
    dq = torch.empty_like(q); dk = torch.empty_like(k); dv = torch.empty_like(v)
    K.attn_bwd(q, k, v, out, dout, lse, dq, dk, dv, B, H, Tq, Tk, key_mask=km, scale=SCALE)
    assert all(torch.isfinite(t.float()).all() for t in (dq, dk, dv))
    _, rq, rk, rv = ref64(q, k, v, dout, H, km, False)
    assert rv[0].abs().max().item() > 0.01, "the uniform softmax has gradients"
    close_order(dq, rq, "dq"); close_order(dk, rk, "dk"); close_order(dv, rv, "dv")


@pytest.mark.parametrize("B,H,Tq,Tk,mask,p_drop", [(2, 2, 64, 300, "keys", 0.25), (2, 3, 20, 44, "keys", 0.0), (2, 2, 64, 64, "causal", 0.0)])
def test_short_kernel_run_to_run(K, B, H, Tq, Tk, mask, p_drop):
    d = H * 64
    q = rnd(B, Tq, d, seed=1); k = rnd(B, Tk, d, seed=2); v = rnd(B, Tk, d, seed=3); dout = rnd(B, Tq, d, seed=4)
    km = len_mask(B, Tk) if mask == "keys" else None
    kw = dict(key_mask=km, causal=mask == "causal", p_drop=p_drop, seed=5)
    out, lse = K.attn_fwd(q, k, v, B, H, Tq, Tk, scale=SCALE, **kw)
    res = []
    for _ in range(2):
        dq = torch.empty_like(q); dk = torch.empty_like(k); dv = torch.empty_like(v)
        delta = bwd_with_delta(K, q, k, v, out, dout, lse, dq, dk, dv, B, H, Tq, Tk, **kw)
        res.append((dq, dk, dv, delta))
    for name, a, b in zip(("dq", "dk", "dv", "delta"), *res):
        assert torch.equal(a, b), name
    assert torch.isfinite(res[0][3]).all()
