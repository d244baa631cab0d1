"""vacnic_attn_probs on the MI355X: the attention map softmax(scale q k^T + masks) (attn_weights_reshaped, MFULL:509-544)
against fp32 torch on the same bf16-rounded inputs.

What is exact is asserted as exact (masked and causal entries == 0, a fully masked row == 1/Tk, two launches bit-identical);
the row sums carry a derived bound; the closeness bound is 4x the error measured on the GPU (profiles/attn_probs_error.txt)."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

FMIN = torch.finfo(torch.float32).min

# Closeness to the torch yardstick.  Both sides start from the same bf16 inputs and accumulate in fp32, so they differ only in
# exp (v_exp_f32 on scale*log2(e)-folded scores against expf) and in summation order.  Measured over every case below
# (profiles/attn_probs_error.txt): max |p - ref| = 7.153e-07 and max |p - ref| / ref = 4.086e-06, both at the encoder
# self-attention shape.  The bounds are 4x the measured maxima — headroom across machines and compiler versions — and far
# inside the 1e-3 that test_attention_single_query_decode_path grants the forward kernel's lse.  The relative error is taken
# over entries whose reference is >= REL_FLOOR: below it the probability nears the denormal range of fp32, where v_exp_f32
# flushes to zero and a relative figure means nothing.
ABS_BOUND = 4 * 7.153e-07
REL_BOUND = 4 * 4.086e-06
REL_FLOOR = 1e-30
assert 0 < ABS_BOUND <= 1e-3 and 0 < REL_BOUND <= 1e-3


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


def rnd(*shape, scale=1.0, dtype=torch.bfloat16, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to("cuda").to(dtype)


def probs_ref(q, k, H, key_mask, causal, scale):
    """fp32 torch: softmax(scale q k^T + additive finfo.min masks), [B, H, Tq, Tk] (the formulas of MFULL:509-541)."""
    B, Tq, Tk = q.shape[0], q.shape[1], k.shape[1]
    q4 = q[..., :H * 64].float().reshape(B, Tq, H, 64)
    k4 = k[..., :H * 64].float().reshape(B, Tk, H, 64)
    s = torch.einsum("bqhd,bkhd->bhqk", q4 * scale, k4)
    if key_mask is not None:
        s = s + ((1.0 - key_mask.float()) * FMIN)[:, None, None, :]
    if causal:
        s = s + torch.full((Tq, Tk), FMIN, device=q.device).triu(1)
    return torch.softmax(s, dim=-1)


# B, H, Tq, Tk, masked, causal, layout.  layout: "kvq" = q and k are column blocks of ONE fused [B, T, 3d] projection output
# ([k | v | q], self-attention), "kv" = k is the first block of a fused [B, Tk, 2d] k|v buffer and q its own tensor
# (cross-attention), "plain" = two contiguous tensors.
MODEL_CASES = [
    (8, 16, 512, 512, True, False, "kvq"),      # encoder text self-attention (bart-large)
    (2, 12, 512, 512, True, False, "kvq"),      # ... bart-base heads
    (4, 16, 512, 40, False, False, "kv"),       # text <- [image prompt ; name prefix]
    (2, 12, 512, 30, False, False, "kv"),       # ... prompt 10 + prefix 20: rows not 16-byte aligned
    (4, 16, 80, 84, True, False, "kv"),         # names <- [faces ; names]
    (8, 16, 64, 64, False, True, "kvq"),        # decoder self-attention, causal
    (3, 12, 64, 64, False, True, "kvq"),
    (8, 16, 64, 512, True, False, "kv"),        # decoder cross-attention
    (2, 1, 64, 64, True, True, "plain"),        # causal and key mask together (finfo.min twice = -inf)
]
_H = itertools.cycle([1, 12, 16])
RAGGED_CASES = [(2, next(_H), tq, tk, True, False, lay)
                for (tq, tk), lay in zip(itertools.product([1, 37, 600], repeat=2), itertools.cycle(["kv", "plain"]))]
RAGGED_CASES += [(2, 12, 37, 37, False, True, "kvq"), (1, 1, 600, 600, False, True, "kvq")]
CASES = MODEL_CASES + RAGGED_CASES


def make_case(B, H, Tq, Tk, masked, causal, layout, seed=0):
    d = H * 64
    if layout == "kvq":
        assert Tq == Tk
        kvq = rnd(B, Tq, 3 * d, scale=1.5, seed=seed + 1)
        q, k = kvq[..., 2 * d:], kvq[..., :d]
    elif layout == "kv":
        q = rnd(B, Tq, d, scale=1.5, seed=seed + 1)
        k = rnd(B, Tk, 2 * d, scale=1.5, seed=seed + 2)[..., :d]
    else:
        q = rnd(B, Tq, d, scale=1.5, seed=seed + 1)
        k = rnd(B, Tk, d, scale=1.5, seed=seed + 2)
    mask = None
    if masked:
        lens = torch.randint(1, Tk + 1, (B,), generator=torch.Generator().manual_seed(seed + 3))
        if not causal:
            lens[0] = 0                                      # a fully masked batch row -> uniform 1/Tk
        mask = (torch.arange(Tk)[None, :] < lens[:, None]).to(torch.uint8).cuda()
    return q, k, mask


def errors(out, ref):
    """(max absolute error, max relative error over reference entries >= REL_FLOOR)."""
    err = (out - ref).abs()
    big = ref >= REL_FLOOR
    rel = (err[big] / ref[big]).max().item() if big.any() else 0.0
    return err.max().item(), rel


@pytest.mark.parametrize("B,H,Tq,Tk,masked,causal,layout", CASES)
def test_attn_probs_matches_torch(K, B, H, Tq, Tk, masked, causal, layout):
    q, k, mask = make_case(B, H, Tq, Tk, masked, causal, layout)
    out = K.attn_probs(q, k, B, H, Tq, Tk, key_mask=mask, causal=causal, scale=0.125)
    again = K.attn_probs(q, k, B, H, Tq, Tk, key_mask=mask, causal=causal, scale=0.125)
    assert out.shape == (B, H, Tq, Tk) and out.dtype == torch.float32 and out.is_contiguous()
    ref = probs_ref(q, k, H, mask, causal, 0.125)
    max_abs, max_rel = errors(out, ref)
    rowsum = out.double().sum(-1)
    max_sum = (rowsum - 1.0).abs().max().item()
    print(f"attn_probs B={B} H={H} Tq={Tq} Tk={Tk} masked={masked} causal={causal} {layout}: "
          f"max_abs={max_abs:.3e} max_rel={max_rel:.3e} max|rowsum-1|={max_sum:.3e}")

    # ---- exact conditions
    assert torch.equal(out, again), "two launches of the same inputs differ"
    assert torch.isfinite(out).all() and (out >= 0).all()
    if mask is not None:
        live = mask.sum(1) > 0                                # rows with at least one visible key
        dead_keys = (mask == 0) & live[:, None]               # [B, Tk]
        assert (out.permute(0, 3, 1, 2)[dead_keys] == 0).all(), "a masked key got probability"
        if (~live).any():
            # every score is finfo.min exactly (it absorbs any finite score), exp(0) = 1, the sum Tk is exact and 1/Tk is
            # rounded once: within one ulp of fp32(1/Tk)
            uni = out[~live]
            assert ((uni - 1.0 / Tk).abs() <= 2.0 ** -23 / Tk).all(), "fully masked row is not uniform 1/Tk"
    if causal:
        upper = torch.ones(Tq, Tk, dtype=torch.bool, device="cuda").triu(1)
        assert (out[..., upper] == 0).all(), "the causal upper triangle got probability"

    # ---- every row sums to 1.  The check itself sums in fp64, so what is bounded is the kernel's own arithmetic, to first
    # order in u = 2^-24:  p_j = e_j * (1 / l) with l the fp32 sum of the Tk terms e_j = 2^(v_j - m) <= 1 of sweep 1.
    #   - the sum of Tk positive fp32 terms, in any order, is off by at most (Tk - 1) u relative;
    #   - each e_j carries 2u from v_exp_f32 (1 ulp) and |v_j - m| u ln2 from the rounded subtraction, in each sweep; weighted
    #     by e_j = 2^-(m - v_j) the latter is at most 0.53 ln2 u = 0.37 u per term relative to l >= 1 (the maximum's term is 1),
    #     so at most 0.37 Tk u for the row;
    #   - the online rescaling of sweep 1 adds 3 roundings per 64-key tile, 3 Tk / 64 u; the reciprocal and the product 2u more.
    # Together (Tk - 1 + 0.37 Tk + 0.05 Tk + 2 * 2 + 2) u < (1.42 Tk + 6) 2^-24 < (Tk + 8) 2^-23.
    assert max_sum <= (Tk + 8) * 2.0 ** -23, f"row sums off by {max_sum:.3e}"

    # ---- closeness to the yardstick
    assert max_abs <= ABS_BOUND, f"max abs err {max_abs:.3e} > {ABS_BOUND:.3e}"
    assert max_rel <= REL_BOUND, f"max rel err {max_rel:.3e} > {REL_BOUND:.3e}"


def test_attn_probs_argument_errors(K):
    from vacnic_amd import _lib
    q = rnd(2, 16, 128, seed=1); k = rnd(2, 24, 128, seed=2)
    out = torch.empty(2, 2, 16, 24, device="cuda")
    args = dict(stream=K._stream(), k=k.data_ptr(), out=out.data_ptr(), key_mask=None, B=2, H=2, Tq=16, Tk=24, ldq=128, ldk=128,
                bsq=16 * 128, bsk=24 * 128, causal=0, scale=0.125)
    with pytest.raises(ValueError, match="null operand"):
        _lib.call_struct("vacnic_attn_probs", q=None, **args)
    with pytest.raises(ValueError, match="do not fit the row strides"):
        K.attn_probs(q, k, 2, 3, 16, 24)                     # 3 heads = 192 columns in rows of 128
    with pytest.raises(ValueError, match="multiples of 8"):
        _lib.call_struct("vacnic_attn_probs", q=q.data_ptr(), **dict(args, ldq=132))
    torch.cuda.synchronize()


def test_attn_probs_is_replayed_by_a_recorded_plan(K):
    from vacnic_amd import _lib
    B, H, Tq, Tk = 2, 2, 37, 84
    q, k, mask = make_case(B, H, Tq, Tk, True, False, "kv", seed=5)
    want = K.attn_probs(q, k, B, H, Tq, Tk, key_mask=mask)
    out = torch.zeros_like(want)
    h = int(_lib.lib.vacnic_plan_begin())
    assert h >= 0
    try:
        _lib.call_struct("vacnic_attn_probs", stream=K._stream(), q=q.data_ptr(), k=k.data_ptr(), out=out.data_ptr(),
                         key_mask=mask.data_ptr(), B=B, H=H, Tq=Tq, Tk=Tk, ldq=q.stride(1), ldk=k.stride(1), bsq=q.stride(0),
                         bsk=k.stride(0), causal=0, scale=0.125)
    finally:
        _lib.check(_lib.lib.vacnic_plan_end(h))
    try:
        assert int(_lib.lib.vacnic_plan_size(h)) == 1
        assert torch.equal(out, want)
        out.zero_()
        _lib.call("vacnic_plan_replay", h, 0, 1)
        assert torch.equal(out, want), "the replayed plan did not rewrite the map"
    finally:
        _lib.check(_lib.lib.vacnic_plan_destroy(h))
