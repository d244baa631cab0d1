"""Attention kernels (csrc/attn.hip) against torch float64 on the host at the edges the older attention tests do not reach: the causal
flag beyond one tile (the forward / dQ tile cap with qblk > 0, the dK/dV kernel's t_begin > 0, both ring parities, t_begin ==
nq_tiles), key masks that are not prefixes (a clean tile after a dirty one, a dirty first tile), an empty batch row on the
three-launch backward (Tq > 64), lse as an output, the decode kernels' switch at Tk = 256 and Tq = 1 on the tiled kernel, the dropout
mask of the long path against a host Philox4x32-10 written from the comments above drop_ctx / drop_patch (not recovered from the
kernels), scale != 0.125 and the largest admitted Tk.

Reference: torch autograd in float64 on the bf16 inputs, additive finfo(float32).min masks, dropout factors applied after the softmax;
lse = logsumexp of the masked scores, rounded to fp32.

Bound (nothing in it is taken from a kernel's output): the same operation as a plain torch fp32 pipeline on the host, rounded to bf16
where the kernels round (P before P.V; P and dS before the dV, dK and dQ products; the outputs; delta = rowsum(dO o O) from the bf16 O
when Tq > 128, as vacnic_attn_bwd chooses it).  The margin of a quantity is 4 x the largest deviation of that emulation from float64
over the tensor, floored at 1e-6 max|ref| (the 4 covers summation order, v_exp_f32 against exp and the online rescaling, which the
emulation does not reproduce); bf16 outputs get 2^-8 |ref| per element on top, lse (fp32) the margin alone.  An lse that is
finfo.min in the reference (a row whose keys are all masked: log(count) is absorbed) is compared exactly and kept out of the margin
of the finite ones, which its magnitude would otherwise make meaningless.
Every check prints `ATTNCHK <case> <quantity> <shape> bound=<margin> err=<max |got - ref|> used=<max err / bound>`;
profiles/attn_tests.txt holds one run.

What is exact is asserted as exact: a masked key of a batch row that keeps a visible key, and a key no query sees under the causal
flag, get dK = dV = 0 bit for bit; p_drop that quantises to thr = 0 equals p_drop = 0 bitwise; two launches are bitwise equal; the
outputs sit in larger sentinel-filled buffers, the sentinel survives outside the views and no element inside them keeps it.

Out of scope: a key mask and the causal flag together hiding every visible key of SOME queries of a batch row that is not empty
(the model never passes both).

Found with these tests (both fixed in attn.hip):
  * attn_fwd_kernel wrote lse = finfo.min * ln 2 for an empty batch row (the running maximum lives in the log2 domain, the additive
    mask does not scale with it); the reference value is finfo.min (test_empty_batch_row, lse_empty_rows).
  * attn_bwd_dq_kernel and attn_bwd_dkv_kernel formed exp(score - lse) for such a row: 0 with the lse above, 1 (not 1 / Tk) with
    the right one, so dQ, dK, dV of the row were zero instead of the uniform softmax's gradients (test_empty_batch_row).
"""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

FMIN = torch.finfo(torch.float32).min
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
SENT = -77.0
SEED = 0xC0FFEE1234567891                # both key words non-zero
TK_MAX = 8192                            # check_common


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


# ------------------------------------------------------------------------------------------ host model
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on numpy arrays (or scalars) of 32-bit values held in uint64; returns the four output words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3, k0, k1))
    m0, m1, w0, w1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                     # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return c0, c1, c2, c3


def drop_threshold(p):
    return min(255, int(p * 256 + 0.5))


def inv_keep_of(thr):
    """256 / (256 - thr) as the fp32 number the kernels multiply with."""
    return float(np.float32(256.0) / np.float32(256 - thr))


def mix_seed(seed, counter):
    return seed ^ ((counter * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)


def attn_keep(B, H, Tq, Tk, seed, thr):
    """keep mask [B, H, Tq, Tk] of the attention-probability dropout: one block per 4 x 4 patch, index ((b H + h) ceil(Tq / 4) +
    (q >> 2)) ceil(Tk / 4) + (k >> 2), counter {idx_lo, idx_hi, 'ATTD', 0}, key = seed; the byte of (q & 3, k & 3) is bits
    8 (k & 3) of word q & 3; keep iff byte >= thr."""
    pq, pk = (Tq + 3) // 4, (Tk + 3) // 4
    u = lambda n: np.arange(n, dtype=np.uint64)                                        # noqa: E731
    idx = (u(B * H)[:, None, None] * np.uint64(pq) + u(pq)[None, :, None]) * np.uint64(pk) + u(pk)[None, None, :]
    w = philox4x32_10(idx & _M32, idx >> np.uint64(32), 0x41545444, 0, seed & 0xFFFFFFFF, seed >> 32)
    w = np.stack(w, axis=2)                                                            # [B H, pq, q & 3, pk]
    by = (w[..., None] >> (u(4) * np.uint64(8))) & np.uint64(0xFF)                     # [B H, pq, q & 3, pk, k & 3]
    return (by >= np.uint64(thr)).reshape(B, H, pq * 4, pk * 4)[:, :, :Tq, :Tk]


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = tuple(int(v) for v in philox4x32_10(*ctr, *key))
        assert got == want, f"{[hex(v) for v in got]} != {[hex(v) for v in want]}"
    assert [drop_threshold(p) for p in (0.25, 0.001, 0.999)] == [64, 0, 255]
    assert mix_seed(SEED, 0) == SEED and mix_seed(SEED, 1) == SEED ^ 0x9E3779B97F4A7C15


def test_host_mask_keep_rate_and_layout():
    thr = drop_threshold(0.25)
    m = attn_keep(1, 1, 256, 256, SEED, thr)
    se = (0.75 * 0.25 / m.size) ** 0.5
    assert abs(m.mean() - 192 / 256) < 5 * se, (m.mean(), se)
    # the patch of (q >> 2, k >> 2) = (1, 2) of a 256-key map is block 1 * 64 + 2; bytes by the rule of the docstring
    w = [int(x) for x in philox4x32_10(66, 0, 0x41545444, 0, SEED & 0xFFFFFFFF, SEED >> 32)]
    for qi in range(4):
        for ki in range(4):
            assert m[0, 0, 4 + qi, 8 + ki] == (((w[qi] >> (8 * ki)) & 0xFF) >= thr)
    # Tq and Tk enter the index through ceil(. / 4) for (b, h) > 0 only
    a, b = attn_keep(2, 2, 129, 130, SEED, thr), attn_keep(2, 2, 133, 130, SEED, thr)
    assert np.array_equal(a[0, 0], b[0, 0, :129]) and not np.array_equal(a[0, 1], b[0, 1, :129])
    assert attn_keep(1, 2, 5, 7, SEED, 0).all()
    assert not np.array_equal(m, attn_keep(1, 1, 256, 256, SEED ^ (1 << 32), thr))


# ------------------------------------------------------------------------------------------ reference, emulation, bound
def randn_bf16(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF16)


def len_mask(B, Tk, seed=3, single=None, empty=None, lens=None):
    """uint8 [B, Tk] key mask of valid prefixes (host); batch row `single` keeps one key, batch row `empty` none."""
    if lens is None:
        lens = torch.randint(max(1, Tk // 4), Tk + 1, (B,), generator=torch.Generator().manual_seed(seed))
    lens = torch.as_tensor(lens).clone()
    if single is not None:
        lens[single] = 1
    if empty is not None:
        lens[empty] = 0
    return (torch.arange(Tk)[None, :] < lens[:, None]).to(torch.uint8)


def heads(t, H):
    return t.reshape(t.shape[0], -1, H, 64).transpose(1, 2)                  # [B, H, T, 64]


def unheads(t):
    return t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1)             # [B, T, H * 64]


def mask_bias(Tq, Tk, key_mask, causal, dtype):
    s = torch.zeros(1, 1, Tq, Tk, dtype=dtype)
    if key_mask is not None:
        s = s + ((1.0 - key_mask.to(dtype)) * FMIN)[:, None, None, :]
    if causal:
        s = s + torch.full((Tq, Tk), FMIN, dtype=dtype).triu(1)
    return s


def ref64(q, k, v, dout, H, key_mask, causal, scale, M=None):
    """torch autograd in float64 on the bf16 inputs (host tensors): additive finfo(float32).min masks (a fully masked row softmaxes
    uniformly, as in float32: the scores are absorbed), dropout factors M [B, H, Tq, Tk] applied after the softmax."""
    qa, ka, va = (heads(t.double(), H).clone().requires_grad_(True) for t in (q, k, v))
    s = qa @ ka.transpose(-1, -2) * scale + mask_bias(q.shape[1], k.shape[1], key_mask, causal, F64)
    p = torch.softmax(s, -1)
    if M is not None:
        p = p * M.double()
    out = p @ va
    r = dict(out=unheads(out.detach()), lse=torch.logsumexp(s.detach(), -1).float())
    if dout is not None:
        out.backward(heads(dout.double(), H))
        r.update(dq=unheads(qa.grad), dk=unheads(ka.grad), dv=unheads(va.grad))
    return r


def emulate32(q, k, v, dout, H, key_mask, causal, scale, M=None, round_p=True):
    """The same operation in torch fp32 on the host, rounded to bf16 where the kernels round (module docstring).  round_p = False:
    the decode kernels, fp32 up to the output."""
    rb = lambda t: t.to(BF16).float()                                        # noqa: E731
    Tq = q.shape[1]
    qa, ka, va = (heads(t.float(), H) for t in (q, k, v))
    s = qa @ ka.transpose(-1, -2) * scale + mask_bias(Tq, k.shape[1], key_mask, causal, F32)
    p = torch.softmax(s, -1)
    pm = p if M is None else p * M.float()
    pb = rb(pm) if round_p else pm
    out = rb(pb @ va)
    r = dict(out=unheads(out), lse=torch.logsumexp(s, -1))
    if dout is not None:
        do = heads(dout.float(), H)
        dp = do @ va.transpose(-1, -2)
        dpm = dp if M is None else dp * M.float()
        delta = (do * out).sum(-1, keepdim=True) if Tq > 128 else (p * dpm).sum(-1, keepdim=True)
        ds = rb(p * (dpm - delta))
        r.update(dq=unheads(rb((ds @ ka) * scale)), dk=unheads(rb((ds.transpose(-1, -2) @ qa) * scale)),
                 dv=unheads(rb(pb.transpose(-1, -2) @ do)))
    return r


def check(fails, case, quantity, got, ref, emu, bf16=True):
    got, ref, emu = got.detach().double().cpu(), ref.double(), emu.double()
    margin = 4.0 * max((emu - ref).abs().max().item(), 1e-6 * ref.abs().max().item())
    bound = margin + (2.0 ** -8 * ref.abs() if bf16 else 0.0)
    err = (got - ref).abs()
    used = (err / bound).max().item()
    print(f"ATTNCHK {case} {quantity} {tuple(got.shape)} bound={margin:.4g} err={err.max().item():.4g} used={used:.3f}")
    if not used <= 1.0:
        fails.append(f"{case} {quantity}: used {used:.3f} of its bound (margin {margin:.4g}, max err {err.max().item():.4g})")


def check_lse(fails, case, got, ref, emu):
    got = got.detach().cpu()
    absorbed = ref == FMIN
    if absorbed.any():
        same = torch.equal(got[absorbed], ref[absorbed])
        err = (got[absorbed].double() - ref[absorbed].double()).abs().max().item()
        print(f"ATTNCHK {case} lse_empty_rows {(int(absorbed.sum()),)} bound=0 err={err:.4g} used={0.0 if same else float('inf'):.3f}")
        if not same:
            fails.append(f"{case} lse of the rows without a visible key: {got[absorbed][:4].tolist()} != finfo.min")
    if (~absorbed).any():
        check(fails, case, "lse", got[~absorbed], ref[~absorbed], emu[~absorbed], bf16=False)


# ------------------------------------------------------------------------------------------ problems (host side, computed once)
_PROBLEMS = {}


def problem(B, H, Tq, Tk, key_mask=None, causal=False, scale=0.125, p_drop=0.0, counter=None, backward=True, round_p=True):
    """inputs, float64 reference and fp32 emulation of a case; shared by the tests that run it more than once."""
    key = (B, H, Tq, Tk, None if key_mask is None else key_mask.numpy().tobytes(), causal, scale, p_drop, counter, backward, round_p)
    if key not in _PROBLEMS:
        d = H * 64
        scale = float(np.float32(scale))                                     # the kernels take it as an fp32 argument
        q, k, v = randn_bf16(B, Tq, d, seed=1), randn_bf16(B, Tk, d, seed=2), randn_bf16(B, Tk, d, seed=3)
        dout = randn_bf16(B, Tq, d, seed=4) if backward else None
        M = None
        thr = drop_threshold(p_drop)
        if thr:
            seed = SEED if counter is None else mix_seed(SEED, counter)
            M = torch.from_numpy(attn_keep(B, H, Tq, Tk, seed, thr)).double() * inv_keep_of(thr)
        args = (q, k, v, dout, H, key_mask, causal, scale)
        _PROBLEMS[key] = dict(B=B, H=H, Tq=Tq, Tk=Tk, q=q, k=k, v=v, dout=dout, key_mask=key_mask, causal=causal, scale=scale,
                              p_drop=p_drop, counter=counter, ref=ref64(*args, M=M), emu=emulate32(*args, M=M, round_p=round_p))
    return _PROBLEMS[key]


# ------------------------------------------------------------------------------------------ device side
def guarded3(B, T, d, lo, width):
    """[B, T, d] bf16 view at columns lo .. lo + d of a sentinel-filled [B, T + 3, width] buffer: strided and 16-byte aligned."""
    buf = torch.full((B, T + 3, width), SENT, device="cuda", dtype=BF16)
    view = buf[:, :T, lo:lo + d]
    assert view.data_ptr() % 16 == 0
    return buf, view


def offset_view(B, T, d):
    """[B, T, d] bf16 view whose base sits 4 elements into a sentinel-filled buffer: 8-byte aligned only."""
    buf = torch.full((B * T * d + 8,), SENT, device="cuda", dtype=BF16)
    view = buf[4:4 + B * T * d].view(B, T, d)
    assert view.data_ptr() % 16 == 8
    return buf, view


def intact(buf, view, what):
    """the sentinel survives everywhere outside `view` and nowhere inside it."""
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    inside.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(True)
    assert (buf[~inside] == SENT).all(), f"{what}: written outside the view"
    assert (view != SENT).all(), f"{what}: {(view == SENT).sum().item()} elements of the view were not written"


def run(K, pr, aligned=True, q=None, k=None, v=None, key_mask="problem", causal=None, p_drop=None):
    """forward (and backward when the problem has a dout) into sentinel-guarded buffers; returns out, lse, dq, dk, dv."""
    B, H, Tq, Tk = pr["B"], pr["H"], pr["Tq"], pr["Tk"]
    d = H * 64
    q = pr["q"].cuda() if q is None else q
    k = pr["k"].cuda() if k is None else k
    v = pr["v"].cuda() if v is None else v
    km = pr["key_mask"] if isinstance(key_mask, str) else key_mask
    km = None if km is None else km.cuda()
    cnt = None if pr["counter"] is None else torch.tensor([pr["counter"]], dtype=torch.int64, device="cuda")
    p, st = K._p, K._stream()
    common = dict(stream=st, q=p(q), k=p(k), v=p(v), key_mask=p(km), B=B, H=H, Tq=Tq, Tk=Tk, ldq=q.stride(1), ldk=k.stride(1),
                  ldv=v.stride(1), bsq=q.stride(0), bsk=k.stride(0), bsv=v.stride(0), causal=int(pr["causal"] if causal is None else causal),
                  scale=pr["scale"], p_drop=pr["p_drop"] if p_drop is None else p_drop, seed=SEED, seed_dev=p(cnt))
    ob, out = guarded3(B, Tq, d, d, 3 * d)
    lb = torch.full((B * H * Tq + 16,), SENT, device="cuda", dtype=F32)
    lse = lb[8:8 + B * H * Tq].view(B, H, Tq)
    K.call_struct("vacnic_attn_fwd", out=p(out), lse=p(lse), ldo=out.stride(1), bso=out.stride(0), **common)
    intact(ob, out, "out"); intact(lb, lse, "lse")
    if pr["dout"] is None:
        return out, lse
    _, dout = guarded3(B, Tq, d, d, 3 * d)                                   # dO shares the strides of O
    dout.copy_(pr["dout"])
    if aligned:
        (qb, dq), (kvb, dk) = guarded3(B, Tq, d, d, 3 * d), guarded3(B, Tk, d, 0, 2 * d)
        dv = kvb[:, :Tk, d:]
    else:
        (qb, dq), (kb, dk), (vb, dv) = offset_view(B, Tq, d), offset_view(B, Tk, d), offset_view(B, Tk, d)
    delta = torch.empty((B, H, Tq), device="cuda", dtype=F32)
    K.call_struct("vacnic_attn_bwd", out=p(out), dout=p(dout), lse=p(lse), delta=p(delta), dq=p(dq), dk=p(dk), dv=p(dv),
                  ldo=out.stride(1), bso=out.stride(0), lddq=dq.stride(1), lddk=dk.stride(1), lddv=dv.stride(1),
                  bsdq=dq.stride(0), bsdk=dk.stride(0), bsdv=dv.stride(0), **common)
    intact(qb, dq, "dq")
    if aligned:
        assert (kvb[:, Tk:] == SENT).all(), "dk / dv: written outside the views"
        assert (dk != SENT).all() and (dv != SENT).all(), "dk / dv: elements of the views were not written"
    else:
        intact(kb, dk, "dk"); intact(vb, dv, "dv")
    return out, lse, dq, dk, dv


def bits_zero(t):
    return bool((t.contiguous().view(torch.int16) == 0).all())


def run_and_check(K, case, pr, aligned=True):
    """one run of a problem against its float64 reference, every quantity, and the exact zeros of dK / dV."""
    res = run(K, pr, aligned)
    ref, emu, fails = pr["ref"], pr["emu"], []
    check(fails, case, "out", res[0], ref["out"], emu["out"])
    check_lse(fails, case, res[1], ref["lse"], emu["lse"])
    if pr["dout"] is not None:
        for name, got in zip(("dq", "dk", "dv"), res[2:]):
            check(fails, case, name, got, ref[name], emu[name])
            assert torch.isfinite(got.float()).all(), name
        dk, dv = res[3], res[4]
        km = pr["key_mask"]
        for b in range(pr["B"] if km is not None else 0):
            if km[b].any():                                                  # a masked key of a row that keeps a visible key
                hidden = (km[b] == 0).cuda()
                assert bits_zero(dk[b][hidden]) and bits_zero(dv[b][hidden]), f"dk / dv of the masked keys of batch row {b}"
        if pr["causal"] and pr["Tk"] > pr["Tq"]:                             # keys no query sees
            assert bits_zero(dk[:, pr["Tq"]:]) and bits_zero(dv[:, pr["Tq"]:]), "dk / dv of the keys past the last query"
    assert not fails, "; ".join(fails)
    return res


ALIGN = [pytest.param(True, id="rows16"), pytest.param(False, id="pieces8")]

# --------------------------------------------------------------------------------------------------- causal beyond one tile
CAUSAL = [
    (1, 2, 129, 129, 0.0),       # one query in block 1; t_begin = 2 with a single tile
    (1, 1, 257, 257, 0.0),       # three blocks; t_begin = 4; both ring parities
    (2, 4, 192, 192, 0.0),       # B H = 8: xcd_order's interleaved branch with nblk = 2
    (1, 2, 100, 100, 0.0),       # the DELTA_PASS sweep under the causal flag
    (1, 1, 100, 300, 0.0),       # key blocks 1, 2: t_begin == nq_tiles, zeros must be stored; forward cap 2 of 5 tiles
    (1, 1, 300, 100, 0.0),       # the cap never binds; queries beyond the keys
    (2, 2, 129, 129, 0.25),      # with dropout, the host mask in the reference
    (1, 1, 200, 200, 0.25),
]


@gpu
@pytest.mark.parametrize("aligned", ALIGN)
@pytest.mark.parametrize("B,H,Tq,Tk,p_drop", CAUSAL)
def test_causal_beyond_one_tile(K, B, H, Tq, Tk, p_drop, aligned):
    pr = problem(B, H, Tq, Tk, causal=True, p_drop=p_drop)
    run_and_check(K, f"causal{'_drop' if p_drop else ''}_{B}x{H}x{Tq}x{Tk}_{'rows16' if aligned else 'pieces8'}", pr, aligned)


# --------------------------------------------------------------------------------------------------- holed key masks
def holed_mask():
    km = torch.ones(2, 200, dtype=torch.uint8)
    km[0, 70:72] = 0; km[0, 100:120] = 0          # tile 1 dirty; tiles 0, 2 and 3 clean
    km[1, 0:5] = 0; km[1, 197:200] = 0            # first and last tile dirty
    return km


@gpu
@pytest.mark.parametrize("name", ["holes", "prefix8"])
def test_key_masks_that_are_not_suffix_tiles(K, name):
    if name == "holes":
        pr = problem(2, 2, 130, 200, key_mask=holed_mask())
    else:                        # B H = 8 with 2 query blocks and 3 key blocks: the interleaved xcd_order branch of the dK/dV kernel
        pr = problem(1, 8, 129, 300, key_mask=len_mask(1, 300, lens=[170]))
    run_and_check(K, f"mask_{name}_{pr['B']}x{pr['H']}x{pr['Tq']}x{pr['Tk']}", pr)


# --------------------------------------------------------------------------------------------------- empty batch row, Tq > 64
@gpu
@pytest.mark.parametrize("B,H,Tq,Tk", [(2, 2, 65, 70), (2, 2, 129, 70), (2, 2, 200, 200)])
def test_empty_batch_row(K, B, H, Tq, Tk):
    """Every key of batch row 0 masked, on the delta sweep + dK/dV + dQ launches: the softmax is uniform over the keys and the
    gradients are those of the uniform softmax.  Before the fix in attn.hip the forward wrote lse = finfo.min * ln 2 for the row and
    exp(score - lse) made dQ, dK, dV of the row exactly zero (with lse = finfo.min they would have been Tk times too large)."""
    km = len_mask(B, Tk, empty=0)
    assert km[0].sum().item() == 0 and km[1].sum().item() > 0
    pr = problem(B, H, Tq, Tk, key_mask=km)
    assert pr["ref"]["dv"][0].abs().max().item() > 0.01, "the uniform softmax has gradients"
    assert (pr["ref"]["lse"][0] == FMIN).all()
    run_and_check(K, f"empty_row_{B}x{H}x{Tq}x{Tk}", pr)


# --------------------------------------------------------------------------------------------------- decode kernels, Tq = 1
def cache_views(pr):
    """q a column block of a wider buffer, K / V the two halves of a cache longer than Tk (as the decoder step passes them)."""
    B, H, Tk = pr["B"], pr["H"], pr["Tk"]
    d = H * 64
    qb = torch.zeros(B, 1, 3 * d, dtype=BF16, device="cuda"); qb[..., 2 * d:] = pr["q"].cuda()
    cache = randn_bf16(B, Tk + 3, 2 * d, seed=9).cuda()
    cache[:, :Tk, :d] = pr["k"].cuda(); cache[:, :Tk, d:] = pr["v"].cuda()
    return qb[..., 2 * d:], cache[:, :Tk, :d], cache[:, :Tk, d:]


@gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Tk", [255, 256, 257])
def test_decode_kernel_switch_point(K, Tk, masked):
    """attn_decode_kernel<1> up to Tk = 255, <4> from 256 on; out and lse, masked runs (batch row 0 empty) included."""
    B, H = 2, 3
    km = len_mask(B, Tk, empty=0) if masked else None
    pr = problem(B, H, 1, Tk, key_mask=km, backward=False, round_p=False)
    q, k, v = cache_views(pr)
    out, lse = run(K, pr, q=q, k=k, v=v)
    fails, case = [], f"decode_{'masked' if masked else 'plain'}_{B}x{H}x1x{Tk}"
    check(fails, case, "out", out, pr["ref"]["out"], pr["emu"]["out"])
    check_lse(fails, case, lse, pr["ref"]["lse"], pr["emu"]["lse"])
    assert not fails, "; ".join(fails)


@gpu
def test_single_query_on_the_tiled_kernel(K):
    """Tq = 1 with the causal flag or with dropout is not the decode kernel's: attn_fwd_kernel with 127 padding queries.  Under the
    causal flag the one query sees key 0 alone, which the decode kernel computes from the same q / k / v with a key mask that keeps
    key 0: the two outputs are compared with each other as well, within the bound."""
    B, H, Tk = 2, 3, 70
    fails = []
    pr = problem(B, H, 1, Tk, causal=True, backward=False)
    q, k, v = cache_views(pr)
    out, lse = run(K, pr, q=q, k=k, v=v)
    check(fails, "tq1_causal", "out", out, pr["ref"]["out"], pr["emu"]["out"])
    check_lse(fails, "tq1_causal", lse, pr["ref"]["lse"], pr["emu"]["lse"])
    out_d, lse_d = run(K, pr, q=q, k=k, v=v, key_mask=len_mask(B, Tk, lens=[1, 1]), causal=False)
    check(fails, "tq1_causal_vs_decode", "out", out, out_d.double().cpu(), pr["emu"]["out"] - pr["ref"]["out"] + out_d.double().cpu())
    check(fails, "tq1_causal_vs_decode", "lse", lse, lse_d.double().cpu(), pr["emu"]["lse"].double() - pr["ref"]["lse"] + lse_d.double().cpu(),
          bf16=False)
    pr = problem(B, H, 1, Tk, p_drop=0.25, backward=False)
    q, k, v = cache_views(pr)
    out, lse = run(K, pr, q=q, k=k, v=v)
    check(fails, "tq1_drop", "out", out, pr["ref"]["out"], pr["emu"]["out"])
    check_lse(fails, "tq1_drop", lse, pr["ref"]["lse"], pr["emu"]["lse"])
    assert not fails, "; ".join(fails)


# --------------------------------------------------------------------------------------------------- dropout: the host mask
@gpu
@pytest.mark.parametrize("B,H,Tq,Tk,masked,counter", [(2, 2, 129, 130, False, None), (2, 3, 67, 131, True, None), (2, 3, 67, 131, True, 5)])
def test_dropout_against_the_host_mask(K, B, H, Tq, Tk, masked, counter):
    """p = 0.25 on the long path, Tq % 4 != 0, Tk % 4 != 0, (b, h) > 0: the forward, dQ and dK/dV kernels regenerate the mask through
    different lane layouts, the reference takes the host's.  counter: seed_dev set, the seed mixed on the device as mix_seed."""
    pr = problem(B, H, Tq, Tk, key_mask=len_mask(B, Tk) if masked else None, p_drop=0.25, counter=counter)
    run_and_check(K, f"drop_host_{B}x{H}x{Tq}x{Tk}{'_seed_dev' if counter is not None else ''}", pr)


@gpu
def test_p_drop_below_one_threshold_step_is_no_dropout(K):
    """p_drop = 0.001 quantises to thr = 0: bitwise the run without dropout."""
    pr = problem(2, 2, 129, 130, key_mask=len_mask(2, 130))
    a, b = run(K, pr), run(K, pr, p_drop=0.001)
    for name, x, y in zip(("out", "lse", "dq", "dk", "dv"), a, b):
        assert torch.equal(x, y), name


@gpu
@pytest.mark.parametrize("B,H,Tq,Tk,causal,p_drop", [(1, 1, 257, 257, True, 0.0), (2, 3, 67, 131, False, 0.25), (1, 1, 100, 300, True, 0.0)])
def test_two_launches_are_bitwise_equal(K, B, H, Tq, Tk, causal, p_drop):
    pr = problem(B, H, Tq, Tk, key_mask=None if causal else len_mask(B, Tk), causal=causal, p_drop=p_drop)
    a, b = run(K, pr), run(K, pr)
    for name, x, y in zip(("out", "lse", "dq", "dk", "dv"), a, b):
        assert torch.equal(x, y), name


# --------------------------------------------------------------------------------------------------- scale
@gpu
@pytest.mark.parametrize("B,H,Tq,Tk,masked", [(1, 2, 129, 129, False), (2, 2, 65, 84, True)])
def test_scale_other_than_an_eighth(K, B, H, Tq, Tk, masked):
    pr = problem(B, H, Tq, Tk, key_mask=len_mask(B, Tk) if masked else None, scale=0.3)
    run_and_check(K, f"scale0.3_{B}x{H}x{Tq}x{Tk}", pr)


# --------------------------------------------------------------------------------------------------- the Tk bound
@gpu
def test_largest_admitted_tk(K):
    """Tk = 8192: the forward and dQ launches take 66,048 bytes of dynamic LDS (32 KiB ring + 4 Tk_pad + Tk_pad / 16), above 64 KiB
    from Tk_pad = 8128 on; attn.hip declares that size for them (hipFuncAttributeMaxDynamicSharedMemorySize)."""
    pr = problem(1, 1, 65, TK_MAX, key_mask=len_mask(1, TK_MAX))
    run_and_check(K, f"tk_max_1x1x65x{TK_MAX}", pr)


@gpu
def test_tk_beyond_the_bound_is_refused_on_the_host(K):
    """Tk = 8193: VACNIC_UNSUPPORTED (5) from check_common, before anything is launched."""
    from vacnic_amd._lib import VacnicError
    Tk = TK_MAX + 1
    z = lambda T: torch.zeros(1, T, 64, device="cuda", dtype=BF16)          # noqa: E731
    q, k, v, out, dout = z(65), z(Tk), z(Tk), z(65), z(65)
    with pytest.raises(VacnicError, match=rf"status 5: attn_fwd: Tk={Tk}"):
        K.attn_fwd(q, k, v, 1, 1, 65, Tk)
    lse = torch.zeros(1, 1, 65, device="cuda")
    with pytest.raises(VacnicError, match=rf"status 5: attn_bwd: Tk={Tk}"):
        K.attn_bwd(q, k, v, out, dout, lse, z(65), z(Tk), z(Tk), 1, 1, 65, Tk)
