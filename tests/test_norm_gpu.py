"""LayerNorm family (csrc/norm.hip): every D / R dispatch edge against torch float64 on the CPU, and the three regenerated
dropout masks against a host Philox4x32-10 written from the comments of common.h / norm.hip (not recovered from the kernels).

Tolerances (none is taken from a kernel's output):
  * fp32 outputs (mean, rstd, dgamma, dbeta, demb, dpos, name_embed): the same torch graph is evaluated in fp32 on the CPU
    from the same inputs; the kernel may deviate from the float64 result by 8x the largest fp32-torch deviation at that
    shape (a different but legitimate summation order: wave shuffle tree, per-block partials, atomics), floored at
    1e-6 * max|ref|.
  * bf16 outputs (out, dx, dresidual): one rounding of an fp32 result: 2^-8 * |ref| + atol, atol measured as above.
  * masks are compared exactly.
Every check prints `NORMCHK <what> <shape> bound=<margin> err=<observed>`; profiles/norm_tests.txt holds one run of them.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

EPS = float(np.float32(1e-5))            # the kernels take eps as an fp32 argument
SEED = 0xC0FFEE1234567891                # both key words non-zero
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


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


def _bytes8(lo, hi):
    sh = (np.arange(4, dtype=np.uint64) * np.uint64(8))
    return np.concatenate([(lo[..., None] >> sh) & np.uint64(0xFF), (hi[..., None] >> sh) & np.uint64(0xFF)], axis=-1)


def hidden_keep(R, D, seed, thr):
    """keep mask [R, D] of the hidden-state dropout (drop8 / actdrop_factors8): chunk c = lane + 64 i of a row takes words
    2 (i & 1), 2 (i & 1) + 1 of block row * 128 + lane + 64 (i >> 1), counter {blk_lo, blk_hi, 'LNDR', 0}, key = seed."""
    c = np.arange(D // 8, dtype=np.uint64)[None, :]
    lane, i = c & np.uint64(63), c >> np.uint64(6)
    row = np.arange(R, dtype=np.uint64)[:, None]
    blk = row * np.uint64(128) + lane + np.uint64(64) * (i >> np.uint64(1))
    w = philox4x32_10(blk & _M32, blk >> np.uint64(32), 0x4C4E4452, 0, seed & 0xFFFFFFFF, seed >> 32)
    odd = np.broadcast_to((i & np.uint64(1)) == 1, blk.shape)
    lo, hi = np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])
    return (_bytes8(lo, hi) >= np.uint64(thr)).reshape(R, D)


def flat_keep(n, seed, thr):
    """keep mask [n] of the flat activation dropout (actdrop_block): element e takes byte e & 15 of block e >> 4."""
    blk = np.arange((n + 15) // 16, dtype=np.uint64)
    w = philox4x32_10(blk & _M32, blk >> np.uint64(32), 0x41435444, 0, seed & 0xFFFFFFFF, seed >> 32)
    b = np.concatenate([_bytes8(w[0], w[1]), _bytes8(w[2], w[3])], axis=-1)
    return (b >= np.uint64(thr)).reshape(-1)[:n]


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = tuple(int(v) for v in philox4x32_10(*ctr, *key))
        assert got == want, f"{[hex(v) for v in got]} != {[hex(v) for v in want]}"
    # vectorised == scalar
    c0 = np.array([0, 0xFFFFFFFF, 0x243F6A88], dtype=np.uint64)
    v = philox4x32_10(c0, [0, 0xFFFFFFFF, 0x85A308D3], [0, 0xFFFFFFFF, 0x13198A2E], [0, 0xFFFFFFFF, 0x03707344],
                      [0, 0xFFFFFFFF, 0xA4093822], [0, 0xFFFFFFFF, 0x299F31D0])
    assert [int(v[0][k]) for k in range(3)] == [0x6627E8D5, 0x408F276D, 0xD16CFE09]


def test_host_thresholds_and_seed_mix():
    assert [drop_threshold(p) for p in (0.1, 0.001, 0.999, 0.2)] == [26, 0, 255, 51]
    assert mix_seed(SEED, 0) == SEED
    assert mix_seed(SEED, 1) == SEED ^ 0x9E3779B97F4A7C15
    assert mix_seed(0, (1 << 40) + 3) == (((1 << 40) + 3) * 0x9E3779B97F4A7C15) % (1 << 64)
    assert inv_keep_of(255) == 256.0 and inv_keep_of(0) == 1.0


def test_host_hidden_mask_statistics():
    thr = drop_threshold(0.1)
    m = hidden_keep(261, 2048, SEED, thr)
    assert abs(m.mean() - (1 - thr / 256)) < 0.01, m.mean()
    m2 = hidden_keep(4100, 64, SEED, thr)
    assert abs(m2.mean() - (1 - thr / 256)) < 0.01, m2.mean()
    assert not np.array_equal(m[0], m[1]) and not np.array_equal(m[7], m[260])           # the row is part of the block index
    for lane in (0, 17, 63):                                                              # chunks i, i + 1 of one lane
        ch = [m[:, (lane + 64 * i) * 8:(lane + 64 * i + 1) * 8] for i in range(4)]
        for i in range(3):
            assert not np.array_equal(ch[i], ch[i + 1]), (lane, i)
    assert not np.array_equal(m, hidden_keep(261, 2048, SEED ^ 1, thr))                   # key low word
    assert not np.array_equal(m, hidden_keep(261, 2048, SEED ^ (1 << 32), thr))           # key high word
    assert abs(hidden_keep(261, 2048, SEED, 255).mean() - 1 / 256) < 0.01
    assert hidden_keep(5, 520, SEED, 0).all()


def test_host_flat_mask_statistics():
    thr = drop_threshold(0.2)
    m = flat_keep(1 << 16, SEED, thr)
    assert abs(m.mean() - (1 - thr / 256)) < 0.01, m.mean()
    assert np.array_equal(flat_keep(24, SEED, thr), m[:24])
    assert not np.array_equal(m[:16], m[16:32])
    assert not np.array_equal(m[:4096], hidden_keep(1, 4096, SEED, thr)[0])               # counter word 2 tells the two apart


# -------------------------------------------------------------------------------------------- plumbing
@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


def cpu_randn(*shape, seed, scale=1.0, dtype=BF16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


def host(t):
    return None if t is None else t.detach().to("cpu")


def f32_margin(ref64, ref32):
    """8x the deviation of fp32 torch from float64 at this shape, floored at 1e-6 * max|ref|."""
    dev = (ref32.to(F64) - ref64).abs().max().item()
    return max(8.0 * dev, 1e-6 * ref64.abs().max().item())


def check(what, got, r64, r32, key):
    """fp32 outputs: |got - ref64| <= margin.  bf16 outputs: <= 2^-8 |ref64| + margin."""
    ref64, ref32 = r64[key], r32[key]
    got = host(got).to(F64).reshape(ref64.shape)
    margin = f32_margin(ref64, ref32)
    bound = margin + (ref64.abs() * 2.0 ** -8 if key in ("out", "dx", "dres") else 0.0)
    err = (got - ref64).abs()
    excess = (err - bound).max().item()
    used = (err / bound).max().item()                   # largest share of its bound that any element uses
    print(f"NORMCHK {what} {key} {tuple(ref64.shape)} bound={margin:.3e} err={err.max().item():.3e} "
          f"refmax={ref64.abs().max().item():.3e} used={used:.3f}")
    assert excess <= 0.0, f"{what} {key}: {(err > bound).sum().item()}/{err.numel()} off, max err {err.max().item():.4g}, margin {margin:.4g}"


# -------------------------------------------------------------------------------------- add_ln reference
def add_ln_inputs(R, D, seed=0):
    return dict(x=cpu_randn(R, D, seed=seed + 1), res=cpu_randn(R, D, seed=seed + 2), dout=cpu_randn(R, D, seed=seed + 5),
                g=cpu_randn(D, seed=seed + 3, dtype=F32) * 0.3 + 1.0, b=cpu_randn(D, seed=seed + 4, dtype=F32) * 0.5,
                dg0=cpu_randn(D, seed=seed + 6, dtype=F32) + 3.0, db0=cpu_randn(D, seed=seed + 7, dtype=F32) - 2.0)


def add_ln_ref(t, dtype, keep=None, inv_keep=1.0, residual=True):
    x = leaf(t["x"], dtype)
    g = leaf(t["g"], dtype); b = leaf(t["b"], dtype)
    h = x if keep is None else x * (torch.from_numpy(keep).to(dtype) * inv_keep)
    if residual:
        h = h + t["res"].to(dtype)
    h = h * 1                                 # a non-leaf of its own: h.grad is d loss / d (residual + dropout(x))
    h.retain_grad()
    out = F.layer_norm(h, (h.shape[-1],), g, b, EPS)
    out.backward(t["dout"].to(dtype))
    hd = h.detach()
    return dict(out=out.detach(), mean=hd.mean(-1), rstd=(hd.var(-1, unbiased=False) + EPS).rsqrt(), dx=x.grad, dres=h.grad,
                dgamma=t["dg0"].to(dtype) + g.grad, dbeta=t["db0"].to(dtype) + b.grad)


def add_ln_run(K, t, p=0.0, seed=0, counter=None, residual=True, fold_on=None):
    c = {k: v.cuda() for k, v in t.items()}
    res = c["res"] if residual else None
    sd = None if counter is None else torch.tensor([counter], dtype=torch.int64, device="cuda")
    out, mean, rstd = K.add_ln_fwd(c["x"], res, c["g"], c["b"], p_drop=p, seed=seed, seed_dev=sd)
    dg, db = c["dg0"].clone(), c["db0"].clone()
    dx, dres = K.add_ln_bwd(c["dout"], c["x"], res, c["g"], mean, rstd, dg, db, p_drop=p, seed=seed, seed_dev=sd, fold_on=fold_on)
    torch.cuda.synchronize()
    return dict(out=out, mean=mean, rstd=rstd, dx=dx, dres=dres, dgamma=dg, dbeta=db)


ALL7 = ("out", "mean", "rstd", "dx", "dres", "dgamma", "dbeta")


def add_ln_compare(what, got, t, keys=ALL7, **ref_kw):
    r64, r32 = add_ln_ref(t, F64, **ref_kw), add_ln_ref(t, F32, **ref_kw)
    for key in keys:
        check(what, got[key], r64, r32, key)
    return r64


# ------------------------------------------------------------------------- 2. add_ln against float64
# Measured on the MI355X (profiles/norm_tests.txt), margins over all add_ln cases without dropout and the kernels' largest errors:
#   mean   5.0e-9 .. 7.5e-7, err <= 3.0e-8 (0.13 of its margin)      rstd  6.7e-7 .. 1.2e-6, err <= 9.3e-8 (0.09)
#   dgamma 3.5e-6 .. 1.1e-3, err <= 3.7e-5 (0.23)                    dbeta 3.6e-6 .. 1.8e-4, err <= 1.3e-5 (0.07)
#   out / dx / dres: atol 1.8e-6 .. 7.9e-6 beside 2^-8 |ref|, err <= 1.6e-2, up to 0.995 of the bound (2^-8 |ref| is exactly
#   half a bf16 ulp at the bottom of a binade, so a correct rounding comes that close; the sums of atomics move from run to run)
WIDTHS = [8, 504, 512, 520, 768, 1032, 1536, 1544, 2048]


@gpu
@pytest.mark.parametrize("R", [5, 1])
@pytest.mark.parametrize("D", WIDTHS)
def test_add_ln_widths(K, R, D):
    """one live lane (8), 63 lanes (504), lane 0 alone in chunk 1 (520), NCH 3 / 4 off the 512 grid (1032, 1544); R = 5 leaves
    a ragged block of 4 waves, R = 1 three idle waves.  dgamma / dbeta accumulate into a non-zero pre-fill."""
    t = add_ln_inputs(R, D, seed=D)
    got = add_ln_run(K, t)
    assert got["dres"] is got["dx"]                      # p = 0: one gradient for both branches
    add_ln_compare(f"add_ln R={R} D={D}", got, t)


@gpu
@pytest.mark.parametrize("R", [255, 256, 4101, 8200])
def test_add_ln_rows(K, R):
    """255: per-column atomics; 256: first two-stage launch (64 blocks of partials); 4101: 1024 blocks, waves with two rows
    beside waves with one, and the first prefetch of all but five rows runs past the end; 8200: three rows for the first waves."""
    t = add_ln_inputs(R, 64, seed=R)
    add_ln_compare(f"add_ln R={R} D=64", add_ln_run(K, t), t)


@gpu
def test_add_ln_without_residual(K):
    t = add_ln_inputs(37, 520, seed=11)
    got = add_ln_run(K, t, residual=False)
    add_ln_compare("add_ln no residual R=37 D=520", got, t, residual=False)


@gpu
@pytest.mark.parametrize("R", [37, 300])
def test_add_ln_frozen_layernorm(K, R):
    """dgamma = dbeta = None: dx is still right, no scratch is taken and the saved inputs are left alone."""
    D = 520
    t = add_ln_inputs(R, D, seed=12)
    c = {k: v.cuda() for k, v in t.items()}
    out, mean, rstd = K.add_ln_fwd(c["x"], c["res"], c["g"], c["b"])
    saved = {k: v.clone() for k, v in dict(c, mean=mean, rstd=rstd).items()}
    dx, dres = K.add_ln_bwd(c["dout"], c["x"], c["res"], c["g"], mean, rstd, None, None)
    torch.cuda.synchronize()
    add_ln_compare(f"add_ln frozen R={R} D={D}", dict(dx=dx, dres=dres), t, keys=("dx", "dres"))
    for k, v in dict(c, mean=mean, rstd=rstd).items():
        assert torch.equal(v, saved[k]), f"{k} was written"


@gpu
def test_add_ln_without_stats(K):
    t = add_ln_inputs(37, 1032, seed=13)
    c = {k: v.cuda() for k, v in t.items()}
    out, mean, rstd = K.add_ln_fwd(c["x"], c["res"], c["g"], c["b"])
    out2, mean2, rstd2 = K.add_ln_fwd(c["x"], c["res"], c["g"], c["b"], need_stats=False)
    torch.cuda.synchronize()
    assert mean2 is None and rstd2 is None
    assert torch.equal(out, out2)
    r64, r32 = add_ln_ref(t, F64), add_ln_ref(t, F32)
    check("add_ln need_stats=False R=37 D=1032", out2, r64, r32, "out")


@gpu
def test_add_ln_deferred_fold(K):
    """fold_on = a second stream: the partials are folded by vacnic_ln_partial_fold there instead of inside the call."""
    R, D = 4101, 64
    t = add_ln_inputs(R, D, seed=14)
    side = torch.cuda.Stream()
    from vacnic_amd import streams
    streams.release_keep()
    got_in = add_ln_run(K, t)
    assert streams.pending_keep() == 0                           # folded inside the call: nothing went to a side stream
    got_def = add_ln_run(K, t, fold_on=side.cuda_stream)         # add_ln_run synchronises the device
    assert streams.pending_keep() > 0, "the wrapper did not take the deferred path"     # partials / dgamma / dbeta kept for the side stream
    streams.release_keep()
    r64 = add_ln_compare(f"add_ln deferred fold R={R} D={D}", got_def, t)
    r32 = add_ln_ref(t, F32)
    for key in ("dgamma", "dbeta"):
        # two fp32 reductions of the same partials, each within the margin of the exact sum
        # measured: margins 3.7e-4 (dgamma) and 1.8e-4 (dbeta), the two folds 1.5e-5 apart; against float64 the deferred fold is
        # 2.3e-5 (0.06 of its margin) and 1.3e-5 (0.07) off
        d = (got_def[key] - got_in[key]).abs().max().item()
        margin = f32_margin(r64[key], r32[key])
        print(f"NORMCHK deferred-vs-in-call {key} ({D},) bound={margin:.3e} err={d:.3e}")
        assert d <= margin, (key, d, margin)
    for key in ("out", "dx", "mean", "rstd"):
        assert torch.equal(got_def[key], got_in[key]), key


@gpu
def test_add_ln_constant_rows(K):
    """variance exactly 0: rstd = 1 / sqrt(eps) and out = beta (rounded to bf16), whatever gamma is."""
    consts = [1.5, -3.0, 0.25, 100.0, 0.0078125]                  # D * c and every partial sum are exact in fp32
    R, D = len(consts), 520
    t = add_ln_inputs(R, D, seed=15)
    cv = torch.tensor(consts)[:, None].expand(R, D)
    t["x"] = (cv * 0.5).to(BF16).contiguous(); t["res"] = (cv * 0.5).to(BF16).contiguous()
    got = add_ln_run(K, t)
    assert torch.equal(host(got["mean"]), torch.tensor(consts)), got["mean"]
    want = 1.0 / math.sqrt(EPS)
    err = (host(got["rstd"]).to(F64) - want).abs().max().item()
    # fp32 rounding: 2 ulps of 316.2 (2 * 2^-15 = 6.1e-5) cover a 1-ulp reciprocal square root and the rounding of eps itself
    # measured: err 1.7e-5 (about half an ulp)
    bound = 2 * 2.0 ** -15
    print(f"NORMCHK constant rows rstd ({R},) bound={bound:.3e} err={err:.3e}")
    assert err <= bound, (err, want)
    assert torch.equal(host(got["out"]), t["b"].to(BF16)[None, :].expand(R, D)), "out != bf16(beta) on a constant row"


@gpu
def test_add_ln_large_offset_rows(K):
    """rows around 1024 with a spread of 8 (exact in bf16): E[x^2] - E[x]^2 in fp32 loses the variance, two passes keep it."""
    R, D = 6, 512
    t = add_ln_inputs(R, D, seed=16)
    g = torch.Generator().manual_seed(16)
    t["x"] = (1024.0 + 8.0 * torch.randint(-1, 2, (R, D), generator=g)).to(BF16)          # 1016, 1024, 1032
    t["res"] = (torch.randint(0, 2, (R, D), generator=g) * 2.0 - 1.0).to(BF16)            # +-1: the sum is exact in fp32
    assert set(t["x"].float().unique().tolist()) == {1016.0, 1024.0, 1032.0}
    add_ln_compare(f"add_ln offset 1024 R={R} D={D}", add_ln_run(K, t), t)


def _raw_add_ln_fwd(K, D, out, x, g, b, R=5):
    from vacnic_amd._lib import call_struct
    call_struct("vacnic_add_ln_fwd", stream=K._stream(), x=x.data_ptr(), residual=None, gamma=g.data_ptr(), beta=b.data_ptr(),
                out=out.data_ptr(), mean=None, rstd=None, R=R, D=D, eps=1e-5, p_drop=0.0, seed=0, seed_dev=None)


@gpu
@pytest.mark.parametrize("D", [0, 12, 2056])
def test_add_ln_refuses_bad_width(K, D):
    R = 5
    x = torch.ones(R, 2056, device="cuda", dtype=BF16); g = torch.ones(2056, device="cuda"); b = torch.zeros(2056, device="cuda")
    out = torch.full((R, 2056), 7.0, device="cuda", dtype=BF16)
    with pytest.raises(ValueError, match="multiple of 8"):
        _raw_add_ln_fwd(K, D, out, x, g, b)
    torch.cuda.synchronize()
    assert (out == 7.0).all(), "a refused call wrote its output"
    mean = torch.zeros(R, device="cuda"); dg = torch.zeros(2056, device="cuda")
    xs = x[:, :D].contiguous()
    why = "multiple of 8" if D else "null operand"              # an empty tensor has no address: refused before check_d
    with pytest.raises(ValueError, match=why):
        K.add_ln_fwd(xs, None, g, b)
    with pytest.raises(ValueError, match=why):
        K.add_ln_bwd(xs, xs, None, g, mean, mean, dg, dg)
    torch.cuda.synchronize()
    assert (dg == 0).all()


# ------------------------------------------------------------------------- 3. hidden dropout, exact
def read_mask(got):
    """keep bit off the backward: dx = keep * inv_keep * dh beside dresidual = dh.  Returns (keep, comparable)."""
    dx, dres = host(got["dx"]).float().numpy(), host(got["dres"]).float().numpy()
    return dx != 0, dres != 0


def assert_mask(what, got, want, max_left_out=1e-3):
    keep, ok = read_mask(got)
    left = 1.0 - ok.mean()
    bad = ((keep != want) & ok).sum()
    print(f"NORMCHK {what} mask {want.shape} mismatches={bad} left_out={left:.2e} keep_rate={want.mean():.4f}")
    assert left <= max_left_out, f"{what}: {left:.3%} of the positions have dresidual == 0"
    assert bad == 0, f"{what}: {bad} keep bits differ from the host Philox mask"


@gpu
@pytest.mark.parametrize("R,D", [(37, 520), (37, 768), (37, 1024), (37, 1544), (37, 2048), (4101, 64)])
def test_add_ln_dropout_exact(K, R, D):
    p = 0.1
    thr = drop_threshold(p)
    t = add_ln_inputs(R, D, seed=100 + D)
    want = hidden_keep(R, D, SEED, thr)
    got = add_ln_run(K, t, p=p, seed=SEED)
    assert got["dres"] is not got["dx"]
    assert_mask(f"add_ln dropout R={R} D={D}", got, want)               # measured: 0 mismatches, nothing left out
    # measured: mean margin 8.3e-8 .. 6.7e-7, err <= 7.4e-8 (0.16 of it); rstd err <= 8.6e-8 (0.11); dgamma margin
    # 2.5e-5 .. 5.5e-4, err <= 2.3e-5 (0.14); dbeta err <= 1.1e-5 (0.06); out / dx / dres up to 0.995 of their bound.  inv_keep = 1/(1-p) is 1.9e-3 larger: rstd moves by ~1e-3.
    r64 = add_ln_compare(f"add_ln dropout R={R} D={D}", got, t, keep=want, inv_keep=inv_keep_of(thr))
    assert (r64["dres"] != 0).all()                      # the reference leaves no position out of the mask comparison


@gpu
@pytest.mark.parametrize("counter", [0, 1, (1 << 40) + 3])
def test_add_ln_dropout_device_counter(K, counter):
    R, D, thr = 37, 1544, drop_threshold(0.1)
    t = add_ln_inputs(R, D, seed=7)
    want = hidden_keep(R, D, mix_seed(SEED, counter), thr)
    got = add_ln_run(K, t, p=0.1, seed=SEED, counter=counter)
    assert_mask(f"add_ln seed_dev={counter}", got, want)
    if counter:
        assert not np.array_equal(want, hidden_keep(R, D, SEED, thr))
    add_ln_compare(f"add_ln seed_dev={counter} R={R} D={D}", got, t, keys=("out", "dgamma"), keep=want, inv_keep=inv_keep_of(thr))


@gpu
def test_add_ln_dropout_threshold_zero_is_identity(K):
    t = add_ln_inputs(37, 1032, seed=8)
    a, b = add_ln_run(K, t, p=0.0), add_ln_run(K, t, p=0.001, seed=SEED)
    for key in ("out", "mean", "rstd", "dx", "dres"):
        assert torch.equal(a[key], b[key]), f"p = 0.001 (threshold 0) changed {key}"
    # dgamma / dbeta are sums of fp32 atomics in arrival order: the same terms, held to the float64 reference of p = 0
    # measured: margin 2.1e-5 for both; dgamma err 3.2e-6 (0.15 of it), dbeta err 9.5e-7 (0.05)
    add_ln_compare("add_ln p=0.001 R=37 D=1032", b, t, keys=("dgamma", "dbeta"))


@gpu
def test_add_ln_dropout_threshold_cap(K):
    R, D = 261, 2048
    t = add_ln_inputs(R, D, seed=9)
    want = hidden_keep(R, D, SEED, 255)
    got = add_ln_run(K, t, p=0.999, seed=SEED)
    assert_mask("add_ln p=0.999", got, want)
    keep, ok = read_mask(got)
    rate = keep[ok].mean()
    assert abs(rate - 1 / 256) < 0.01, rate
    dx, dres = host(got["dx"]).float(), host(got["dres"]).float()
    sel = torch.from_numpy(keep)
    assert torch.equal(dx[sel], dres[sel] * 256.0), "kept gradients are not scaled by exactly 256"     # a power of two: exact in bf16
    add_ln_compare(f"add_ln p=0.999 R={R} D={D}", got, t, keep=want, inv_keep=256.0)


# ---------------------------------------------------------------------- 4. embed_ln / name_embed_mean
PAD = 1


def embed_inputs(B, T, V, D, off, seed):
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (B, T), generator=gen)
    ids[0, -5:] = PAD; ids[1, 3] = -1; ids[2, 7] = V + 5; ids[B - 1, T - 1] = V + 5; ids[0, 0] = -1
    return dict(ids=ids, emb=cpu_randn(V, D, seed=seed + 1, scale=0.5), pos=cpu_randn(T + off, D, seed=seed + 2, scale=0.5),
                dout=cpu_randn(B, T, D, seed=seed + 5), g=cpu_randn(D, seed=seed + 3, dtype=F32) * 0.3 + 1.0,
                b=cpu_randn(D, seed=seed + 4, dtype=F32) * 0.5, de0=cpu_randn(V, D, seed=seed + 6, dtype=F32) + 3.0,
                dp0=cpu_randn(T + off, D, seed=seed + 7, dtype=F32) - 2.0, dg0=cpu_randn(D, seed=seed + 8, dtype=F32) + 1.0,
                db0=cpu_randn(D, seed=seed + 9, dtype=F32) - 1.0)


def embed_ref(t, scale, off, dtype, keep=None, inv_keep=1.0):
    ids = t["ids"]; B, T = ids.shape; V, D = t["emb"].shape
    emb = leaf(t["emb"], dtype); pos = leaf(t["pos"], dtype)
    g = leaf(t["g"], dtype); b = leaf(t["b"], dtype)
    e = emb[ids.clamp(0, V - 1)]                                          # -1 -> 0, V + 5 -> V - 1
    e = torch.where((ids == PAD)[..., None], e.detach(), e)               # the padding row takes no gradient
    h = e * scale + pos[off:off + T][None]
    out = F.layer_norm(h, (D,), g, b, EPS)
    if keep is not None:
        out = out * (torch.from_numpy(keep).reshape(B, T, D).to(dtype) * inv_keep)
    out.backward(t["dout"].to(dtype))
    hd = h.detach().reshape(B * T, D)
    return dict(out=out.detach(), mean=hd.mean(-1), rstd=(hd.var(-1, unbiased=False) + EPS).rsqrt(), demb=t["de0"].to(dtype) + emb.grad,
                dpos=t["dp0"].to(dtype) + pos.grad, dgamma=t["dg0"].to(dtype) + g.grad, dbeta=t["db0"].to(dtype) + b.grad)


def embed_run(K, t, scale, off, p=0.0, seed=0):
    c = {k: v.cuda() for k, v in t.items()}
    out, mean, rstd = K.embed_ln_fwd(c["ids"], c["emb"], c["pos"], c["g"], c["b"], embed_scale=scale, pos_offset=off, p_drop=p, seed=seed)
    de, dp, dg, db = c["de0"].clone(), c["dp0"].clone(), c["dg0"].clone(), c["db0"].clone()
    K.embed_ln_bwd(c["ids"], c["emb"], c["pos"], c["dout"], c["g"], mean, rstd, de, dp, dg, db, embed_scale=scale, pos_offset=off,
                   padding_idx=PAD, p_drop=p, seed=seed)
    torch.cuda.synchronize()
    return dict(out=out, mean=mean, rstd=rstd, demb=de, dpos=dp, dgamma=dg, dbeta=db)


def bf16_ulp(v):
    """spacing of bf16 (8 significant bits) at |v|."""
    _, e = torch.frexp(v)                                     # |v| in [2^(e-1), 2^e)
    return torch.ldexp(torch.ones_like(v), e - 8)


@gpu
@pytest.mark.parametrize("off", [0, 2])
@pytest.mark.parametrize("D,B,T,V", [(8, 3, 40, 50), (520, 3, 40, 50), (768, 3, 40, 50), (1032, 3, 40, 50), (64, 3, 1400, 7)])
def test_embed_ln(K, D, B, T, V, off):
    """embed_scale = sqrt(D), ids -1 and V + 5 clamp to 0 and V - 1, the padding row's gradient stays at its pre-fill, all four
    gradients accumulate; (64, 3 x 1400, 7) walks the grid-stride loop (R = 4200) with 600 colliding rows per embedding row."""
    scale = float(np.float32(math.sqrt(D)))
    t = embed_inputs(B, T, V, D, off, seed=D + off)
    what = f"embed_ln D={D} R={B * T} V={V} off={off}"
    got = embed_run(K, t, scale, off)
    r64, r32 = embed_ref(t, scale, off, F64), embed_ref(t, scale, off, F32)
    # measured over the ten cases, p = 0 and 0.1: demb margin 2.0e-5 .. 9.9e-4, err <= 1.7e-4 (0.18 of its margin); dpos margin
    # 5.8e-6 .. 9.1e-6, err <= 7.2e-7 (0.11); dgamma margin 1.4e-5 .. 6.4e-4, err <= 2.8e-4 (0.43); dbeta margin 2.0e-5 .. 4.1e-4,
    # err <= 2.3e-4 (0.63, the largest share of an fp32 margin in this file: 4200 rows of atomics); mean / rstd err <= 1.7e-7 (0.13)
    for key in ("out", "mean", "rstd", "demb", "dpos", "dgamma", "dbeta"):
        check(what, got[key], r64, r32, key)
    assert torch.equal(host(got["demb"])[PAD], t["de0"][PAD]), "demb[padding_idx] moved"
    # the clamped ids are ids 0 and V - 1
    t2 = dict(t, ids=t["ids"].clamp(0, V - 1))
    got2 = embed_run(K, t2, scale, off)
    assert torch.equal(got2["out"], got["out"]) and torch.equal(got2["mean"], got["mean"])

    # p = 0.1: the forward drops after the LayerNorm, the backward masks dout
    thr = drop_threshold(0.1); inv = inv_keep_of(thr)
    keep = hidden_keep(B * T, D, SEED, thr)
    gp = embed_run(K, t, scale, off, p=0.1, seed=SEED)
    out0, outp = host(got["out"]).float().reshape(B * T, D), host(gp["out"]).float().reshape(B * T, D)
    kt = torch.from_numpy(keep)
    assert (outp[~kt] == 0).all(), "a dropped element is not exactly 0"
    # "within one bf16 ulp" is taken between bf16 numbers: out_p against out_0 * inv_keep rounded to bf16.  Against the unrounded
    # product no kernel can promise it: out_0 carries half an ulp of its own, which inv_keep stretches, and out_p rounds once
    # more, 0.5 + 0.5 * 256/230 = 1.06 ulp in the worst case (an fp32 torch model of the kernel reaches 1.05).  The float64
    # comparison of out_p below is the check that holds the unrounded value to one rounding.
    want = (out0 * inv).to(BF16).float()
    err = (outp - want).abs()[kt]; ulp = torch.maximum(bf16_ulp(want), bf16_ulp(outp))[kt]
    print(f"NORMCHK {what} p=0.1 out_p vs bf16(out_0*inv_keep): max err/ulp={(err / ulp).max().item():.3f} keep_rate={keep.mean():.4f}")
    assert (err <= ulp).all(), "a kept element is more than one bf16 ulp from out_0 * 256/230"
    assert ((outp != 0) == (out0 != 0))[kt].all(), "a kept element was zeroed"
    assert torch.equal(gp["mean"], got["mean"]) and torch.equal(gp["rstd"], got["rstd"])
    p64, p32 = embed_ref(t, scale, off, F64, keep, inv), embed_ref(t, scale, off, F32, keep, inv)
    for key in ("out", "demb", "dpos", "dgamma", "dbeta"):
        check(what + " p=0.1", gp[key], p64, p32, key)
    assert torch.equal(host(gp["demb"])[PAD], t["de0"][PAD])


@gpu
def test_embed_ln_refuses_bad_width(K):
    t = embed_inputs(3, 40, 50, 12, 2, seed=1)
    c = {k: v.cuda() for k, v in t.items()}
    with pytest.raises(ValueError, match="multiple of 8"):
        K.embed_ln_fwd(c["ids"], c["emb"], c["pos"], c["g"], c["b"])
    with pytest.raises(ValueError, match="multiple of 8"):
        K.name_embed_mean(c["ids"][:, None, :8].contiguous(), c["emb"], c["pos"], c["g"], c["b"])


@gpu
@pytest.mark.parametrize("shape", [(2, 5, 8), (1, 1, 1)])
@pytest.mark.parametrize("D", [8, 520, 1024])
def test_name_embed_mean(K, D, shape):
    B, Nn, Ln = shape
    V, off = 30, 2
    scale = float(np.float32(math.sqrt(D)))
    ids = torch.randint(0, V, shape, generator=torch.Generator().manual_seed(D))
    ids[-1, -1, -1] = V + 9                                                # clamps to V - 1
    if Ln > 1:
        ids[0, 0, 0] = -4                                                  # clamps to 0
    emb = cpu_randn(V, D, seed=1, scale=0.5); pos = cpu_randn(Ln + off, D, seed=2, scale=0.5)
    g = cpu_randn(D, seed=3, dtype=F32) * 0.3 + 1.0; b = cpu_randn(D, seed=4, dtype=F32) * 0.5
    out = K.name_embed_mean(ids.cuda(), emb.cuda(), pos.cuda(), g.cuda(), b.cuda(), embed_scale=scale, pos_offset=off)
    torch.cuda.synchronize()

    def ref(dtype):
        h = emb.to(dtype)[ids.clamp(0, V - 1)] * scale + pos.to(dtype)[off:off + Ln][None, None]
        return dict(name_embed=F.layer_norm(h, (D,), g.to(dtype), b.to(dtype), EPS).mean(2))
    # measured: margin 1.5e-6 .. 5.2e-6, err <= 8.8e-7 (0.17 of its margin)
    check(f"name_embed_mean D={D} shape={shape}", out, ref(F64), ref(F32), "name_embed")


# ------------------------------------------------------------------------- 5. flat activation dropout
@gpu
@pytest.mark.parametrize("counter", [None, (1 << 40) + 3])
@pytest.mark.parametrize("n", [8, 16, 24, 4104])
def test_flat_dropout(K, n, counter):
    """n % 16 == 8: the last Philox block serves one chunk of 8.  p = 0.2 -> threshold 51, kept values 256 / 205."""
    thr = drop_threshold(0.2)
    assert thr == 51
    sd = None if counter is None else torch.tensor([counter], dtype=torch.int64, device="cuda")
    buf = torch.ones(n + 16, device="cuda", dtype=BF16)                     # 16 guard elements behind the array
    x = buf[:n]
    K.dropout_(x, 0.2, SEED, sd)
    torch.cuda.synchronize()
    want = flat_keep(n, SEED if counter is None else mix_seed(SEED, counter), thr)
    got = host(x).float()
    assert np.array_equal((got != 0).numpy(), want), "flat keep mask differs from the host Philox mask"
    kept = torch.tensor(256.0 / 205.0).to(BF16).float()
    assert (got[torch.from_numpy(want)] == kept).all()
    assert (host(buf[n:]) == 1).all(), "wrote past the end of the array"
    # a second tensor through the same mask: scaled where kept, in place
    y = cpu_randn(n, seed=n)
    z = K.dropout_(y.cuda(), 0.2, SEED, sd)
    ref = torch.where(torch.from_numpy(want), y.float() * float(np.float32(256.0) / np.float32(205.0)), torch.zeros(n)).to(BF16)
    assert torch.equal(host(z), ref)


@gpu
def test_flat_dropout_refusals(K):
    x = torch.ones(32, device="cuda", dtype=BF16)
    with pytest.raises(ValueError):
        K.dropout_(x[:12], 0.2, SEED)
    for p in (0.0, 1.0):
        with pytest.raises(ValueError):
            K.dropout_(x, p, SEED)
    torch.cuda.synchronize()
    assert (x == 1).all()
