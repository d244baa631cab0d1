"""Data-movement kernels (csrc/misc.hip, the casts of csrc/optim.hip): every path edge against host models on the CPU.

Margins (none is taken from a kernel's output):
  * exact outputs (copies, masks, ids, arg-max, casts, bf16 add / copy3d(accumulate), vit_assemble, im2col, bias_grad on integer
    data): torch.equal.  The inputs are chosen so that exactness is owed: small integers, or multiples of 2^-6 in [-4, 4]
    (at most 9 significant bits: exact in bf16 up to 256/64, and every fp32 sum of two of them is exact), so a bf16 result is
    ONE rounding (to nearest even) of an exact fp32 intermediate and the float64 reference rounded once must match bit for bit.
  * fp32 outputs on random data (dbias): the same sum is evaluated in fp32 on the CPU; the kernel may deviate from float64 by 8x
    the largest fp32 deviation at that shape (a different but legitimate summation order: four row groups, atomics), floored at
    1e-6 * max|ref|.
  * arg-max decisions: the data are integers (and +-inf), so every comparison is exact and "lowest index wins" is owed.
The unmarked tests check the host models against torch and show, for every value check, that a deliberately wrong model (pad
columns included, last column dropped, pos offset by one row, cls row omitted, tie routed to the last index, ...) differs from the
true reference on the very inputs the GPU test uses; the margin of an exact check is zero, so any difference is caught.
Every check prints `MISCCHK <what> <shape> bound=<margin> err=<observed>`; profiles/loss_misc_tests.txt holds one run of them.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
CAP = 4096 * 256                      # grid_for's cap: more work items than this walk the grid-stride loop


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


def host(t):
    return None if t is None else t.detach().to("cpu")


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def q64(*shape, seed, dtype=BF16):
    """multiples of 2^-6 in [-4, 4]."""
    return (torch.randint(-256, 257, shape, generator=gen(seed)).to(F32) / 64.0).to(dtype)


def ints(lo, hi, shape, seed, dtype=BF16):
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).to(dtype)


def check_equal(what, got, want):
    got, want = host(got), host(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} != {want.shape} {want.dtype}"
    ne = (got != want)
    diff = (got.to(F64) - want.to(F64)).abs()
    diff = torch.nan_to_num(diff, nan=float("inf"))[ne].max().item() if ne.any() else 0.0
    print(f"MISCCHK {what} {tuple(want.shape)} bound=0.000e+00 err={diff:.3e}")
    assert torch.equal(got, want), f"{what}: {int(ne.sum())}/{want.numel()} elements differ (max diff {diff})"


def assert_differs(what, ref, mutant):
    assert ref.shape == mutant.shape and not torch.equal(ref, mutant), f"{what}: the mutant equals the reference"


def round_up(v, m):
    return (v + m - 1) // m * m


# ------------------------------------------------------------------------------------------- host models
def bf16_rne_bits(f32_bits):
    """round-to-nearest-even of fp32 bit patterns (finite values) to bf16 bit patterns, on uint32 numpy arrays."""
    b = f32_bits.astype(np.uint64)
    return (((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint16)


def prep_ids_model(ids, pad, start):
    """mask = ids != pad; shifted[b][0] = start, shifted[b][t] = ids[b][t - 1]; a -100 in shifted becomes pad (misc.hip)."""
    mask = (ids != pad).to(torch.uint8)
    sh = torch.cat([torch.full_like(ids[:, :1], start), ids[:, :-1]], 1)
    return mask, torch.where(sh == -100, torch.full_like(sh, pad), sh)


def vit_assemble_model(pe, cls, pos, B, G2, W, pos_shift=0, drop_cls=False):
    """x[b][0] = cls + pos[0]; x[b][1 + i] = patch_emb[b * G2 + i] + pos[1 + i], in float64, rounded once to bf16."""
    x = torch.cat([cls.to(F64)[None, None].expand(B, 1, W), pe.to(F64).reshape(B, G2, W)], 1)
    if drop_cls:
        x = torch.cat([x[:, 1:2], x[:, 1:]], 1)
    p = pos.to(F64)[:G2 + 1]
    return (x + torch.roll(p, pos_shift, 0)[None]).to(BF16)


def im2col_model(img, p, Kp, swap=False):
    """patches[(b g + gy) g + gx][c p p + py p + px] = img[b][c][gy p + py][gx p + px], zero up to Kp, rounded once to bf16."""
    B, _, HW, _ = img.shape
    g = HW // p
    x = img.reshape(B, 3, g, p, g, p)                              # b c gy py gx px
    x = x.permute(0, 2, 4, 1, 5, 3) if swap else x.permute(0, 2, 4, 1, 3, 5)
    return F.pad(x.reshape(B * g * g, 3 * p * p), (0, Kp - 3 * p * p)).to(BF16)


def pad_cols_model(x2d, Cp):
    return F.pad(x2d, (0, Cp - x2d.shape[1]))


def argmax_model(x, last=False):
    a = x.to(F64).numpy()
    if last:
        return torch.from_numpy(a.shape[1] - 1 - np.flip(a, 1).argmax(1))
    return torch.from_numpy(a.argmax(1))                           # numpy: the first occurrence of the maximum


# ------------------------------------------------------------------------------------------------- cases
ARGMAX_V = [1, 255, 256, 257, 1000, 50267]
PAD_VAL = 1000.0
_CASES = {}


def cached(fn):
    def wrap(*a):
        key = (fn.__name__,) + a
        if key not in _CASES:
            _CASES[key] = fn(*a)
        return _CASES[key]
    return wrap


@cached
def argmax_case(V, f32):
    """integers in [-50, 50] (ties everywhere), the maximum 100 planted: in one thread's stride (j, j + 256), in neighbouring
    threads, on both sides of every reduction half (t, t + 128), (t, t + 64), ..., (0, 1); a row of -inf; one with a single
    finite value at the end.  The padding behind V holds 1000."""
    R = 12
    ldl = V + 5
    buf = torch.full((R, ldl), PAD_VAL, dtype=F32)
    x = ints(-50, 50, (R, V), seed=V, dtype=F32)
    plants = [(300, 44), (45, 44, 46), (200, 72), (67, 3), (33, 1), (17, 1), (9, 1), (5, 1), (3, 1), (1, 0)]
    for r, cols in enumerate(plants):
        cols = [c for c in cols if c < V]
        if len(cols) > 1:
            x[r, cols] = 100.0
    x[10] = float("-inf")
    x[11] = float("-inf"); x[11, V - 1] = -7.0
    buf[:, :V] = x
    return dict(buf=buf.to(F32 if f32 else BF16), x=x, want=argmax_model(x))


BIAS_M, BIAS_N = [1, 3, 4, 5, 33, 65, 300], [8, 512, 513, 520]


@cached
def bias_case(M, N, integer):
    ldy = round_up(N, 8) + 8
    dy = torch.full((M, ldy), 64.0, dtype=BF16)                    # the padding must stay out of the sums
    dy[:, :N] = ints(-3, 3, (M, N), seed=M * 1000 + N) if integer else (torch.randn(M, N, generator=gen(M * 1000 + N + 1))).to(BF16)
    db0 = ints(-5, 5, (N,), seed=N, dtype=F32) if integer else torch.randn(N, generator=gen(N))
    r64 = db0.to(F64) + dy[:, :N].to(F64).sum(0)
    r32 = db0 + dy[:, :N].to(F32).sum(0)
    return dict(dy=dy, db0=db0, r64=r64, r32=r32)


# ---------------------------------------------------------------------------------- unmarked: host models
def test_bf16_rounding_model_is_torch():
    bits = np.concatenate([np.arange(0, 1 << 16, dtype=np.uint32) << 16 | 0x8000,           # every exact tie
                           torch.randint(0, 1 << 31, (4096,), generator=gen(0)).numpy().astype(np.uint32)])
    bits = bits[(bits & 0x7F800000) != 0x7F800000]                                            # finite
    x = torch.from_numpy(bits.view(np.int32)).view(F32)
    want = x.to(BF16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(bf16_rne_bits(bits), want)
    trunc = (bits >> 16).astype(np.uint16)
    assert not np.array_equal(trunc, want)                                                   # mutant: truncation


def test_host_models_against_torch():
    img = torch.randn(3, 3, 28, 28, generator=gen(1))
    ref = F.unfold(img, 14, stride=14).transpose(1, 2).reshape(3 * 4, 588)
    assert torch.equal(im2col_model(img, 14, 592)[:, :588], ref.to(BF16)) and (im2col_model(img, 14, 592)[:, 588:] == 0).all()
    assert_differs("im2col py / px swapped", im2col_model(img, 14, 592), im2col_model(img, 14, 592, swap=True))
    ids = torch.tensor([[0, 5, -100, 2, 1], [0, 9, 2, 1, -100]])
    mask, sh = prep_ids_model(ids, 1, 2)
    assert mask.tolist() == [[1, 1, 1, 1, 0], [1, 1, 1, 0, 1]] and sh.tolist() == [[2, 0, 5, 1, 2], [2, 0, 9, 2, 1]]
    x = torch.tensor([[1.0, 5.0, 5.0, 2.0], [3.0, 3.0, 3.0, 3.0]])
    assert argmax_model(x).tolist() == [1, 0] and argmax_model(x, last=True).tolist() == [2, 3]
    assert torch.equal(argmax_model(x), x.argmax(1))


@pytest.mark.parametrize("B,G2,W", [(1, 1, 8), (2, 4, 72), (3, 49, 768)])
def test_vit_assemble_mutants_differ(B, G2, W):
    pe, cls, pos = q64(B * G2, W, seed=1), q64(W, seed=2), q64(G2 + 1, W, seed=3)
    ref = vit_assemble_model(pe, cls, pos, B, G2, W)
    exact = torch.cat([cls.float()[None, None].expand(B, 1, W), pe.float().reshape(B, G2, W)], 1) + pos.float()[None]
    assert torch.equal(ref, exact.to(BF16)), "the fp32 sum of these inputs is exact: one rounding either way"
    assert_differs("pos offset by one row", ref, vit_assemble_model(pe, cls, pos, B, G2, W, pos_shift=1))
    assert_differs("cls row omitted", ref, vit_assemble_model(pe, cls, pos, B, G2, W, drop_cls=True))


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("V", ARGMAX_V)
def test_argmax_cases_hold_ties(V, f32):
    c = argmax_case(V, f32)
    assert torch.equal(c["buf"][:, :V].to(F32), c["x"]), "the data are not exact in this dtype"
    assert c["want"][10].item() == 0 and c["want"][11].item() == V - 1
    if V >= 255:
        assert c["want"][1:10].tolist() == [44, 72, 3, 1, 1, 1, 1, 1, 0] and (V < 1000 or c["want"][0].item() == 44)
        assert_differs("tie routed to the last index", c["want"], argmax_model(c["x"], last=True))
        assert_differs("pad columns included", c["want"], argmax_model(c["buf"].to(F32)))
    if V > 1:
        assert_differs("last column dropped", c["want"], argmax_model(c["x"][:, :V - 1]))


def test_bias_grad_mutants_differ():
    for N in BIAS_N:
        c = bias_case(300, N, True)
        dy = c["dy"].to(F64)
        assert torch.equal(c["r64"], c["r32"].to(F64)), "integer sums must be exact in fp32"
        assert_differs("last row dropped", c["r64"], c["db0"].to(F64) + dy[:-1, :N].sum(0))
        assert_differs("dbias overwritten", c["r64"], dy[:, :N].sum(0))
        shifted = c["db0"].to(F64) + dy[:, 1:N + 1].sum(0)
        assert_differs("pad column read", c["r64"], shifted)
        r = bias_case(300, N, False)
        margin = max(8 * (r["r32"].to(F64) - r["r64"]).abs().max().item(), 1e-6 * r["r64"].abs().max().item())
        mut = r["db0"].to(F64) + r["dy"].to(F64)[:-1, :N].sum(0)
        assert ((mut - r["r64"]).abs() >= 10 * margin).any()


def test_copy_mutants_differ():
    big = q64(5, 588 + 7, seed=588)
    ref = pad_cols_model(big[:, 3:3 + 588], 592)
    assert_differs("pad columns included", ref, big[:, 3:3 + 592])
    assert_differs("last column dropped", ref, F.pad(big[:, 3:3 + 587], (0, 5)))
    a = torch.randint(0, 2, (4, 3), generator=gen(1), dtype=torch.uint8); b = torch.randint(0, 2, (4, 5), generator=gen(2), dtype=torch.uint8)
    assert_differs("masks row-major instead of side by side", torch.cat([a, b], 1), torch.cat([a.reshape(-1), b.reshape(-1)]).reshape(4, 8))
    parts = [q64(3, t, 72, seed=t) for t in (5, 1, 9)]
    assert_differs("parts in the wrong order", torch.cat(parts, 1), torch.cat(parts[::-1], 1))


def test_exact_inputs_are_exact():
    a, b = q64(4096, seed=1), q64(4096, seed=2)
    assert torch.equal(a.to(F64) * 64, (a.to(F64) * 64).round()) and a.abs().max() <= 4
    s = a.float() + b.float()
    assert torch.equal(s.to(F64), a.to(F64) + b.to(F64)), "the fp32 intermediate is exact"
    assert not torch.equal(s.to(BF16).float(), s), "some sums need the rounding"
    assert_differs("accumulate overwrites", s.to(BF16), b)


# ------------------------------------------------------------------------------------------- GPU: copies
@gpu
@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("B,rows,cols", [(3, 5, 8), (2, 7, 72), (2, 1030, 4096)])
def test_copy3d(K, B, rows, cols, acc):
    """strided source and destination views (a window of a larger tensor), cols = 8, and B * rows * cols / 8 above the 4096 * 256
    cap (the grid-stride loop); everything outside the window keeps its value."""
    assert (B, rows, cols) != (2, 1030, 4096) or B * rows * cols // 8 > CAP
    src_big = q64(B, rows + 3, cols + 16, seed=rows)
    dst_big = q64(B, rows + 5, cols + 24, seed=rows + 1)
    s, d = src_big.cuda(), dst_big.cuda()
    K.copy3d(s[:, 2:2 + rows, 8:8 + cols], d[:, 1:1 + rows, 16:16 + cols], B, rows, cols, accumulate=acc)
    torch.cuda.synchronize()
    want = dst_big.clone()
    win = src_big[:, 2:2 + rows, 8:8 + cols]
    want[:, 1:1 + rows, 16:16 + cols] = (want[:, 1:1 + rows, 16:16 + cols].float() + win.float()).to(BF16) if acc else win
    check_equal(f"copy3d B={B} rows={rows} cols={cols} accumulate={acc}", d, want)
    check_equal("copy3d source untouched", s, src_big)


@gpu
def test_copy3d_refuses_ragged_columns(K):
    s = torch.ones(1, 4, 16, device="cuda", dtype=BF16); d = torch.zeros(1, 4, 16, device="cuda", dtype=BF16)
    with pytest.raises(ValueError, match="multiples of 8"):
        K.copy3d(s, d, 1, 4, 12)
    with pytest.raises(ValueError, match="multiples of 8"):
        K.copy3d(s[:, :, 4:], d, 1, 4, 8)                     # base 8 bytes off
    torch.cuda.synchronize()
    assert (d == 0).all()


@gpu
def test_cat_tokens_and_zero_strided(K):
    parts = [q64(3, t, 72, seed=t) for t in (5, 1, 9)]
    check_equal("cat_tokens three parts", K.cat_tokens([p.cuda() for p in parts]), torch.cat(parts, 1))
    big = q64(3, 9, 40, seed=4)
    d = big.cuda()
    K.zero_strided(d[:, 2:6, 8:32])
    torch.cuda.synchronize()
    want = big.clone(); want[:, 2:6, 8:32] = 0
    check_equal("zero_strided", d, want)


@gpu
@pytest.mark.parametrize("n8", [1, 300, CAP + 3])
def test_add(K, n8):
    a, b = q64(n8 * 8, seed=1), q64(n8 * 8, seed=2)
    check_equal(f"add n={n8 * 8}", K.add(a.cuda(), b.cuda()), (a.float() + b.float()).to(BF16))


@gpu
@pytest.mark.parametrize("R,C,Cp", [(5, 1, 8), (5, 588, 592), (5, 588, 588), (2000, 588, 592)])
def test_pad_cols(K, R, C, Cp):
    """a strided source (a column window of a wider tensor whose neighbours are non-zero), Cp == C, R * Cp above the cap."""
    assert R != 2000 or R * Cp > CAP
    big = q64(R, C + 7, seed=C)
    assert (big[:, 3 + C:] != 0).any()
    check_equal(f"pad_cols R={R} C={C} Cp={Cp}", K.pad_cols(big.cuda()[:, 3:3 + C], Cp), pad_cols_model(big[:, 3:3 + C], Cp))


@gpu
@pytest.mark.parametrize("na,nb", [(3, 5), (0, 5), (3, 0), (300, 1)])
def test_cat_masks(K, na, nb):
    B = 4
    a = torch.randint(0, 2, (B, na), generator=gen(1), dtype=torch.uint8); b = torch.randint(0, 2, (B, nb), generator=gen(2), dtype=torch.uint8)
    check_equal(f"cat_masks na={na} nb={nb}", K.cat_masks(a.cuda(), b.cuda()), torch.cat([a, b], 1))


@gpu
def test_casts(K):
    """every fp32 value halfway between two bf16 neighbours rounds to the even one; bf16 -> fp32 -> bf16 is the identity."""
    bits = np.concatenate([np.arange(0, 1 << 16, dtype=np.uint32) << 16 | 0x8000,
                           torch.randint(0, 1 << 31, (4099,), generator=gen(0)).numpy().astype(np.uint32)])
    bits = bits[(bits & 0x7F800000) != 0x7F800000]                        # finite
    bits = bits[:bits.size - (bits.size - 3) % 4]                         # n % 4 == 3: the scalar tail of the cast
    assert bits.size % 4 == 3
    x = torch.from_numpy(bits.view(np.int32)).view(F32)
    want = torch.from_numpy(bf16_rne_bits(bits).view(np.int16)).view(BF16)
    got = K.cast_f32_bf16(x.cuda())
    check_equal("cast_f32_bf16 ties to even (bit patterns)", got.view(torch.int16), want.view(torch.int16))
    allb = np.arange(0, 1 << 16, dtype=np.uint32)
    allb = allb[(allb & 0x7F80) != 0x7F80].astype(np.uint16)             # every finite bf16
    h = torch.from_numpy(allb.view(np.int16)).view(BF16)
    f = K.cast_bf16_f32(h.cuda())
    check_equal("cast_bf16_f32 (bit patterns)", f.view(torch.int32), torch.from_numpy((allb.astype(np.uint32) << 16).view(np.int32)))
    check_equal("cast round trip", K.cast_f32_bf16(f).view(torch.int16), h.view(torch.int16))


@gpu
@pytest.mark.parametrize("dtype,n", [(F32, 1000), (BF16, 1001), (BF16, 8)])
def test_zero(K, dtype, n):
    buf = torch.full((n + 9,), 3.0, device="cuda", dtype=dtype)
    K.zero_(buf[:n])
    torch.cuda.synchronize()
    want = torch.full((n + 9,), 3.0, dtype=dtype); want[:n] = 0
    check_equal(f"zero_ {dtype} n={n}", buf, want)


@gpu
def test_face_mask(K):
    B, Fn, D = 65, 5, 24                                            # B * F = 325 > 256: two blocks
    faces = torch.randn(B, Fn, D, generator=gen(3))
    pad = torch.rand(B, Fn, generator=gen(4)) < 0.4
    faces[pad] = 1.0                                                # padded faces are rows of ones
    faces[0, 0, :-1] = 1.0; faces[0, 1, 0] = 1.0                    # only the last element decides
    want = (faces[..., -1] != 1.0).to(torch.uint8)
    assert_differs("first element tested", want, (faces[..., 0] != 1.0).to(torch.uint8))
    check_equal("face_mask BF=325", K.face_mask(faces.cuda()), want)


# ------------------------------------------------------------------------------------------ GPU: prep_ids
@gpu
@pytest.mark.parametrize("B,T", [(2, 5), (7, 33), (1025, 1024)])
def test_prep_ids(K, B, T):
    """mask only, shifted only, both; -100 in the ids (a label id: it becomes pad in the shifted ids); B * T above the cap."""
    assert (B, T) != (1025, 1024) or B * T > CAP
    ids = torch.randint(0, 50, (B, T), generator=gen(B))
    ids[torch.rand(B, T, generator=gen(B + 1)) < 0.2] = -100
    ids[torch.rand(B, T, generator=gen(B + 2)) < 0.2] = 1
    ids[0, T - 2] = -100; ids[B - 1, T - 1] = -100
    mask, sh = prep_ids_model(ids, 1, 2)
    assert_differs("-100 kept", sh, torch.cat([torch.full_like(ids[:, :1], 2), ids[:, :-1]], 1))
    assert_differs("shift across rows", sh, torch.cat([torch.tensor([2]), ids.reshape(-1)[:-1]]).reshape(B, T))
    d = ids.cuda()
    m, s = K.prep_ids(d, pad_id=1, start_id=2)
    check_equal(f"prep_ids B={B} T={T} mask", m, mask); check_equal(f"prep_ids B={B} T={T} shifted", s, sh)
    m, s = K.prep_ids(d, pad_id=1, start_id=None)
    assert s is None
    check_equal(f"prep_ids B={B} T={T} mask only", m, mask)
    m, s = K.prep_ids(d, pad_id=1, start_id=2, want_mask=False)
    assert m is None
    check_equal(f"prep_ids B={B} T={T} shifted only", s, sh)
    check_equal("prep_ids ids untouched", d, ids)


# -------------------------------------------------------------------------------- GPU: im2col, vit_assemble
@gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW,p,Kp", [(28, 14, 592), (32, 16, 768), (14, 14, 588)])
def test_im2col(K, HW, p, Kp, B):
    img = torch.randn(B, 3, HW, HW, generator=gen(HW + B))
    check_equal(f"im2col HW={HW} p={p} Kp={Kp} B={B}", K.im2col_patches(img.cuda(), p, Kp), im2col_model(img, p, Kp))


@gpu
def test_im2col_grid_stride(K):
    B, HW, p, Kp = 8, 224, 14, 592
    assert B * (HW // p) ** 2 * Kp > CAP
    img = torch.randn(B, 3, HW, HW, generator=gen(9))
    check_equal(f"im2col HW={HW} p={p} Kp={Kp} B={B}", K.im2col_patches(img.cuda(), p, Kp), im2col_model(img, p, Kp))


@gpu
@pytest.mark.parametrize("B,G2,W", [(1, 1, 8), (2, 4, 72), (3, 49, 768), (28, 49, 768)])
def test_vit_assemble(K, B, G2, W):
    assert B != 28 or B * (G2 + 1) * W > CAP
    pe, cls, pos = q64(B * G2, W, seed=1), q64(W, seed=2), q64(G2 + 1, W, seed=3)
    got = K.vit_assemble(pe.cuda(), cls.cuda(), pos.cuda(), B, G2, W)
    check_equal(f"vit_assemble B={B} G2={G2} W={W}", got, vit_assemble_model(pe, cls, pos, B, G2, W))


# ---------------------------------------------------------------------------------------- GPU: argmax_rows
@gpu
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("V", ARGMAX_V)
def test_argmax_rows(K, V, f32):
    """V < 256 (threads that keep the sentinel), ties inside a thread's stride, across threads and across every reduction half
    (the lowest index wins), ldl > V with larger values in the padding, an all -inf row (0)."""
    c = argmax_case(V, f32)
    got = K.argmax_rows(c["buf"].cuda()[:, :V], V)
    check_equal(f"argmax_rows V={V} f32={f32}", got, c["want"])


# ------------------------------------------------------------------------------------------ GPU: bias_grad
def bias_run(K, c, M, N):
    db = c["db0"].cuda().clone()
    K.bias_grad(c["dy"].cuda()[:, :N], db, M, N)
    torch.cuda.synchronize()
    return db


@gpu
@pytest.mark.parametrize("N", BIAS_N)
@pytest.mark.parametrize("M", BIAS_M)
def test_bias_grad(K, M, N):
    """M < 4 (idle row groups), M = 33 / 65 (a slab that is no multiple of 32; two slabs), N = 513 (one ragged chunk), ldy > N
    with 64 in the padding; accumulates onto a non-zero dbias.  Integer data: exact.  Random data: the fp32 rule."""
    c = bias_case(M, N, True)
    check_equal(f"bias_grad M={M} N={N} integers", bias_run(K, c, M, N), c["r32"])
    r = bias_case(M, N, False)
    got = host(bias_run(K, r, M, N)).to(F64)
    margin = max(8 * (r["r32"].to(F64) - r["r64"]).abs().max().item(), 1e-6 * r["r64"].abs().max().item())
    err = (got - r["r64"]).abs().max().item()
    print(f"MISCCHK bias_grad M={M} N={N} random ({N},) bound={margin:.3e} err={err:.3e}")
    assert err <= margin


@gpu
def test_bias_grad_row_cap(K):
    """M = 1300, N = 50267: 99 column blocks cap the row blocks at 20 < ceil(M / 64) = 21, 65 rows per slab.  Integer data
    generated on the device, a float64 sum as the reference: exact."""
    M, N, ldy = 1300, 50267, 50272
    assert (M + 63) // 64 > 2048 // ((N + 511) // 512)
    g = torch.Generator(device="cuda").manual_seed(5)
    dy = torch.randint(-3, 4, (M, ldy), device="cuda", dtype=torch.int8, generator=g).to(BF16)
    dy[:, N:] = 64.0
    db0 = torch.randint(-5, 6, (N,), device="cuda", generator=g).to(F32)
    want = (db0.to(F64) + dy[:, :N].sum(0, dtype=F64))
    assert want.abs().max().item() < 2 ** 24 and (dy[:-1, :N].sum(0, dtype=F64) != dy[:, :N].sum(0, dtype=F64)).any()
    db = db0.clone()
    K.bias_grad(dy[:, :N], db, M, N)
    torch.cuda.synchronize()
    check_equal(f"bias_grad M={M} N={N} row cap", db.to(F64), want)
