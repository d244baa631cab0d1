"""GPU: the deterministic mode (vacnic_amd.ops.set_deterministic) — the fixed-order kernels one by one, then the whole step.

Where a test says EXACT the reference is a host emulation in np.float32 of the order documented in include/vacnic_hip.h (one
rounded addition after the other), compared with torch.equal; integer-valued inputs must separately match an int64 sum.  Where a
kernel's arithmetic cannot be emulated bit for bit (the LayerNorm / embedding backward), two or three launches must be bit-equal
and the result must meet the float64 bound of the existing test of the same kernel (tests/test_norm_gpu.py: check / f32_margin —
imported, not re-derived)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F32, BF16 = torch.float32, torch.bfloat16
f32 = np.float32
PAD = 1


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


@pytest.fixture()
def det(K):
    """the mode on for one test, whatever it was before afterwards"""
    from vacnic_amd import ops
    with ops.deterministic_mode(True):
        yield ops
    assert not K.DETERMINISTIC


def rnd(*shape, seed, ints=False, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    if ints:
        return torch.randint(-4, 5, shape, generator=g).to(F32)
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------ host emulations
def fold_emul(p, dst0):
    """vacnic_fold_ordered: strand w adds rows w, w + 4, ... from +0; ((s0 + s1) + s2) + s3; dst + t."""
    NB, cols = p.shape
    s = np.zeros((4, cols), f32)
    for b in range(NB):
        s[b % 4] = s[b % 4] + p[b]
    t = ((s[0] + s[1]) + s[2]) + s[3]
    return dst0 + t


def sum_emul(src):
    """vacnic_sum_ordered: strand t adds src[t], src[t + 256], ... from +0; the 256 strand sums are added in ascending order."""
    n = src.shape[0]
    pad = np.zeros(((n + 255) // 256) * 256, f32)         # x + 0 == x: the padding adds nothing
    pad[:n] = src
    s = np.zeros(256, f32)
    for row in pad.reshape(-1, 256):
        s = s + row
    t = f32(0.0)
    for v in s:
        t = f32(t + v)
    return t


def scatter_emul(src, ids, V, T, off, scale, demb, dpos):
    """vacnic_scatter_ordered on host arrays (demb: dict id -> prefilled row; dpos: prefilled array), in place."""
    R = src.shape[0]
    acc = {}
    for r in range(R):
        if ids[r] == PAD:
            continue
        k = int(min(max(ids[r], 0), V - 1))
        acc[k] = src[r].copy() if k not in acc else acc[k] + src[r]
    out = {k: demb[k] + f32(scale) * a for k, a in acc.items()}
    nt = min(T, R)
    a = src[:nt].copy()
    for r0 in range(T, R, T):
        n = min(T, R - r0)
        a[:n] = a[:n] + src[r0:r0 + n]
    dpos = dpos.copy()
    dpos[off:off + nt] = dpos[off:off + nt] + a
    return out, dpos


# ------------------------------------------------------------------------------------------------ 1. ordered fold
@pytest.mark.parametrize("cols", [8, 64, 72, 2048])
@pytest.mark.parametrize("NB", [1, 3, 4, 5, 1024])
def test_fold_ordered_exact(K, NB, cols):
    for ints in (False, True):
        p = rnd(NB, cols, seed=NB * 7 + cols, ints=ints)
        d0 = rnd(cols, seed=cols + 1, ints=ints) + 3.0
        dst = d0.cuda()
        K.fold_ordered(p.cuda(), dst, None, NB, cols)
        want = fold_emul(p.numpy(), d0.numpy())
        assert torch.equal(dst.cpu(), torch.from_numpy(want)), f"fold NB={NB} cols={cols} ints={ints}"
        if ints:
            assert torch.equal(dst.cpu().to(torch.int64), d0.to(torch.int64) + p.to(torch.int64).sum(0))
    # two destinations out of rows [NB][2][cols] with a row stride of its own (the LayerNorm layout), a pad column block behind
    p = rnd(NB, 2 * cols + 8, seed=NB + cols)
    d0, e0 = rnd(cols, seed=1) - 2.0, rnd(cols, seed=2) + 5.0
    dst, dst2 = d0.cuda(), e0.cuda()
    K.fold_ordered(p.cuda(), dst, dst2, NB, cols, ld=2 * cols + 8)
    assert torch.equal(dst.cpu(), torch.from_numpy(fold_emul(p[:, :cols].numpy(), d0.numpy())))
    assert torch.equal(dst2.cpu(), torch.from_numpy(fold_emul(p[:, cols:2 * cols].numpy(), e0.numpy())))


def test_fold_ordered_empty_and_refusals(K):
    d0 = rnd(72, seed=3)
    dst = d0.cuda()
    K.fold_ordered(torch.zeros(1, 72, device="cuda"), dst, None, 0, 72)
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), d0), "NB = 0 must leave dst alone"
    with pytest.raises(ValueError, match="fold_ordered"):
        K.fold_ordered(torch.zeros(4, 72, device="cuda"), dst, None, 4, 72, ld=64)
    with pytest.raises(ValueError, match="fold_ordered"):
        K.fold_ordered(torch.zeros(4, 72, device="cuda"), dst, None, -1, 72)
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), d0)


# ------------------------------------------------------------------------------------------------ 2. ordered scatter
def scatter_ids(R, V, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (R,), generator=g)
    if V == 7:
        heavy = torch.rand(R, generator=g) < 0.55            # one id holds more than half of the rows: every segment is long
        ids[heavy] = 3
    if R >= 8:
        ids[5::13] = PAD
        ids[2], ids[R - 1], ids[4] = -3, V + 5, 0            # -3 joins id 0, V + 5 joins id V - 1
    return ids


@pytest.mark.parametrize("D", [8, 768, 1024])
@pytest.mark.parametrize("R", [1, 64, 65, 4099])
def test_scatter_ordered_exact(K, R, D):
    off, scale = 2, float(f32(math.sqrt(D)))
    for V in (7, 50265):
        for B in (1, 3):
            T = (R + B - 1) // B
            for ints in (False, True):
                ids = scatter_ids(R, V, seed=R + D + V)
                src = rnd(R, D, seed=R * 3 + D + B, ints=ints)
                sc = 2.0 if ints else scale
                # pre-filled destinations from a pattern the host can repeat for the touched rows only (V = 50265: 200 MB)
                demb = ((torch.arange(V * D, device="cuda", dtype=torch.int64) % 1021).to(F32) * 0.125 - 3.0).view(V, D)
                dpos0 = ((torch.arange((T + off) * D, dtype=torch.int64) % 509).to(F32) * 0.25 - 7.0).view(T + off, D)
                demb0 = demb.clone()
                dpos = dpos0.cuda()
                K.scatter_ordered(src.cuda(), ids.cuda(), demb, dpos, T, V, pos_offset=off, padding_idx=PAD, scale=sc)
                torch.cuda.synchronize()
                touched = sorted({int(min(max(i, 0), V - 1)) for i in ids.tolist() if i != PAD})
                rows0 = {k: demb0[k].cpu().numpy() for k in touched}
                want_e, want_p = scatter_emul(src.numpy(), ids.numpy(), V, T, off, sc, rows0, dpos0.numpy())
                what = f"scatter R={R} D={D} V={V} B={B} ints={ints}"
                for k in touched:
                    assert torch.equal(demb[k].cpu(), torch.from_numpy(want_e[k])), f"{what}: demb[{k}]"
                keep = torch.ones(V, dtype=torch.bool, device="cuda")
                keep[torch.tensor(touched, device="cuda", dtype=torch.int64)] = False
                assert torch.equal(demb[keep], demb0[keep]), f"{what}: a row without a contribution (padding_idx among them) moved"
                assert torch.equal(dpos.cpu(), torch.from_numpy(want_p)), f"{what}: dpos"
                if ints:
                    s64, i64 = src.to(torch.int64), ids.clamp(0, V - 1)
                    e64 = torch.zeros(V, D, dtype=torch.int64).index_add_(0, i64[ids != PAD], s64[ids != PAD])
                    got = (demb.cpu().double() - demb0.cpu().double())
                    assert torch.equal(got[touched], 2.0 * e64[touched].double()), f"{what}: int64 sum"


def test_scatter_ordered_refusals(K):
    src = torch.zeros(4, 12, device="cuda")
    ids = torch.zeros(4, dtype=torch.int64, device="cuda")
    dst = torch.zeros(8, 12, device="cuda")
    with pytest.raises(ValueError, match="scatter_ordered"):
        K.scatter_ordered(src[:, :10].contiguous(), ids, dst, None, 4, 8)          # D % 4 != 0
    with pytest.raises(ValueError, match="scatter_ordered"):
        K.scatter_ordered(src, ids, dst, None, 0, 8)                               # T = 0
    torch.cuda.synchronize()
    assert (dst == 0).all()


# ------------------------------------------------------------------------------------------------ 3. embedding backward
def _embed(K, N, t, scale, off, p, seed, ordered):
    K.DETERMINISTIC = ordered
    try:
        return N.embed_run(K, t, scale, off, p=p, seed=seed)
    finally:
        K.DETERMINISTIC = False


@pytest.mark.parametrize("D", [768, 1032])
def test_embed_bwd_ordered_equals_atomic_without_collisions(K, D):
    """B = 1, all ids distinct, zeroed gradients: no two contributions meet in demb / dpos, so the ordered path must give the atomic
    kernel's bits.  T = 8 is two blocks of four rows: dgamma / dbeta then have exactly two contributions each, whose sum does not
    depend on the order (a + b == b + a), so they must be equal too; with more blocks the atomic kernel's own result varies."""
    import test_norm_gpu as N
    off, scale = 2, float(f32(math.sqrt(D)))
    for T in (8, 40):
        t = N.embed_inputs(3, 40, 50, D, off, seed=D)
        vals = torch.tensor([v for v in range(50) if v != PAD])          # no pad row, all distinct
        ids = vals[torch.randperm(49, generator=torch.Generator().manual_seed(T))[:T]].view(1, T)
        assert ids.unique().numel() == T
        t = dict(t, ids=ids, dout=t["dout"][:1, :T].contiguous(), de0=torch.zeros_like(t["de0"]), dp0=torch.zeros_like(t["dp0"]),
                 dg0=torch.zeros_like(t["dg0"]), db0=torch.zeros_like(t["db0"]))
        for p in (0.0, 0.1):
            a = _embed(K, N, t, scale, off, p, N.SEED, False)
            o = _embed(K, N, t, scale, off, p, N.SEED, True)
            for key in ("demb", "dpos") + (("dgamma", "dbeta") if T == 8 else ()):
                assert torch.equal(a[key], o[key]), f"D={D} T={T} p={p}: {key} differs from the atomic kernel's"


@pytest.mark.parametrize("D", [768, 1032])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_embed_bwd_ordered_collisions(K, D, p):
    """B = 3, T = 70, 7 ids: ~30 rows per embedding row.  Two launches bit-equal; the float64 bound of test_norm_gpu.test_embed_ln."""
    import test_norm_gpu as N
    off, scale, B, T, V = 2, float(f32(math.sqrt(D))), 3, 70, 7
    t = N.embed_inputs(B, T, V, D, off, seed=D + 1)
    o1 = _embed(K, N, t, scale, off, p, N.SEED, True)
    o2 = _embed(K, N, t, scale, off, p, N.SEED, True)
    for key in ("demb", "dpos", "dgamma", "dbeta"):
        assert torch.equal(o1[key], o2[key]), f"{key}: two launches differ"
    keep, inv = None, 1.0
    if p:
        thr = N.drop_threshold(p)
        keep, inv = N.hidden_keep(B * T, D, N.SEED, thr), N.inv_keep_of(thr)
    r64, r32 = N.embed_ref(t, scale, off, N.F64, keep, inv), N.embed_ref(t, scale, off, N.F32, keep, inv)
    for key in ("demb", "dpos", "dgamma", "dbeta"):
        N.check(f"embed_ln ordered D={D} p={p}", o1[key], r64, r32, key)
    assert torch.equal(o1["demb"].cpu()[PAD], t["de0"][PAD]), "demb[padding_idx] moved"


# ------------------------------------------------------------------------------------------------ 4. LayerNorm backward
@pytest.mark.parametrize("residual,p", [(True, 0.0), (True, 0.1), (False, 0.1)])
@pytest.mark.parametrize("D", [768, 1024])
@pytest.mark.parametrize("R", [1, 3, 255, 256, 257, 4100])
def test_add_ln_bwd_ordered(K, R, D, residual, p):
    """dx / dres are the default path's bits; dgamma / dbeta bit-equal over three launches and inside the float64 bound of
    test_norm_gpu (add_ln_compare); no atomic fold and no atomic branch at any R (the entry points are logged)."""
    import test_norm_gpu as N
    from vacnic_amd import _lib
    t = N.add_ln_inputs(R, D, seed=R + D)
    base = N.add_ln_run(K, t, p=p, seed=N.SEED, residual=residual)
    log, call0, cs0 = [], K.call, K.call_struct
    K.call = lambda name, *a: (log.append(name), call0(name, *a))[1]
    K.call_struct = lambda name, **kw: (log.append((name, kw.get("partials_any"), kw.get("defer_fold"))), cs0(name, **kw))[1]
    K.DETERMINISTIC = True
    try:
        runs = [N.add_ln_run(K, t, p=p, seed=N.SEED, residual=residual) for _ in range(3)]
    finally:
        K.DETERMINISTIC = False
        K.call, K.call_struct = call0, cs0
    assert "vacnic_ln_partial_fold" not in log and log.count("vacnic_fold_ordered") == 3
    assert log.count(("vacnic_add_ln_bwd", 1, 1)) == 3, log
    for r in runs:
        assert torch.equal(r["dx"], base["dx"]) and torch.equal(r["dres"], base["dres"]), "dx / dres moved"
        for key in ("dgamma", "dbeta"):
            assert torch.equal(r[key], runs[0][key]), f"{key}: launches differ"
    keep, inv = None, 1.0
    if p:
        thr = N.drop_threshold(p)
        keep, inv = N.hidden_keep(R, D, N.SEED, thr), N.inv_keep_of(thr)
    N.add_ln_compare(f"add_ln ordered R={R} D={D} res={residual} p={p}", runs[0], t, keys=("dx", "dgamma", "dbeta") + (("dres",) if residual else ()), keep=keep,
                     inv_keep=inv, residual=residual)


# ------------------------------------------------------------------------------------------------ 5. bias gradient
@pytest.mark.parametrize("N_", [8, 72, 520])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 1000])
def test_bias_grad_ordered(K, M, N_):
    ldy = N_ + 8
    assert K.bias_grad_ordered_rows(M) == min(256, max(1, (M + 63) // 64))
    big = rnd(M, ldy, seed=M + N_, ints=True).to(BF16).cuda()
    d0 = rnd(N_, seed=N_, ints=True)
    db = d0.cuda()
    K.bias_grad_ordered(big[:, :N_], db, M, N_)
    assert torch.equal(db.cpu().to(torch.int64), d0.to(torch.int64) + big[:, :N_].cpu().to(torch.int64).sum(0)), "integer data: exact"
    big = (rnd(M, ldy, seed=M * 3 + N_)).to(BF16).cuda()
    outs = []
    for _ in range(2):
        db = (d0 + 0.5).cuda()
        K.DETERMINISTIC = True                       # the public wrapper of a bias without a weight takes the ordered kernel too
        try:
            K.bias_grad(big[:, :N_], db, M, N_)
        finally:
            K.DETERMINISTIC = False
        outs.append(db.clone())
    assert torch.equal(outs[0], outs[1])
    ref = (d0 + 0.5).double() + big[:, :N_].cpu().double().sum(0)
    # every partial sum is below sum |x|, and there are at most M + 8 rounded additions behind an element
    bound = (M + 8) * 2.0 ** -24 * (big[:, :N_].cpu().double().abs().sum(0) + (d0 + 0.5).abs().double())
    assert ((outs[0].cpu().double() - ref).abs() <= bound).all()


def test_bias_grad_ordered_refusals(K):
    dy = torch.zeros(100, 16, device="cuda", dtype=BF16)
    db = torch.zeros(16, device="cuda")
    with pytest.raises(ValueError, match="partials holds 1 rows, 2 needed"):
        K.bias_grad_ordered(dy, db, 100, 16, partials=torch.zeros(1, 16, device="cuda"))
    torch.cuda.synchronize()
    assert (db == 0).all()


# ------------------------------------------------------------------------------------------------ 6. loss sums
def _targets(R, V, seed, all_ignored):
    tgt = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(seed))
    tgt[tgt == PAD] = 0
    if R > 1:
        tgt[1::3] = PAD
    if all_ignored:
        tgt[:] = PAD
    return tgt


@pytest.mark.parametrize("all_ignored", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("R", [1, 4, 5, 2051])
def test_lmhead_loss_sum_ordered(K, R, eps, all_ignored):
    V, d = 50265, 64
    Vp = (V + 31) // 32 * 32
    E = torch.zeros(Vp, d, dtype=BF16)
    E[:V] = (rnd(V, d, seed=9, scale=0.3)).to(BF16)
    h, E = rnd(R, d, seed=R).to(BF16).cuda(), E.cuda()
    tgt = _targets(R, V, R + 1, all_ignored).cuda()
    lse0, acc0 = K.lmhead_ce_fwd(h, E, tgt, V, ignore_index=PAD, label_smoothing=eps)
    tiles = (V + 255) // 256
    part = torch.empty((R, tiles, 2), device="cuda"); tl = torch.empty(R, device="cuda"); lse = torch.empty(R, device="cuda")
    ps = torch.empty((R, tiles), device="cuda") if eps else None
    outs = [K.lmhead_ce_fwd_ordered(h, E, tgt, V, part, tl, lse, PAD, eps, None, ps) for _ in range(2)]
    lse1, acc1, row_loss = outs[0]
    torch.cuda.synchronize()
    assert torch.equal(lse1, lse0), "row_lse moved"
    assert torch.equal(acc1[1], acc0[1]) and acc0[1].item() == (tgt != PAD).sum().item(), "count moved"
    assert (row_loss[tgt == PAD] == 0).all() and torch.signbit(row_loss[tgt == PAD]).sum() == 0, "ignored rows: an exact +0"
    assert acc1[0].item() == float(sum_emul(row_loss.cpu().numpy())), "loss_sum is not the documented sum of the kernel's own row terms"
    assert torch.equal(outs[1][1][:2], acc1[:2])
    # against the default path's atomic sum (not bit-equal by design): both add the same terms, at most 2 R of them with label
    # smoothing (the default adds the two parts of a row separately, together at most 1.5 of the row term here), each order off by
    # at most (addends - 1) * 2^-24 * sum |addend|
    bound = 2 * (2 * R) * 2.0 ** -24 * 1.5 * row_loss.double().abs().sum().item()
    assert abs(acc1[0].item() - acc0[0].item()) <= bound, (acc1.tolist(), acc0.tolist(), bound)
    # the mode switch takes the same path, and the backward operands built from its outputs are the default path's bits
    K.DETERMINISTIC = True
    try:
        lse2, acc2 = K.lmhead_ce_fwd(h, E, tgt, V, ignore_index=PAD, label_smoothing=eps)
    finally:
        K.DETERMINISTIC = False
    assert torch.equal(lse2, lse0) and torch.equal(acc2[:2], acc1[:2])
    n = 512
    dl = []
    for l, a in ((lse0, acc0), (lse2, acc2)):
        rowp = K.lmhead_ce_rowp(l, tgt, a, ignore_index=PAD, label_smoothing=eps, V=V)
        buf = torch.zeros((R, n), device="cuda", dtype=BF16)
        K.lmhead_ce_dlogits(h, E, tgt, V, rowp, buf, 0, n, ignore_index=PAD, label_smoothing=eps)
        dl.append(buf)
    assert torch.equal(dl[0], dl[1]), "dlogits moved"


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("R", [1, 4, 5, 2051])
def test_ce_fwd_loss_sum_ordered(K, R, eps):
    V = 264
    for all_ignored in (False, True):
        for dt in (BF16, F32):
            logits = rnd(R, V + 8, seed=R + 3).to(dt).cuda()
            tgt = _targets(R, V, R + 2, all_ignored).cuda()
            lse0, acc0 = K.ce_fwd(logits, tgt, V, ignore_index=PAD, label_smoothing=eps)
            lse1, acc1, row_loss = K._ce_fwd_ordered(logits, tgt, V, PAD, eps, torch.empty(R, device="cuda"))
            K.DETERMINISTIC = True
            try:
                lse2, acc2 = K.ce_fwd(logits, tgt, V, ignore_index=PAD, label_smoothing=eps)
            finally:
                K.DETERMINISTIC = False
            assert torch.equal(lse1, lse0) and torch.equal(lse2, lse0), "row_lse moved"
            assert torch.equal(acc1[1], acc0[1]) and torch.equal(acc2[:2], acc1[:2]), "count moved"
            assert (row_loss[tgt == PAD] == 0).all()
            assert acc1[0].item() == float(sum_emul(row_loss.cpu().numpy()))
            dls = []
            for l, a in ((lse0, acc0), (lse2, acc2)):
                dlg = torch.zeros((R, V + 8), device="cuda", dtype=BF16)
                K.ce_bwd(logits, tgt, V, l, a, dlg, ignore_index=PAD, label_smoothing=eps)
                dls.append(dlg)
            assert torch.equal(dls[0], dls[1]), "dlogits moved"


def test_sum_ordered_exact(K):
    for n in (0, 1, 255, 256, 257, 5000):
        src = rnd(n, seed=n + 1) if n else torch.zeros(0)
        dst = torch.full((1,), 7.0, device="cuda")
        K.sum_ordered(src.cuda(), dst)
        assert dst.item() == float(sum_emul(src.numpy())), n
    src = rnd(5000, seed=1, ints=True)
    dst = torch.zeros(1, device="cuda")
    K.sum_ordered(src.cuda(), dst)
    assert int(dst.item()) == int(src.to(torch.int64).sum())


# ------------------------------------------------------------------------------------------------ 7. the step
def _step_model(tied=False, drop=0.1):
    from vacnic_amd.config import ClipVisionConfig, VacnicConfig
    from vacnic_amd.training import build_models
    kw = dict(encoder_layers=2, decoder_layers=1, enc_fusion_layer=[0, 1], init_attn_weight=True) if tied else \
        dict(encoder_layers=2, decoder_layers=2, enc_fusion_layer=[0])
    cfg = VacnicConfig(d_model=768, encoder_attention_heads=12, decoder_attention_heads=12, encoder_ffn_dim=3072, decoder_ffn_dim=3072,
                       dim_common=768, clip_width=128, dropout=drop, attention_dropout=drop, activation_dropout=drop, **kw)
    vcfg = ClipVisionConfig(width=128, layers=1, patch_size=16, image_size=32, output_dim=64)
    model, guide, _ = build_models(cfg, vcfg, init="synthetic", seed=3)
    model.train()
    return cfg, model, guide


class _Busy:
    """unrelated GEMMs of the project queued on a second stream: they change which workgroups of the pass under test arrive first"""

    def __init__(self):
        self.stream = torch.cuda.Stream()
        self.x = torch.randn(2048, 2048, device="cuda").to(BF16)
        self.o = torch.empty(2048, 2048, device="cuda", dtype=BF16)

    def run(self, K, shape, n):
        M, N, Kd = shape
        with torch.cuda.stream(self.stream):
            for _ in range(n):
                K.gemm(self.x, self.x, M, N, Kd, out=self.o, ldx=2048, ldw=2048, ldo=2048)


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("side", [True, False])
def test_step_is_bitwise_reproducible(K, det, side, tied):
    """three forward + backward passes from the same state (all three dropouts 0.1, same seeds and device counter), passes 2 and 3
    beside unrelated GEMMs on another stream: the whole gradient arena and the loss vector, bit for bit."""
    from vacnic_amd import ops, streams, synthetic
    from vacnic_amd.training import TrainArgs, forward_losses, to_device
    streams.enable(side)
    try:
        cfg, model, guide = _step_model(tied)
        geo = dict(S=40, T=10, F=2) if tied else dict(S=48, T=12, F=3)
        batch = to_device(synthetic.make_batch(cfg, 2 if tied else 3, seed=11, image_size=32, full_length=True, **geo), "cuda")
        args, busy = TrainArgs(), _Busy()
        grads, losses = [], []
        for i in range(3):
            model.arena.grad.zero_()
            ops.Rng.manual_seed(5); ops.Rng.device_counter().zero_()
            torch.cuda.synchronize()
            if i:
                busy.run(K, [(2048, 2048, 1024), (512, 2048, 2048)][i - 1], 300)
            ops.begin_step()
            total, out4, _ = forward_losses(model, guide, batch, args)
            with torch.autograd.set_multithreading_enabled(False):
                total.backward(ops.const_one(total.device))
            ops.flush_wgrads()
            streams.join_all()
            torch.cuda.synchronize()
            grads.append(model.arena.grad.clone()); losses.append(out4.clone())
        assert torch.isfinite(losses[0]).all() and grads[0].abs().sum().item() > 0
        for i in (1, 2):
            assert torch.equal(losses[i], losses[0]), (i, losses[i].tolist(), losses[0].tolist())
            nd = int((grads[i] != grads[0]).sum().item())
            assert nd == 0, f"pass {i}: {nd} of {grads[0].numel()} gradient elements differ"
    finally:
        streams.enable(False)


@pytest.mark.parametrize("side", [True, False])
def test_planned_step_equals_eager_bitwise(K, side):
    """the set-up of test_model_gpu.test_planned_step_replays_like_eager (dropout off, three batches, no tower graphs) with
    TrainArgs.deterministic: losses and final fp32 weights are torch.equal, no tolerance."""
    from vacnic_amd import ops, streams, synthetic
    from vacnic_amd.config import ClipVisionConfig
    from vacnic_amd.training import FusedAdamW, PlannedTrainStep, TrainArgs, build_models, to_device, train_step
    from test_model_gpu import small_cfg
    cfg = small_cfg(dropout=0.0, encoder_layers=2, decoder_layers=2, enc_fusion_layer=[0, 1])
    vcfg = ClipVisionConfig(width=768, layers=1, patch_size=16, image_size=32, output_dim=64)
    args = TrainArgs(num_training_steps=20, warmup_rate=0.1, lr_bart=1e-4, deterministic=True)
    batches = [to_device(synthetic.make_batch(cfg, 3, S=32, T=12, F=3, seed=40 + i, image_size=32), "cuda") for i in range(3)]
    streams.enable(side)
    try:
        runs, weights = [], []
        for planned in (False, True):
            ops.Rng.manual_seed(3); ops.Rng.device_counter().zero_()
            model, guide, _ = build_models(cfg, vcfg, init="synthetic", seed=0)
            opt = FusedAdamW(model.arena, lr=args.lr_bart, weight_decay=args.weight_decay, num_warmup_steps=2, num_training_steps=20)
            if planned:
                step = PlannedTrainStep(model, guide, opt, args, batches[0], warmup=2)
                assert not ops.deterministic(), "TrainArgs.deterministic must not leak out of the step"
                losses = [step(b).clone() for b in batches[1:] + batches[:1]]
                step.close()
            else:
                for _ in range(3):
                    train_step(model, guide, opt, batches[0], args)
                losses = [train_step(model, guide, opt, b, args).clone() for b in batches[1:] + batches[:1]]
            torch.cuda.synchronize()
            runs.append(torch.stack(losses))
            weights.append(model.arena.flat32.clone())
        assert torch.isfinite(runs[0]).all()
        assert torch.equal(runs[1], runs[0]), (runs[1].tolist(), runs[0].tolist())
        assert torch.equal(weights[1], weights[0]), int((weights[1] != weights[0]).sum().item())
    finally:
        streams.enable(False)


NEW_ENTRY_POINTS = {"vacnic_fold_ordered", "vacnic_bias_grad_ordered", "vacnic_scatter_ordered", "vacnic_embed_ln_bwd_ordered",
                    "vacnic_sum_ordered", "vacnic_lmhead_row_loss"}


@pytest.mark.parametrize("side", [True, False])
def test_off_is_untouched_and_on_is_complete(K, side):
    """entry points of one step in each mode: off calls none of the new ones (and passes no partials_any); on has no launch with a
    non-null xsum, no out_mode 2 split-K launch without the fix-up, no atomic LayerNorm fold and no atomic bias gradient."""
    from vacnic_amd import _lib, ops, streams, synthetic
    from vacnic_amd.training import FusedAdamW, TrainArgs, to_device, train_step
    streams.enable(side)
    log = []
    call0, cs0, lcall0, lcs0 = K.call, K.call_struct, _lib.call, _lib.call_struct

    def call(name, *a):
        log.append((name, {}))
        return call0(name, *a)

    def call_struct(name, **kw):
        log.append((name, dict(kw)))
        return cs0(name, **kw)
    try:
        cfg, model, guide = _step_model()
        batch = to_device(synthetic.make_batch(cfg, 3, S=48, T=12, F=3, seed=11, image_size=32, full_length=True), "cuda")
        opt = FusedAdamW(model.arena, lr=1e-4, weight_decay=0.01, num_warmup_steps=2, num_training_steps=20)
        K.call = _lib.call = call
        K.call_struct = _lib.call_struct = call_struct
        for mode in (False, True):
            del log[:]
            train_step(model, guide, opt, batch, TrainArgs(num_training_steps=20, deterministic=mode))
            torch.cuda.synchronize()
            names = [n for n, _ in log]
            gemms = [kw for n, kw in log if n == "vacnic_gemm_bf16"]
            assert len(gemms) > 50
            if not mode:
                assert not NEW_ENTRY_POINTS & set(names), NEW_ENTRY_POINTS & set(names)
                assert all(not kw.get("partials_any") for n, kw in log if n == "vacnic_add_ln_bwd")
                assert any(kw["xsum"] for kw in gemms), "the default step forms bias gradients in the weight-gradient GEMMs"
            else:
                assert NEW_ENTRY_POINTS - {"vacnic_scatter_ordered"} <= set(names), NEW_ENTRY_POINTS - set(names)
                assert not any(kw["xsum"] for kw in gemms), "a launch carries a non-null xsum"
                bad = [kw for kw in gemms if kw["out_mode"] == 2 and kw["split_k"] > 1 and not kw["workspace"]]
                assert not bad, f"{len(bad)} split-K launches sum through atomics"
                assert "vacnic_ln_partial_fold" not in names and "vacnic_bias_grad" not in names and "vacnic_embed_ln_bwd" not in names
                assert all(kw.get("partials_any") == 1 and kw.get("defer_fold") == 1 for n, kw in log if n == "vacnic_add_ln_bwd")
    finally:
        K.call, K.call_struct, _lib.call, _lib.call_struct = call0, cs0, lcall0, lcs0
        streams.enable(False)
