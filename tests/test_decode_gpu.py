"""Decode kernels (csrc/decode.hip): vacnic_beam_topk, vacnic_lmhead_topk, vacnic_gather_rows, vacnic_beam_init / vacnic_beam_step
against float64 references and the host beam-search bookkeeping of oracle/vacnic_oracle.py, at every path edge of the kernels.

Margins (none is taken from a kernel's output; every value check prints `DECCHK <what> margin=.. err=.. used=..`, one run of them
is kept in profiles/decode_tests.txt):
  * scores (top_val): float64 log_softmax of the exact inputs (+ the beam score) is the reference; the kernel may deviate by 8x the
    largest deviation of torch's fp32 log_softmax (+ beam score) on the same input, floored at 1e-6 * max|ref|.
  * vacnic_lmhead_topk's logits output: 8x the deviation of the fp32 skinny GEMM (K.gemm, out_mode=1) from float64 h @ emb.T + bias,
    same floor.
  * picks, bans, histories, n-best lists: exact.

vacnic_beam_topk: which input enters which path of beam_topk_fast_kernel.  `fast_path()` restates on the host which thread walks
which element, and from that the threshold T (K <= 16: K-th largest WAVE maximum; K > 16: K-th largest THREAD maximum) and
cnt = #{masked logit >= T}; every test asserts the path on its INPUT before it looks at the output.
  test_topk_wave_pick        random fp32 / bf16, V = 50267, K = 1, 10, 16, R = 5 and 80: cnt <= 256, wave 0 picks.  bf16 rows hold exact
                             ties inside the top K (asserted), so (score desc, index asc) decides.
  test_topk_wave_pick_many_ties  200 copies of the row maximum: still cnt <= 256, several tied candidates per lane of wave 0.
  test_topk_block_pick       600 copies of the row maximum: 256 < cnt <= 1024, block-wide pick; K = 10 (wave-maximum threshold) and
                             K = 300 (thread-maximum threshold, picks from many lanes).
  test_topk_overflow         1500 copies: cnt > 1024 -> K arg-max passes over the row.
  test_topk_minus_inf_threshold  V = 40, K = 10 (one wave has data) and V = 5000 with all but K - 1 tokens banned: T == -inf -> the same
                             fallback.  The kernel documents that the slots beyond the finite scores hold -inf with the remaining token
                             ids in ascending order (banned ones included: they score -inf like any other).
  test_topk_thread_threshold K = 17, 32, 64: the K-th largest thread maximum.
  test_topk_scalar_walk      fp32, ldl = 50269 in a view one element into its buffer: rows at 16-byte boundaries take 16-byte loads
                             + the V % 4 tail, the others scalar loads (data_ptr % 16 asserted, both kinds present); V = 1027 (tail of 3).
  test_topk_bans_and_suppression  ban entries -1, V, > V, duplicates, the arg-max; eos inside / outside the vocabulary.
  test_topk_slow_kernel      K = 1025 > 1024 threads: beam_topk_kernel's generic path; forced tokens (0, V - 1, with a beam score).
  test_topk_refusals
The padding columns V..ldl of every logits buffer hold 1e4 and must never be picked.

vacnic_lmhead_topk: LM_CASES names what each (V, d, R, K2) is there for (tpw = 16-column tiles per workgroup 1 / 2 / 7, a single-tile
last workgroup, lmhead_part_kernel<2> / <8>, a cut K step); then list exhaustion in the merge, ties across workgroups, bans at the
column-range edges, the merge kernel's LDS above 64 KiB, refusals.

vacnic_gather_rows: the grid-stride wrap (rows x chunks > 4096 x 256), period with stride > row, duplicates, empty calls, refusals.

vacnic_beam_init / vacnic_beam_step: the device state and a host loop built from oracle._BeamHyps / banned_ngram_tokens (itself pinned
against oracle.beam_search_bookkeeping on the same table, on the CPU) advance in lockstep over a scripted score table whose values are
negative multiples of 2^-8 below 16: every running sum is exact in fp32, so scores compare bitwise.  The per-row top-K2 lists the
kernel consumes are computed on the host (device bans and beam scores applied), which isolates the step kernel from the top-k
kernels.  A separate hand-written case pins the merge order on equal scores.

Open (not covered): logits rows that are entirely -inf (log-sum-exp of nothing); the slow kernel with long ban lists (its scan is
n_ban compares per logit; the fast kernel is run with n_ban = 4991); nb = 16 with the 2 nb candidates per row that beam search needs
(vacnic_beam_step refuses nb * K2 > 128, generate() keeps such searches on the host scorer).
"""
import math

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
NEG = -float("inf")
PAD_LOGIT = 1e4                          # what the columns V..ldl hold


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


def rng(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def margin_of(ref64, ref32, what):
    """8x the deviation of fp32 torch from float64 over the finite entries, floored at 1e-6 * max|ref|."""
    fin = torch.isfinite(ref64)
    dev = (ref32.to(F64)[fin] - ref64[fin]).abs().max().item()
    return max(8.0 * dev, 1e-6 * ref64[fin].abs().max().item()), dev


def report(what, margin, err):
    print(f"DECCHK {what} margin={margin:.3e} err={err:.3e} used={err / margin:.3f}")


# ------------------------------------------------------------------------------------------ beam_topk: host model
def ban_mask(R, V, bans, eos, suppress):
    m = np.zeros((R, V), dtype=bool)
    if bans is not None:
        for r, row in enumerate(bans.tolist()):
            for t in row:
                if 0 <= t < V:
                    m[r, t] = True
    if suppress and 0 <= eos < V:
        m[:, eos] = True
    return m


def topk_reference(raw, K_, bs, mask):
    """raw [R, V] (fp32 / bf16, CPU).  Picks in the order (masked raw logit desc, index asc); float64 and fp32-torch scores [R, V]."""
    x = raw.to(F64)
    masked = np.where(mask, NEG, x.numpy())
    order = np.argsort(-masked, axis=1, kind="stable")[:, :K_]
    b64 = torch.zeros(raw.shape[0], dtype=F64) if bs is None else bs.to(F64)
    b32 = torch.zeros(raw.shape[0], dtype=F32) if bs is None else bs
    s64 = torch.log_softmax(x, -1) + b64[:, None]
    s32 = torch.log_softmax(raw.to(F32), -1) + b32[:, None]
    return masked, order, s64, s32


def fast_path(masked_row, K_, aligned):
    """(path, cnt) of beam_topk_fast_kernel for one row: the row walk gives element j to thread (j // 4) % 1024 on the 16-byte path
    (tail: (j - 4 * (V // 4)) % 1024) and to thread j % 1024 on the scalar path."""
    V = masked_row.shape[0]
    j = np.arange(V)
    if aligned:
        nv = (V >> 2) << 2
        tid = np.where(j < nv, (j >> 2) % 1024, (j - nv) % 1024)
    else:
        tid = j % 1024
    tmax = np.full(1024, NEG)
    np.maximum.at(tmax, tid, masked_row)
    m = tmax.reshape(16, 64).max(1) if K_ <= 16 else tmax
    T = np.sort(m)[::-1][K_ - 1]
    if T == NEG:
        return "fallback", 0
    cnt = int((masked_row >= T).sum())
    return ("wave" if cnt <= 256 else "block" if cnt <= 1024 else "overflow"), cnt


def padded(raw, ldl):
    """[R, ldl] buffer of raw's dtype: raw in the first V columns, PAD_LOGIT beyond."""
    R, V = raw.shape
    buf = torch.full((R, ldl), PAD_LOGIT, dtype=raw.dtype)
    buf[:, :V] = raw
    return buf


def check_topk(K, what, raw, K_, *, bs=None, bans=None, eos=2, suppress=False, ldl=None, path=None, dev_logits=None):
    """run vacnic_beam_topk on raw [R, V] and compare picks exactly and scores to the measured margin; returns (tv, ti, paths)."""
    R, V = raw.shape
    lg = dev_logits if dev_logits is not None else padded(raw, ldl or (V + 7) // 8 * 8).cuda()
    mask = ban_mask(R, V, bans, eos, suppress)
    masked, order, s64, s32 = topk_reference(raw, K_, bs, mask)
    paths = []
    if K_ <= 1024 and V <= 262144:
        for r in range(R):
            aligned = raw.dtype == F32 and (lg.data_ptr() + r * lg.stride(0) * 4) % 16 == 0
            paths.append(fast_path(masked[r], K_, aligned))
        if path is not None:
            assert all(p[0] == path for p in paths), (what, path, paths)
    tv, ti = K.beam_topk(lg, V, K_, beam_scores=None if bs is None else bs.cuda(), bans=None if bans is None else bans.cuda(), eos=eos,
                         suppress_eos=suppress)
    torch.cuda.synchronize()
    tv, ti = tv.cpu(), ti.cpu().long()
    assert ti.min() >= 0 and ti.max() < V, (what, "a pick outside the vocabulary")
    want_i = torch.from_numpy(order)
    assert torch.equal(ti, want_i), (what, (ti != want_i).nonzero()[:5].tolist(), ti[ti != want_i][:5].tolist(), want_i[ti != want_i][:5].tolist())
    want = torch.where(torch.from_numpy(np.take_along_axis(mask, order, 1)), torch.tensor(NEG, dtype=F64), s64.gather(1, want_i))
    inf = want == NEG
    assert torch.equal(tv == NEG, inf), (what, "-inf slots")
    if (~inf).any():
        margin, _ = margin_of(s64, s32, what)
        err = (tv.to(F64) - want)[~inf].abs().max().item()
        report(f"beam_topk {what} {str(raw.dtype)[6:]} R={R} V={V} K={K_} paths={sorted(set(p[0] for p in paths))}", margin, err)
        assert err <= margin, (what, err, margin)
    return tv, ti, paths


def some_bans(R, V, n, seed, also=None):
    b = torch.randint(0, V, (R, n), generator=rng(seed), dtype=torch.int32)
    b[:, n // 2] = -1
    if also is not None:
        b[:, 0] = also.to(torch.int32)
    return b


# ------------------------------------------------------------------------------------------ beam_topk: tests
VBIG, LDBIG = 50267, 50272


@gpu
@pytest.mark.parametrize("dtype,R", [(F32, 5), (BF16, 5), (F32, 80), (BF16, 80)])
def test_topk_wave_pick(K, dtype, R):
    raw = (torch.randn(R, VBIG, generator=rng(11 + R)) * 3).to(dtype)
    bs = torch.randn(R, generator=rng(12))
    bans = some_bans(R, VBIG, 6, 13, also=raw.to(F64).argmax(1) * (torch.arange(R) % 2) + (torch.arange(R) % 2 - 1))   # odd rows ban their arg-max
    for K_ in (1, 10, 16):
        if dtype == BF16 and K_ > 1:
            top = raw.to(F64).topk(K_, dim=1).values
            assert bool((top[:, 1:] == top[:, :-1]).any()), "the bf16 input must hold exact ties inside its top K"
        check_topk(K, "wave-pick", raw, K_, bs=bs, bans=bans, suppress=True, ldl=LDBIG, path="wave")


def planted(R, V, n, dtype, seed):
    """rows whose maximum 9.0 appears at n scattered indices, everything else strictly below it"""
    g = rng(seed)
    raw = (torch.randn(R, V, generator=g) * 2).clamp(max=8.0).to(dtype)
    where = []
    for r in range(R):
        idx = torch.randperm(V, generator=g)[:n].sort().values
        raw[r, idx] = 9.0
        where.append(idx)
    assert bool((raw.to(F64) == 9.0).sum(1).eq(n).all())
    return raw, where


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("K_", [10, 300])
def test_topk_block_pick(K, dtype, K_):
    R = 3
    raw, where = planted(R, VBIG, 600, dtype, 21)
    bans = torch.stack([w[torch.tensor([0, 3, 4, 299, 599])] for w in where]).to(torch.int32)        # five of the planted ones
    tv, ti, paths = check_topk(K, "block-pick", raw, K_, bans=bans, eos=VBIG + 5, suppress=True, ldl=LDBIG, path="block")
    for r in range(R):
        keep = [int(t) for t in where[r].tolist() if t not in bans[r].tolist()]
        assert ti[r].tolist() == keep[:K_], r                                   # the first K unbanned planted indices, ascending


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_topk_wave_pick_many_ties(K, dtype):
    """200 copies of the maximum: cnt <= 256, so wave 0 picks with up to four tied candidates in one lane (candidates c, c + 64, ...)"""
    raw, where = planted(3, VBIG, 200, dtype, 27)
    bans = torch.stack([w[torch.tensor([0, 1, 7])] for w in where]).to(torch.int32)
    for K_ in (10, 16):
        tv, ti, _ = check_topk(K, "wave-pick-ties", raw, K_, bans=bans, ldl=LDBIG, path="wave")
        for r in range(3):
            keep = [int(t) for t in where[r].tolist() if t not in bans[r].tolist()]
            assert ti[r].tolist() == keep[:K_], r


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_topk_overflow(K, dtype):
    raw, where = planted(3, VBIG, 1500, dtype, 22)
    bans = torch.stack([w[:2] for w in where]).to(torch.int32)
    tv, ti, _ = check_topk(K, "overflow", raw, 10, bans=bans, bs=torch.tensor([0.5, -1.0, 2.0]), ldl=LDBIG, path="overflow")
    assert ti.tolist() == [w[2:12].tolist() for w in where]


@gpu
def test_topk_minus_inf_threshold(K):
    raw = torch.randn(4, 40, generator=rng(23))
    check_topk(K, "V=40", raw, 10, bs=torch.randn(4, generator=rng(24)), bans=torch.tensor([[3, -1]] * 4, dtype=torch.int32), path="fallback")
    check_topk(K, "V=40", raw.to(BF16), 10, path="fallback")
    V, K_ = 5000, 10
    raw = torch.randn(2, V, generator=rng(25)) * 3
    keep = torch.stack([torch.randperm(V, generator=rng(26 + r))[:K_ - 1] for r in range(2)])
    bans = torch.stack([torch.tensor([t for t in range(V) if t not in set(keep[r].tolist())], dtype=torch.int32) for r in range(2)])
    assert bans.shape == (2, V - (K_ - 1))
    tv, ti, _ = check_topk(K, "all-but-9-banned", raw, K_, bans=bans, path="fallback")
    for r in range(2):
        assert sorted(ti[r, :K_ - 1].tolist()) == sorted(keep[r].tolist())
        assert tv[r, K_ - 1] == NEG and int(ti[r, K_ - 1]) == int(bans[r].min())        # -inf, lowest remaining token id


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_topk_thread_threshold(K, dtype):
    raw = (torch.randn(5, VBIG, generator=rng(31)) * 3).to(dtype)
    for K_ in (17, 32, 64):
        _, _, paths = check_topk(K, "thread-threshold", raw, K_, bs=torch.randn(5, generator=rng(32)), bans=some_bans(5, VBIG, 4, 33),
                                 suppress=True, ldl=LDBIG)
        assert all(p[0] in ("wave", "block") for p in paths), paths


@gpu
def test_topk_scalar_walk(K):
    R, V, ldl = 5, VBIG, VBIG + 2
    raw = torch.randn(R, V, generator=rng(41)) * 3
    raw[1, V - 1] = 20.0; raw[3, V - 2] = 20.0                                 # maxima in the last elements (row 3: in the V % 4 tail)
    flat = torch.full((R * ldl + 1,), PAD_LOGIT).cuda()
    view = flat[1:].view(R, ldl)
    view[:, :V] = raw.cuda()
    align = [(view.data_ptr() + r * ldl * 4) % 16 for r in range(R)]
    assert 0 in align and any(a != 0 for a in align), align                     # both row walks in one launch
    assert view.data_ptr() % 16 == 4 and align[3] == 0
    check_topk(K, "odd-ldl", raw, 10, bs=torch.randn(R, generator=rng(42)), bans=some_bans(R, V, 4, 43), suppress=True, dev_logits=view)
    check_topk(K, "odd-ldl", raw, 17, dev_logits=view)
    raw = torch.randn(3, 1027, generator=rng(44)) * 3
    raw[0, 1026] = 15.0; raw[1, 1024] = 15.0
    check_topk(K, "V%4=3", raw, 10, bans=torch.tensor([[1026], [5], [-1]], dtype=torch.int32), ldl=1028)
    check_topk(K, "V%4=3", raw.to(BF16), 10, ldl=1032)


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_topk_bans_and_suppression(K, dtype):
    R, V = 6, VBIG
    raw = (torch.randn(R, V, generator=rng(51)) * 3).to(dtype)
    am = raw.to(F64).argmax(1).to(torch.int32)
    bans = torch.full((R, 6), -1, dtype=torch.int32)
    bans[:, 1] = am                                                             # the arg-max
    bans[0, 0] = V; bans[1, 0] = V + 1000; bans[2, 0] = 2 ** 31 - 1              # == V, above V: the padding columns stay out of reach
    bans[3, 2] = am[3]; bans[3, 3] = 77; bans[3, 4] = 77                        # duplicates
    bans[4, 5] = V - 1; bans[5, 0] = 0
    eos = int(raw[0].to(F64).topk(2).indices[1])                                 # row 0's runner-up
    a = check_topk(K, "bans", raw, 10, bs=torch.randn(R, generator=rng(52)), bans=bans, eos=eos, suppress=True, ldl=LDBIG)
    assert int(a[1][0, 0]) not in (int(am[0]), eos)
    plain = check_topk(K, "bans", raw, 10, bans=bans, eos=eos, suppress=False, ldl=LDBIG)
    for out_eos in (V, V + 3, -1):                                               # an EOS outside the vocabulary suppresses nothing
        b = check_topk(K, "bans", raw, 10, bans=bans, eos=out_eos, suppress=True, ldl=LDBIG)
        assert torch.equal(b[0], plain[0]) and torch.equal(b[1], plain[1])


def forced_want(V, K_, forced, base):
    rest = [t for t in range(K_ + 1) if t != forced][:K_ - 1]
    return [forced] + [t if t < V else -1 for t in rest], [base] + [NEG] * (K_ - 1)


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_topk_slow_kernel(K, dtype):
    V, K_ = 2048, 1025                                                           # K > 1024: beam_topk_kernel without a forced token
    raw = (torch.randn(2, V, generator=rng(61)) * 3).to(dtype)
    bans = some_bans(2, V, 8, 62, also=raw.to(F64).argmax(1))
    check_topk(K, "slow", raw, K_, bs=torch.tensor([0.25, -3.0]), bans=bans, eos=5, suppress=True)
    bs = torch.tensor([0.0, -2.5], dtype=F32)
    for forced, scores in ((0, None), (V - 1, None), (7, bs), (V - 1, bs)):
        tv, ti = K.beam_topk(padded(raw, V + 8).cuda(), V, 6, beam_scores=None if scores is None else scores.cuda(), bans=bans.cuda(), eos=5,
                             suppress_eos=True, forced_token=forced)
        for r in range(2):
            wi, wv = forced_want(V, 6, forced, 0.0 if scores is None else float(scores[r]))
            assert ti[r].tolist() == wi and tv[r].tolist() == wv, (forced, r, ti[r].tolist(), tv[r].tolist())


@gpu
def test_topk_refusals(K):
    from vacnic_amd import _lib
    lg = torch.zeros(2, 64, device="cuda")
    tv = torch.zeros(2, 4, device="cuda"); ti = torch.zeros(2, 4, device="cuda", dtype=torch.int32)
    with pytest.raises(ValueError, match="bad V/ldl/K"):
        K.beam_topk(lg, 64, 65)
    with pytest.raises(ValueError, match="bad V/ldl/K"):
        K.beam_topk(lg, 65, 4)                                                  # ldl = 64 < V
    for args in ((lg.data_ptr(), None, ti.data_ptr()), (lg.data_ptr(), tv.data_ptr(), None), (None, tv.data_ptr(), ti.data_ptr())):
        st = _lib.lib.vacnic_beam_topk(args[0], None, None, 0, 2, 0, -1, args[1], args[2], 2, 64, 64, 4, 1, K._stream())
        assert st == 1 and b"null operand" in _lib.lib.vacnic_last_error_string()
    torch.cuda.synchronize()
    assert bool((tv == 0).all())


# ------------------------------------------------------------------------------------------ lmhead_topk
def lm_geometry(V):
    """(tpw, G, columns per workgroup) of lmhead_part_kernel: at most 512 workgroups of tpw 16-column tiles each"""
    nt = (V + 15) // 16
    tpw = max(1, (nt + 511) // 512)
    return tpw, (nt + tpw - 1) // tpw, tpw * 16


def lm_inputs(V, d, R, seed, ldw=None, bias=True, scores=True):
    g = rng(seed)
    Vp, ldw = (V + 7) // 8 * 8, ldw or d
    emb = torch.zeros(Vp, ldw, dtype=BF16)
    emb[:, :d] = (torch.randn(Vp, d, generator=g) * 0.5).to(BF16)
    h = torch.randn(R, d, generator=g).to(BF16)
    return dict(V=V, d=d, R=R, Vp=Vp, emb=emb, h=h, bias=torch.randn(V, generator=g) * 0.1 if bias else None,
                bs=torch.randn(R, generator=g) if scores else None)


def check_lmhead(K, what, t, K2, *, bans=None, eos=2, suppress=False, want_logits=True, expect=None):
    """vacnic_lmhead_topk on the inputs t against float64 h @ emb.T + bias -> log_softmax -> processors -> + beam score."""
    V, d, R, Vp = t["V"], t["d"], t["R"], t["Vp"]
    emb_d = t["emb"].cuda()[:, :d]                                              # stride(0) = ldw
    h_d = t["h"].cuda()
    bias_d = None if t["bias"] is None else t["bias"].cuda()
    bs_d = None if t["bs"] is None else t["bs"].cuda()
    bans_d = None if bans is None else bans.cuda()
    kw = dict(bias=bias_d, beam_scores=bs_d, bans=bans_d, eos=eos, suppress_eos=suppress)
    lg = torch.full((R, Vp + 8), 7.0, device="cuda", dtype=F32)
    tv, ti = K.lmhead_topk(h_d, emb_d, V, K2, logits=lg, **kw)
    tv_b, ti_b = K.lmhead_topk(h_d, emb_d, V, K2, logits=torch.empty_like(lg), **kw)
    tv_n, ti_n = K.lmhead_topk(h_d, emb_d, V, K2, **kw)                         # without the logits output
    bt_v, bt_i = K.beam_topk(lg, V, K2, beam_scores=bs_d, bans=bans_d, eos=eos, suppress_eos=suppress)
    gm = torch.empty((R, Vp), device="cuda", dtype=F32)
    K.gemm(h_d, emb_d, R, V, d, bias=bias_d, out=gm, ldw=emb_d.stride(0), ldo=Vp, out_mode=1)
    torch.cuda.synchronize()
    assert torch.equal(tv, tv_b) and torch.equal(ti, ti_b), (what, "two calls differ")
    assert torch.equal(tv, tv_n) and torch.equal(ti, ti_n), (what, "the logits output changes the result")
    assert torch.equal(ti, bt_i), (what, "picks differ from beam_topk on the logits written out", ti.tolist(), bt_i.tolist())
    assert bool((lg[:, V:] == 7.0).all()), (what, "logits written beyond V")
    tv, ti, lg, gm = tv.cpu(), ti.cpu().long(), lg.cpu()[:, :V], gm.cpu()[:, :V]
    # ---- float64 reference
    b64 = torch.zeros(V, dtype=F64) if t["bias"] is None else t["bias"].to(F64)
    s64 = torch.zeros(R, dtype=F64) if t["bs"] is None else t["bs"].to(F64)
    l64 = t["h"].to(F64) @ t["emb"][:V, :d].to(F64).t() + b64
    l32 = t["h"].to(F32) @ t["emb"][:V, :d].to(F32).t() + b64.to(F32)
    m_log, _ = margin_of(l64, gm, what)
    err = (lg.to(F64) - l64).abs().max().item()
    report(f"lmhead_topk logits {what} V={V} d={d} R={R}", m_log, err)
    assert err <= m_log, (what, "logits", err, m_log)
    sc64 = torch.log_softmax(l64, -1) + s64[:, None]
    sc32 = torch.log_softmax(l32, -1) + s64.to(F32)[:, None]
    m_sc, _ = margin_of(sc64, sc32, what)
    mask = torch.from_numpy(ban_mask(R, V, bans, eos, suppress))
    assert ti.min() >= 0 and ti.max() < V and not bool(mask.gather(1, ti).any()), (what, "a banned / suppressed / out-of-range pick")
    assert all(len(set(row)) == K2 for row in ti.tolist()), (what, "a token picked twice")
    got64 = sc64.gather(1, ti)
    err = (tv.to(F64) - got64).abs().max().item()
    report(f"lmhead_topk scores {what} V={V} d={d} R={R} K2={K2}", m_sc, err)
    assert err <= m_sc, (what, "scores", err, m_sc)
    assert bool((tv[:, 1:] <= tv[:, :-1]).all()), (what, "scores not sorted")
    kth = sc64.masked_fill(mask, NEG).topk(K2, dim=1).values[:, -1:]
    assert bool((got64 >= kth - 2 * m_sc).all()), (what, "a pick below the K2-th best float64 score", (kth - got64).max().item(), m_sc)
    if expect is not None:
        assert ti.tolist() == expect, (what, ti.tolist(), expect)
    return tv, ti


# (V, d, R, K2, ldw - d, bias, beam scores, bans, suppress): what it is there for
LM_CASES = [
    (17, 8, 1, 1, 0, False, False, False, False),        # tpw 1, second workgroup of one column; KS 2 with one cut K step (waves 1-3 idle)
    (256, 72, 5, 10, 0, True, True, True, True),         # KS 2, nst = 3: wave 3 idle, the third K step cut at k = 72
    (2049, 256, 8, 18, 0, True, True, True, False),      # KS 2 at its upper edge (d = 256), last workgroup of one column, K2 = 18
    (8192, 264, 5, 10, 0, True, False, True, True),      # KS 8 at its lower edge (d = 264, nst = 9), tpw 1 at its upper edge (512 workgroups)
    (8193, 264, 1, 10, 0, False, True, True, False),     # tpw 2; the last workgroup has a single tile (t_lo + 1 < t_hi false) of one column
    (8193, 72, 8, 1, 0, True, True, False, True),        # tpw 2 with KS 2, K2 = 1
    (50265, 1024, 5, 10, 0, True, True, True, True),     # tpw 7, G = 449, KS 8 full: the production shape
    (50265, 1024, 8, 18, 0, True, True, True, False),    # R = 8 (both row passes of every wave), K2 = 18: the last K2 below 64 KiB of merge LDS
    (2049, 1024, 5, 10, 8, True, True, True, True),      # ldw = d + 8
    (256, 8, 5, 18, 8, False, False, False, False),      # every switch off, ldw > d at KS 2
    (17, 256, 8, 10, 0, True, True, True, True),         # K2 = 10 of 17 tokens from two workgroups
    (50265, 72, 1, 18, 0, False, True, True, True),      # tpw 7 with a cut K step, one row
]


@gpu
@pytest.mark.parametrize("case", LM_CASES, ids=lambda c: "V%d-d%d-R%d-K%d" % c[:4])
def test_lmhead_topk_matches_float64(K, case):
    V, d, R, K2, extra, bias, scores, with_bans, suppress = case
    t = lm_inputs(V, d, R, seed=V + d + R, ldw=d + extra, bias=bias, scores=scores)
    bans = None
    if with_bans:
        top = (t["h"].to(F64) @ t["emb"][:V, :d].to(F64).t()).topk(min(3, V), dim=1).indices
        bans = torch.full((R, 5), -1, dtype=torch.int32)
        bans[:, 0] = top[:, 0]; bans[:, 3] = top[:, -1]                          # the best and the third-best token
        bans[:, 4] = (torch.arange(R) * 97) % V
    check_lmhead(K, "grid", t, K2, bans=bans, suppress=suppress)


def plant_rows(t, cols, scales):
    """embedding rows `cols` = 0.5 * scale everywhere and hidden rows made positive: those columns' logits dominate every other one"""
    t["h"] = t["h"].abs() + torch.tensor(0.25, dtype=BF16)
    for c, s in zip(cols, scales):
        t["emb"][c, :t["d"]] = torch.tensor(0.5 * s, dtype=BF16)
    return t


@gpu
def test_lmhead_merge_list_exhaustion(K):
    """the K2 best all lie in ONE workgroup's 112 columns (2 K2 scaled copies of one row, distinct scales): the merge walks that list
    to its end (hp == K2) while every other list keeps its head."""
    V, d, R, K2 = 50265, 1024, 5, 10
    tpw, G, ncol = lm_geometry(V)
    assert (tpw, G, ncol) == (7, 449, 112)
    c_lo = 3 * ncol
    cols = [c_lo + 5 * i for i in range(2 * K2)]
    assert cols[-1] < c_lo + ncol
    scales = [1.0 + ((7 * i) % 20) / 32.0 for i in range(2 * K2)]                # distinct, exact in bf16
    t = plant_rows(lm_inputs(V, d, R, seed=71), cols, scales)
    order = [c for _, c in sorted(zip(scales, cols), reverse=True)][:K2]
    check_lmhead(K, "one-list", t, K2, expect=[order] * R)


@gpu
def test_lmhead_ties_across_workgroups_and_range_edge_bans(K):
    """identical embedding rows in different workgroups' column ranges tie exactly: lowest token ids first, banned ones skipped.  The
    planted columns sit at c_lo, at c_lo + ncol - 1 and at V - 1, every row bans another subset, and -1 / V / > V entries ban nothing."""
    V, d, R, K2 = 50265, 256, 8, 10
    tpw, G, ncol = lm_geometry(V)
    cols = [0, ncol - 1, ncol, 5 * ncol - 1, 5 * ncol, 5 * ncol + 1, 200 * ncol + 17, 300 * ncol, (G - 1) * ncol, V - 2, V - 1, 7 * ncol + 3,
            9 * ncol - 1, 100 * ncol]
    cols = sorted(cols)
    assert V - 1 - (G - 1) * ncol < ncol and len(set(cols)) == len(cols) >= K2 + 4
    t = plant_rows(lm_inputs(V, d, R, seed=72, bias=False), cols, [1.0] * len(cols))
    bans = torch.full((R, 6), -1, dtype=torch.int32)
    bans[:, 4] = V; bans[:, 5] = V + 77
    bans[0, 0] = cols[0]                                                         # c_lo of workgroup 0
    bans[1, 0] = ncol - 1; bans[1, 1] = ncol                                     # the last column of one range, the first of the next
    bans[2, 0] = V - 1; bans[2, 1] = (G - 1) * ncol                              # the last valid column, c_lo of the last workgroup
    bans[3, :3] = torch.tensor(cols[:3], dtype=torch.int32)
    bans[4, 2] = 5 * ncol - 1; bans[5, 3] = 5 * ncol; bans[6, 0] = cols[1]; bans[6, 1] = cols[1]
    expect = [[c for c in cols if c not in bans[r].tolist()][:K2] for r in range(R)]
    check_lmhead(K, "ties", t, K2, bans=bans, expect=expect)
    expect = [[c for c in cols if c not in bans[r].tolist() and c != cols[2]][:K2] for r in range(R)]
    check_lmhead(K, "ties+eos", t, K2, bans=bans, eos=cols[2], suppress=True, expect=expect)


@gpu
def test_lmhead_merge_lds_above_64k(K):
    """G x K2 x 8 bytes of dynamic LDS in the merge: 449 x 32 x 8 = 114944 and 449 x 45 x 8 = 161640 need the raised limit, K2 >= 46
    does not fit 160 KiB and is refused by the predicate the library exports."""
    from vacnic_amd import _lib
    V, d, R = 50265, 1024, 5
    sup = lambda k2: int(_lib.lib.vacnic_lmhead_topk_supported(R, V, d, k2))
    assert [sup(k) for k in (1, 18, 19, 32, 45, 46, 64, 65)] == [1, 1, 1, 1, 1, 0, 0, 0]
    other = lambda v, k2: int(_lib.lib.vacnic_lmhead_topk_supported(R, v, d, k2))
    assert [other(8192, 39), other(8192, 40), other(8193, 64)] == [1, 0, 1]          # G = 512: 512 x 40 x 8 = 160 KiB + the static arrays
    assert int(_lib.lib.vacnic_lmhead_topk_supported(9, V, d, 10)) == 0 and int(_lib.lib.vacnic_lmhead_topk_supported(R, V, 1032, 10)) == 0
    t = lm_inputs(V, d, R, seed=73)
    bans = torch.full((R, 3), -1, dtype=torch.int32)
    bans[:, 1] = (t["h"].to(F64) @ t["emb"][:V].to(F64).t()).argmax(1)
    check_lmhead(K, "K2=32", t, 32, bans=bans, suppress=True)
    check_lmhead(K, "K2=45", t, 45, bans=bans)
    for k2 in (46, 64):                                                          # the smallest and the largest K2 that must be refused here
        with pytest.raises(_lib.VacnicError, match="LDS"):
            K.lmhead_topk(t["h"].cuda(), t["emb"].cuda(), V, k2)
    torch.cuda.synchronize()


def tiny_generation_model():
    from vacnic_amd import synthetic
    from vacnic_amd.config import ClipVisionConfig, VacnicConfig
    from vacnic_amd.training import build_models
    cfg = VacnicConfig(d_model=768, encoder_layers=1, decoder_layers=1, encoder_attention_heads=12, decoder_attention_heads=12,
                       encoder_ffn_dim=3072, decoder_ffn_dim=3072, enc_fusion_layer=[0], dim_common=768, clip_width=768, dropout=0.0)
    assert cfg.vocab_size == 50267                                                # 3142 tiles -> G = 449, as at V = 50265
    vcfg = ClipVisionConfig(width=128, layers=1, patch_size=16, image_size=32, output_dim=64)
    sd = synthetic.make_state_dict(synthetic.mmbart_param_shapes(cfg), seed=1)
    sd["model.shared.weight"] = sd["model.shared.weight"] * synthetic.GEN_SHARPEN
    model, _, _ = build_models(cfg, vcfg, init="synthetic",
                               state_dicts=(sd, synthetic.make_state_dict(synthetic.guide_bart_param_shapes(cfg), seed=2),
                                            synthetic.make_state_dict(synthetic.clip_visual_param_shapes(vcfg), seed=4, std=0.05)))
    return cfg, sd, model


@gpu
def test_decode_session_wide_beams_take_a_supported_tail(K):
    """DecodeSession asks the library's predicate: 16 beams at the real vocabulary (16 rows: not the fused tail's shape) run the
    GEMM -> vacnic_beam_topk chain, 4 beams the fused tail; both give the oracle's caption."""
    from oracle import vacnic_oracle as O
    from vacnic_amd import _lib, synthetic
    cfg, sd, model = tiny_generation_model()
    batch = synthetic.make_batch(cfg, 1, S=24, T=8, F=2, seed=9, image_size=32)
    img = synthetic._normal("img_cls", (1, 768), 1.0, 3)
    src = batch["article_ids"]; omask = O.create_src_mask_bart(src)
    okw = dict(face_features=batch["face_emb"], face_mask=O.create_src_mask_bart(batch["face_emb"][:, :, -1]),
               name_ids=batch["names_art_ids"], name_mask=O.create_src_mask_bart(batch["names_art_ids"]))
    dev = {k: v.cuda() for k, v in batch.items()}
    mask, _ = K.prep_ids(dev["article_ids"], 1)
    nmask, _ = K.prep_ids(dev["names_art_ids"], 1)
    for nb, fused in ((16, False), (4, True)):
        model.__dict__.pop("_decode_sessions", None)
        kw = dict(input_ids=dev["article_ids"], attention_mask=mask, num_beams=nb, max_length=6, length_penalty=1.0,
                  image_features=img.cuda(), face_features=dev["face_emb"], face_mask=K.face_mask(dev["face_emb"]),
                  name_ids=dev["names_art_ids"], name_mask=nmask, add_ner_ffn=True)
        got = model.generate(**kw)
        (ses,) = model._decode_sessions.values()
        assert ses.fused_tail is fused
        assert ses.fused_tail == bool(_lib.lib.vacnic_lmhead_topk_supported(nb, model.V, model.emb16_pad.shape[1], 2 * nb))
        host = model.generate(device_beams=False, **kw)                             # the host-side scorer over the same kernels
        assert torch.equal(got, host), (nb, got.tolist(), host.tolist())
        assert got.shape[0] == 1 and 2 <= got.shape[1] <= 6 and int(got[0, 0]) == 2 and int(got.min()) >= 0 and int(got.max()) < model.V
        if fused:
            want = O.beam_search_decode(sd, cfg, src, omask, img, nb, 6, 1.0, forced_eos_token_id=2, **okw)
            assert torch.equal(got.cpu(), want), (nb, got.tolist(), want.tolist())


@gpu
def test_lmhead_refusals(K):
    from vacnic_amd import _lib
    V = 300
    mk = lambda R, d: (torch.zeros(R, d, dtype=BF16, device="cuda"), torch.zeros(304, d, dtype=BF16, device="cuda"))
    for R, d in ((9, 64), (5, 1032), (5, 12)):
        with pytest.raises(_lib.VacnicError):
            K.lmhead_topk(*mk(R, d), V, 4)
    h, emb = mk(5, 64)
    with pytest.raises(_lib.VacnicError):
        K.lmhead_topk(h, emb, V, 65)
    with pytest.raises(ValueError, match="forced token outside"):
        K.lmhead_topk(h, emb, V, 4, forced_token=V)
    tv = torch.zeros(5, 4, device="cuda"); ti = torch.zeros(5, 4, device="cuda", dtype=torch.int32)
    lg = torch.zeros(5, 304, device="cuda")
    nws = int(_lib.lib.vacnic_lmhead_topk_workspace(5, V, 4))
    ws = torch.zeros(nws, device="cuda")
    base = dict(stream=K._stream(), h=h.data_ptr(), emb=emb.data_ptr(), bias=None, beam_scores=None, bans=None, top_val=tv.data_ptr(),
                top_idx=ti.data_ptr(), R=5, V=V, d=64, ldw=64, ldl=304, n_ban=0, eos=2, suppress_eos=0, K2=4)
    with pytest.raises(_lib.VacnicError, match="computes no logits"):
        _lib.call_struct("vacnic_lmhead_topk", logits=lg.data_ptr(), workspace=ws.data_ptr(), workspace_floats=nws, forced_token=2, **base)
    with pytest.raises(ValueError, match="workspace of"):
        _lib.call_struct("vacnic_lmhead_topk", logits=None, workspace=ws.data_ptr(), workspace_floats=nws - 1, forced_token=-1, **base)
    with pytest.raises(ValueError, match="ldl < V"):
        _lib.call_struct("vacnic_lmhead_topk", logits=lg.data_ptr(), workspace=ws.data_ptr(), workspace_floats=nws, forced_token=-1,
                         **dict(base, ldl=V - 1))
    torch.cuda.synchronize()
    assert bool((tv == 0).all())


# ------------------------------------------------------------------------------------------ gather_rows
@gpu
def test_gather_rows_grid_stride_wrap(K):
    rows, row_bytes = 64, 320 * 1024                                             # 64 x 20480 chunks > 4096 blocks x 256 threads
    assert rows * (row_bytes // 16) > 4096 * 256
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, row_bytes // 4), generator=rng(81), dtype=torch.int32).cuda()
    idx = torch.randint(0, rows, (rows,), generator=rng(82))
    idx[:4] = torch.tensor([7, 7, 7, 0])                                         # duplicate source rows
    dst = torch.zeros_like(src)
    K.gather_rows(src, dst, idx.cuda(), rows, row_bytes)
    assert torch.equal(dst, src[idx.cuda()])


@gpu
def test_gather_rows_period_stride_and_fill(K):
    rows, period, stride_w, row_w = 12, 4, 96, 40                                # int32 words: 384-byte stride, 160-byte rows
    src = torch.arange(rows * stride_w, dtype=torch.int32).view(rows, stride_w).cuda()
    dst = torch.full_like(src, -5)
    perm = torch.tensor([3, 3, 0, 1])
    K.gather_rows(src, dst, perm.cuda(), rows, row_w * 4, row_stride_bytes=stride_w * 4, period=period)
    g = torch.tensor([(r // period) * period + int(perm[r % period]) for r in range(rows)]).cuda()
    assert torch.equal(dst[:, :row_w], src[g][:, :row_w]) and bool((dst[:, row_w:] == -5).all())
    for r_, b_ in ((0, 160), (rows, 0)):                                         # empty calls write nothing
        dst.fill_(-5)
        K.gather_rows(src, dst, perm.cuda(), r_, b_, row_stride_bytes=stride_w * 4, period=period)
        assert bool((dst == -5).all())
    with pytest.raises(ValueError, match="16-byte multiples"):
        K.gather_rows(src, dst, perm.cuda(), rows, 152, row_stride_bytes=stride_w * 4)
    with pytest.raises(ValueError, match="stride < row bytes"):
        K.gather_rows(src, dst, perm.cuda(), rows, 400, row_stride_bytes=stride_w * 4)
    with pytest.raises(ValueError, match="not a multiple of the period"):
        K.gather_rows(src, dst, perm.cuda(), 10, 160, row_stride_bytes=stride_w * 4, period=period)
    torch.cuda.synchronize()
    assert bool((dst == -5).all())


# ------------------------------------------------------------------------------------------ beam_init / beam_step: host model
VS, EOS, PAD = 40, 2, 1                                                          # the scripted vocabulary
_M = [np.array([v], dtype=np.uint64) for v in (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0xD6E8FEB86659FD93,
                                                0xA0761D6478BD642F, 0xE7037ED1A0B428DB)]


def _mix(x):
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * _M[1]
        x = (x ^ (x >> np.uint64(27))) * _M[2]
    return x ^ (x >> np.uint64(31))


def table_rows(c, seqs, pos):
    """next-token log-probabilities [R, VS] (fp32) as a function of (batch item, last two tokens, position): -q / 256 with
    q in 1 .. 4095, most of a row near -16 and a few tokens near 0 (like a trained model: it keeps the best 2 nb + 1 group scores
    apart); EOS is pulled towards 0 from position c['eos_from'] on."""
    R = len(seqs)
    u64 = lambda v: np.asarray(v, dtype=np.uint64)
    b = u64([r // c["nb"] for r in range(R)])
    t1 = u64([s[-1] for s in seqs]); t2 = u64([s[-2] if len(s) > 1 else 0 for s in seqs])
    with np.errstate(over="ignore"):
        key = _mix(u64([c["seed"]]) * _M[0] + b * _M[3] + t1 * _M[4] + t2 * _M[5] + u64([pos]) * _M[1])
        h = _mix(key[:, None] + u64(np.arange(VS))[None, :] * _M[2])
    u = (h >> np.uint64(11)).astype(np.float64) / 2.0 ** 53
    if pos >= c["eos_from"]:
        u[:, EOS] *= c["eos_boost"]
    q = 1 + np.floor(4094 * u ** c["shape"])
    if c["good"] is not None:
        # the long case: a fraction c['good'] of the tokens spread over -q / 256, q in 1 .. 3000, the rest packed into 3500 .. 4094, so
        # that the best five group scores stay apart for 511 positions
        u2 = (_mix(h + _M[3]) >> np.uint64(11)).astype(np.float64) / 2.0 ** 53
        q = np.where(u2 < c["good"], 1 + np.floor(3000 * u), 3500 + np.floor(595 * u))
    return (-q / 256.0).astype(np.float32)


def make_hyps(O, nb, lp, early):
    class Hyps(O._BeamHyps):
        """oracle._BeamHyps + counters: when the list fills, and which list index every eviction from a full list removes"""
        filled, evicted = False, ()

        def add(self, hyp, s):
            before = len(self.beams)
            score = s / (self._len(len(hyp)) ** self.lp)
            if before == self.n and score > self.worst:
                self.evicted = self.evicted + (sorted((sc, i) for i, (sc, _) in enumerate(self.beams + [(score, hyp)]))[0][1],)
            super().add(hyp, s)
            self.filled = self.filled or (before < self.n and len(self.beams) == self.n)
    return Hyps(nb, lp, early)


class HostBeams:
    """GenerationMixin.beam_search + BeamSearchScorer.process position by position: the loop body of oracle.beam_search_bookkeeping
    with its state exposed (test_host_lockstep_equals_oracle_bookkeeping pins the two against each other)."""

    def __init__(self, O, c):
        self.O, self.c, self.B, self.nb = O, c, c["B"], c["nb"]
        R = self.B * self.nb
        self.seqs = [[c["start"]] for _ in range(R)]
        self.scores = np.where(np.arange(R) % self.nb == 0, 0.0, -1e9).astype(np.float32)
        self.hyps = [make_hyps(O, self.nb, c["lp"], c["early"]) for _ in range(self.B)]
        self.done = [False] * self.B
        self.cur_len = 1
        self.src = list(range(R))
        self.ev = dict(two_eos=0, late_eos=0, distinct=True, staggered=False)

    def processed(self, lp):
        lp = lp.copy()
        for r, s in enumerate(self.seqs):
            for tok in self.O.banned_ngram_tokens(s, self.c["ngram"]):
                lp[r, tok] = NEG
            if self.cur_len < self.c["min_length"]:
                lp[r, EOS] = NEG
        return lp

    def step(self, lp):
        B, nb, c = self.B, self.nb, self.c
        was_done = list(self.done)
        sc = (self.processed(lp) + self.scores[:, None]).reshape(B, nb * VS)          # fp32, exact
        order = np.argsort(-sc, axis=1, kind="stable")[:, :2 * nb + 1]
        top = np.take_along_axis(sc, order, 1)
        seqs, scores, src = [], [], []
        for b in range(B):
            if self.done[b]:
                seqs += [self.seqs[b * nb] + [PAD]] * nb; scores += [0.0] * nb; src += [b * nb] * nb
                continue
            self.ev["distinct"] = self.ev["distinct"] and len(set(top[b].tolist())) == 2 * nb + 1
            chosen, n_eos = [], 0
            for rank in range(2 * nb):
                tok, s, row = int(order[b, rank] % VS), float(top[b, rank]), b * nb + int(order[b, rank] // VS)
                if tok == EOS:
                    if rank >= nb:
                        self.ev["late_eos"] += 1
                        continue
                    n_eos += 1
                    self.hyps[b].add(self.seqs[row], s)
                else:
                    chosen.append((s, tok, row))
                if len(chosen) == nb:
                    break
            self.ev["two_eos"] += n_eos >= 2
            self.done[b] = self.hyps[b].is_done(float(top[b].max()), self.cur_len)
            for s, tok, row in chosen:
                seqs.append(self.seqs[row] + [tok]); scores.append(s); src.append(row)
        self.ev["staggered"] = self.ev["staggered"] or (any(self.done) and not all(self.done))
        self.seqs, self.scores, self.src = seqs, np.asarray(scores, dtype=np.float32), src
        self.cur_len += 1
        return was_done

    def events(self):
        ev = dict(self.ev)
        ev["filled"] = any(h.filled for h in self.hyps)
        ev["evict_inner"] = sum(i < self.nb - 1 for h in self.hyps for i in h.evicted)
        return ev

    def finalize(self):
        """BeamSearchScorer.finalize as in oracle.beam_search_bookkeeping: the n-best lists, best first"""
        out = []
        for b in range(self.B):
            if not self.done[b]:
                for j in range(self.nb):
                    self.hyps[b].add(self.seqs[b * self.nb + j], float(self.scores[b * self.nb + j]))
            out.append([(float(s), list(q)) for s, q in reversed(sorted(self.hyps[b].beams, key=lambda x: x[0]))])
        return out


def run_host(O, c):
    host = HostBeams(O, c)
    while True:
        host.step(table_rows(c, host.seqs, host.cur_len))
        if all(host.done) or host.cur_len >= c["Lmax"]:
            return host


def case(nb, B, lp, early, ngram, min_length, Lmax, seed, start=0, eos_from=2, eos_boost=1e-3, shape=0.2, good=None, expect=()):
    return dict(nb=nb, B=B, lp=lp, early=early, ngram=ngram, min_length=min_length, Lmax=Lmax, seed=seed, start=start, eos_from=eos_from,
                eos_boost=eos_boost, shape=shape, good=good, expect=expect)


# seeds found by a host-only search: every position keeps its best 2 nb + 1 group scores pairwise distinct and the events in
# `expect` happen (both asserted below on the host reference)
ALL4 = ("filled", "evict_inner", "two_eos", "late_eos")
STEP_CASES = [
    case(1, 1, 1.0, False, 0, 0, 12, seed=5, start=2, eos_from=6, eos_boost=0.05, expect=("filled",)),
    case(2, 3, 2.0, False, 2, 3, 12, seed=1, start=2, expect=ALL4),
    case(5, 1, 2.0, False, 3, 0, 64, seed=5, expect=ALL4),                                  # 63 positions, evictions all along
    case(5, 3, 0.5, True, 0, 4, 12, seed=8, start=2, expect=ALL4 + ("staggered",)),
    # nb = 8 is the widest beam the kernel takes with the 2 nb candidates per row that beam search hands it (nb * K2 <= 128: both
    # candidate slots of every lane in use); nb = 16 runs with K2 <= 8 only: test_beam_step_sixteen_beams
    case(8, 1, 1.0, False, 4, 0, 12, seed=5, expect=ALL4),
    case(8, 3, 2.0, True, 0, 2, 12, seed=7, start=2, eos_from=4, expect=ALL4 + ("staggered",)),
    case(2, 1, 1.0, False, 3, 512, 512, seed=49, start=2, good=0.1),                          # 511 positions: tmp[8], sseq[.][512], long ban scans
    case(5, 1, 1.0, False, 1, 2, 12, seed=3, eos_from=3, eos_boost=0.01, expect=ALL4),
    case(2, 3, 0.5, True, 4, 0, 64, seed=4, start=2, eos_from=20, eos_boost=0.05, expect=("filled", "two_eos", "late_eos", "staggered")),
    case(1, 3, 2.0, True, 2, 0, 12, seed=5, eos_from=4, eos_boost=0.1, expect=("filled", "staggered")),
]


def case_id(c):
    return "nb%d-B%d-lp%s-%s-ng%d-min%d-L%d" % (c["nb"], c["B"], c["lp"], "early" if c["early"] else "full", c["ngram"], c["min_length"], c["Lmax"])


@pytest.mark.parametrize("c", STEP_CASES, ids=case_id)
def test_host_lockstep_equals_oracle_bookkeeping(c):
    """CPU: HostBeams is oracle.beam_search_bookkeeping (same captions, same n-best lists and scores) on the scripted table, keeps
    its best 2 nb + 1 group scores distinct in every position (torch.topk's tie order is unspecified) and meets the case's events."""
    from oracle import vacnic_oracle as O
    host = run_host(O, c)
    ev = host.events()
    assert ev["distinct"], "tied group scores inside the best 2 nb + 1"
    for name in c["expect"]:
        assert ev[name], (name, ev)
    pos = [0]

    def fn(seqs):
        pos[0] += 1
        return torch.from_numpy(table_rows(c, seqs, pos[0]))
    res, nbest = O.beam_search_bookkeeping(fn, c["B"], c["nb"], c["Lmax"], EOS, PAD, c["start"], length_penalty=c["lp"], early_stopping=c["early"],
                                           no_repeat_ngram_size=c["ngram"], min_length=c["min_length"], return_nbest=True)
    assert pos[0] == host.cur_len - 1
    assert nbest == host.finalize()


def test_step_cases_cover_every_event():
    want = {"filled", "evict_inner", "two_eos", "late_eos", "staggered"}
    assert want <= {e for c in STEP_CASES for e in c["expect"]}
    assert {c["nb"] for c in STEP_CASES} == {1, 2, 5, 8} and {c["B"] for c in STEP_CASES} == {1, 3}
    assert {c["lp"] for c in STEP_CASES} == {0.5, 1.0, 2.0} and {c["ngram"] for c in STEP_CASES} == {0, 1, 2, 3, 4}
    assert {c["Lmax"] for c in STEP_CASES} == {12, 64, 512} and {c["early"] for c in STEP_CASES} == {False, True}


# ------------------------------------------------------------------------------------------ beam_init / beam_step: device
def row_lists(lp, bans, scores, suppress, K2):
    """what vacnic_beam_topk hands to the step kernel: per row the best K2 of lp (bans / EOS at -inf) + score, (score desc, token asc)"""
    x = lp.copy()
    if bans is not None:
        for r, row in enumerate(bans.tolist()):
            for t in row:
                if t >= 0:
                    x[r, t] = NEG
    if suppress:
        x[:, EOS] = NEG
    s = x + scores[:, None]
    order = np.argsort(-s, axis=1, kind="stable")[:, :K2]
    return torch.from_numpy(np.take_along_axis(s, order, 1)), torch.from_numpy(order.astype(np.int32))


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def compare_state(O, st, host, was_done, prev_seqs, c, cur):
    """device state after vacnic_beam_step(cur) against the host reference after the same position"""
    B, nb, L = c["B"], c["nb"], c["Lmax"]
    torch.cuda.synchronize()
    seq = st.seq.cpu().numpy()
    live, prev = seq[cur & 1], seq[(cur - 1) & 1]
    for r, s in enumerate(host.seqs):
        assert live[r, :cur + 1].tolist() == s and bool((live[r, cur + 1:] == PAD).all()), (cur, r, live[r, :cur + 2].tolist(), s)
        assert prev[r, :cur].tolist() == prev_seqs[r], (cur, r, "the input histories changed")
    assert np.array_equal(bits(st.beam_scores.cpu().numpy()), bits(host.scores)), (cur, st.beam_scores.cpu().tolist(), host.scores.tolist())
    assert st.next_ids.cpu().tolist() == [s[-1] for s in host.seqs], cur
    assert st.src_idx.cpu().tolist() == host.src, (cur, st.src_idx.cpu().tolist(), host.src)
    assert st.done.cpu().tolist() == [int(d) for d in host.done], cur
    cnt, worst = st.hyp_cnt.cpu().tolist(), st.hyp_worst.cpu().numpy()
    hs, hl, hq = st.hyp_score.cpu().numpy(), st.hyp_len.cpu().numpy(), st.hyp_seq.cpu().numpy()
    for b, h in enumerate(host.hyps):
        assert cnt[b] == len(h.beams), (cur, b, cnt[b], len(h.beams))
        assert bits(worst[b:b + 1])[0] == bits(np.array([h.worst]))[0], (cur, b, worst[b], h.worst)
        for i, (s, q) in enumerate(h.beams):
            assert bits(hs[b, i:i + 1])[0] == bits(np.array([s]))[0], (cur, b, i, hs[b, i], s)
            assert hl[b, i] == len(q) and hq[b, i, :len(q)].tolist() == q, (cur, b, i, hl[b, i], hq[b, i, :len(q) + 1].tolist(), q)
    if st.bans is not None:
        bans = st.bans.cpu().numpy()
        for r, s in enumerate(host.seqs):
            want = [] if was_done[r // nb] else O.banned_ngram_tokens(s, c["ngram"])          # a finished item bans nothing
            assert sorted(bans[r, :len(want)].tolist()) == sorted(want) and bool((bans[r, len(want):] == -1).all()), (cur, r, bans[r, :len(want) + 2].tolist(), want)


@gpu
@pytest.mark.parametrize("c", STEP_CASES, ids=case_id)
def test_beam_step_lockstep(K, c):
    from oracle import vacnic_oracle as O
    B, nb, L = c["B"], c["nb"], c["Lmax"]
    R, K2 = B * nb, min(2 * nb, VS)
    st = K.beam_alloc(B, nb, L, VS, EOS, PAD, no_repeat_ngram_size=c["ngram"], early_stopping=c["early"], length_penalty=c["lp"])
    for t in (st.seq, st.beam_scores, st.done, st.hyp_cnt, st.hyp_len, st.next_ids, st.src_idx):
        t.fill_(77)                                                              # beam_init owns all of it
    K.beam_init(st, c["start"])
    host = HostBeams(O, c)
    torch.cuda.synchronize()
    assert st.seq[0].cpu().tolist() == [[c["start"]] + [PAD] * (L - 1)] * R
    assert np.array_equal(bits(st.beam_scores.cpu().numpy()), bits(host.scores)) and st.next_ids.cpu().tolist() == [c["start"]] * R
    assert st.done.cpu().tolist() == [0] * B and st.hyp_cnt.cpu().tolist() == [0] * B and st.hyp_worst.cpu().tolist() == [1e9] * B
    assert st.bans is None or bool((st.bans == -1).all())
    for cur in range(1, L):
        lp = table_rows(c, host.seqs, cur)
        tv, ti = row_lists(lp, None if st.bans is None else st.bans.cpu(), st.beam_scores.cpu().numpy(), cur < c["min_length"], K2)
        prev = host.seqs
        K.beam_step(st, tv.cuda(), ti.cuda(), cur)
        was_done = host.step(lp)
        compare_state(O, st, host, was_done, prev, c, cur)
        if all(host.done):
            break
    ev = host.events()
    assert ev["distinct"] and all(ev[name] for name in c["expect"]), ev
    assert all(host.done) or host.cur_len == L                                  # no position skipped
    assert c["min_length"] < L or host.cur_len == L == 512                      # the long case ran its 511 positions


def merge_reference(tv, ti, nb, V, eos):
    """the documented order of one batch item's candidates: (score desc, beam * V + token asc) without the unused entries (id < 0),
    the best 2 nb kept; EOS inside the first nb ranks finishes a hypothesis, the first nb other candidates continue."""
    K2 = len(tv[0])
    cand = sorted((-tv[j][k], j * V + ti[j][k]) for j in range(nb) for k in range(K2) if ti[j][k] >= 0)[:K2]
    hyps, chosen = [], []
    for rank, (neg, key) in enumerate(cand):
        if key % V == eos:
            if rank < nb:
                hyps.append((-neg, key // V))
        elif len(chosen) < nb:
            chosen.append((-neg, key % V, key // V))
    return hyps, chosen


@gpu
def test_beam_step_merges_ties_by_beam_then_token(K):
    B, nb, V, L, K2 = 2, 3, 50, 8, 6
    tv = [[[-1.0, -1.0, -2.0, -2.0, -3.0, -3.5], [-1.0, -1.0, -2.0, -2.5, NEG, NEG], [-1.0, NEG, NEG, NEG, NEG, NEG]],          # item 0
          [[-0.5, -1.5, -1.5, -2.0, -2.0, -4.0], [-1.5, -2.0, -2.0, -2.25, -5.0, NEG], [-1.5, -2.0, -6.0, -7.0, NEG, NEG]]]     # item 1
    ti = [[[EOS, 30, 5, 9, 11, 12], [5, 9, EOS, 4, 0, 1], [EOS, 0, 1, 3, 4, 5]],          # row 2: a forced-token row (one finite score)
          [[-1, 9, 30, 7, 8, 3], [5, EOS, 7, 6, 3, -1], [4, 7, 10, 11, 0, 1]]]            # -1: an unused entry, whatever its score
    st = K.beam_alloc(B, nb, L, V, EOS, PAD, length_penalty=1.0)
    K.beam_init(st, 0)
    K.beam_step(st, torch.tensor(tv, dtype=F32).view(B * nb, K2).cuda(), torch.tensor(ti, dtype=torch.int32).view(B * nb, K2).cuda(), 1)
    torch.cuda.synchronize()
    for b in range(B):
        hyps, chosen = merge_reference(tv[b], ti[b], nb, V, EOS)
        assert len(chosen) == nb and len({s for s, _, _ in chosen}) < nb                  # ties among the continuing beams
        rows = slice(b * nb, (b + 1) * nb)
        assert st.next_ids[rows].tolist() == [t for _, t, _ in chosen], (b, st.next_ids[rows].tolist(), chosen)
        assert st.src_idx[rows].tolist() == [b * nb + j for _, _, j in chosen], (b, st.src_idx[rows].tolist(), chosen)
        assert st.beam_scores[rows].tolist() == [s for s, _, _ in chosen]
        assert int(st.hyp_cnt[b]) == len(hyps) and st.hyp_score[b, :len(hyps)].tolist() == [s for s, _ in hyps]
        assert st.seq[1][rows, :2].tolist() == [[0, t] for _, t, _ in chosen]
    assert merge_reference(tv[0], ti[0], nb, V, EOS)[0] == [(-1.0, 0)] and int(st.hyp_cnt[1]) == 0


@gpu
def test_beam_step_sixteen_beams(K):
    """nb = 16: 16 waves, sseq[16][.], and (nb * K2 <= 128) at most K2 = 8 candidates per row, fewer than beam search needs: the kernel
    documents that the best K2 of the group are kept and that beams left without a candidate continue row b * nb with the pad token at
    -1e9.  Hand-written distinct scores, against merge_reference + that rule."""
    from oracle import vacnic_oracle as O
    B, nb, V, L, K2, start = 2, 16, 50, 16, 8, 7
    n = B * nb * K2
    tv = (-(1 + (np.arange(n) * 37) % 256) / 16.0).astype(np.float32).reshape(B, nb, K2)
    assert len(set(tv.reshape(-1).tolist())) == n
    tv = -np.sort(-tv, axis=2)                                                      # every row's list best first
    ti = (3 + (np.arange(n) * 11) % 40).astype(np.int32).reshape(B, nb, K2)
    best = np.argsort(-tv.reshape(B, -1), axis=1)
    ti.reshape(B, -1)[0, best[0, 2]] = EOS; ti.reshape(B, -1)[0, best[0, 5]] = EOS     # item 0: two EOS inside the best eight
    ti.reshape(B, -1)[1, best[1, 0]] = start                                       # item 1: its best beam repeats the start token
    st = K.beam_alloc(B, nb, L, V, EOS, PAD, no_repeat_ngram_size=2, length_penalty=1.0)
    K.beam_init(st, start)
    K.beam_step(st, torch.from_numpy(tv).view(B * nb, K2).cuda(), torch.from_numpy(ti).view(B * nb, K2).cuda(), 1)
    torch.cuda.synchronize()
    seq, bans = st.seq[1].cpu().numpy(), st.bans.cpu().numpy()
    for b in range(B):
        hyps, chosen = merge_reference(tv[b].tolist(), ti[b].tolist(), nb, V, EOS)
        assert len(hyps) == (2, 0)[b] and len(chosen) == K2 - len(hyps)
        chosen += [(-1e9, PAD, 0)] * (nb - len(chosen))
        rows = slice(b * nb, (b + 1) * nb)
        assert st.next_ids[rows].tolist() == [t for _, t, _ in chosen], (b, st.next_ids[rows].tolist(), chosen)
        assert st.src_idx[rows].tolist() == [b * nb + j for _, _, j in chosen]
        assert st.beam_scores[rows].tolist() == [float(np.float32(s)) for s, _, _ in chosen]
        assert int(st.hyp_cnt[b]) == len(hyps) and st.hyp_score[b, :len(hyps)].tolist() == [s for s, _ in hyps]
        assert st.hyp_seq[b, :len(hyps), 0].tolist() == [start] * len(hyps) and st.hyp_len[b, :len(hyps)].tolist() == [1] * len(hyps)
        for j, (_, t, _) in enumerate(chosen):
            r = b * nb + j
            assert seq[r].tolist() == [start, t] + [PAD] * (L - 2), r
            want = O.banned_ngram_tokens([start, t], 2)
            assert bans[r, :len(want)].tolist() == want and bool((bans[r, len(want):] == -1).all()), (r, bans[r, :3].tolist(), want)
    assert O.banned_ngram_tokens([start, start], 2) == [start] and int(st.next_ids[nb]) == start


@gpu
def test_beam_step_refusals(K):
    from vacnic_amd import _lib

    def step(nb, K2, cur, L, B=1):
        st = K.beam_alloc(B, nb, min(L, 600), VS, EOS, PAD)
        st.st.Lmax = L
        K.beam_step(st, torch.zeros(B * nb, K2, device="cuda"), torch.zeros(B * nb, K2, device="cuda", dtype=torch.int32), cur)
    for nb, K2 in ((17, 2), (16, 9), (16, 32), (2, 65)):
        with pytest.raises(_lib.VacnicError, match="nb <= 16"):
            step(nb, K2, 1, 12)
    for cur, L in ((0, 12), (12, 12), (1, 513)):
        with pytest.raises(ValueError, match="outside"):
            step(2, 4, cur, L)
    torch.cuda.synchronize()
