"""GPU: vacnic_sample_step against the host model of tests/test_sample.py (written from the header comment alone).

What is exact and what carries a bound:
  * processors, the temperature division, the top-k threshold and count, u: no rounding is involved -> equality.
  * top-p: the kernel sums integer masses q = rint(expf(z' - max) * 2^31).  The float64 mass e_v of the strictly larger tokens is a
    sum of at most V terms; a sum of V fp32 terms has worst-case relative error V * 2^-24 in any order, doubled for expf:
    eps = 2 * V * 2^-24.  Tokens with e_v < p - eps must be kept, tokens with e_v > p + eps dropped, in between either.
  * the draw: the chosen token's float64 CDF interval, widened by V * 2^-24 on both sides, contains u; at V <= 2048 the token equals
    the float64 choice in >= 95 % of 512 rows.
Shapes: V in {1, 7, 64, 1000, 1025, 2048, 50265} (one lane, part of a wave, one element per lane and one more, 2 and 50 per lane),
rows in {1, 3, 9, 512, 20000}; ldl > V with large garbage in the padding columns."""
import types

import numpy as np
import pytest
import torch

from test_sample import F32, chi2_quantile, host_choose, host_processors, host_u, host_warp

gpu = pytest.mark.gpu
EOS, PAD = 2, 1


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


_ROWS = {}


def make_logits(R, V, seed=0):
    """normal(0, 2) rows [R, ldl], ldl > V, 1e30 in the padding (a kernel that read it would always choose it).  Rows r % 4 == 1 are
    rounded to halves (large tie groups), rows r % 4 == 2 have a random third of their tokens banned (-inf), row R - 1 (R >= 4)
    keeps ONE finite token.  Cached: the tests share the inputs."""
    key = (R, V, seed)
    if key not in _ROWS:
        rng = np.random.default_rng([seed, R, V])
        ldl = (V + 8) // 8 * 8 + 8
        z = np.full((R, ldl), 1e30, F32)
        z[:, :V] = rng.normal(0, 2, size=(R, V)).astype(F32)
        z[1::4, :V] = np.round(z[1::4, :V] * 2) / 2
        ban = rng.random((R, V)) < 1 / 3
        ban[:, 0] = False
        ban[np.arange(R) % 4 != 2] = False
        z[:, :V][ban] = -np.inf
        if R >= 4:
            z[R - 1, :V] = -np.inf
            z[R - 1, V // 2] = -1.25
        _ROWS[key] = z
    return _ROWS[key]


def launch(K, z, V, *, T=1.0, top_k=0, top_p=1.0, seed=11, call=0, cur_len=1, Lmax=8, history=None, done=None, ngram=0,
           suppress_eos=False, forced=-1):
    R = z.shape[0]
    dev = "cuda"
    logits = torch.from_numpy(z).to(dev)
    params = K.sample_params(T, top_k, top_p, seed, call).to(dev)
    seq = torch.full((R, Lmax), PAD, dtype=torch.int32)
    if history is not None:
        seq[:, :cur_len] = torch.as_tensor(history, dtype=torch.int32)
    seq = seq.to(dev)
    done_t = (torch.zeros(R, dtype=torch.int32) if done is None else torch.as_tensor(done, dtype=torch.int32)).to(dev)
    next_ids = torch.full((R,), -7, dtype=torch.int64, device=dev)
    logp = torch.full((R, Lmax), 9.0, device=dev)
    kept = torch.full((R,), -7, dtype=torch.int32, device=dev)
    thr, mass, u = (torch.full((R,), 9.0, device=dev) for _ in range(3))
    K.sample_step(logits, V, params, seq, done_t, next_ids, cur_len, logp=logp, eos=EOS, pad=PAD, no_repeat_ngram_size=ngram,
                  suppress_eos=suppress_eos, forced_token=forced, kept=kept, thr=thr, mass=mass, u=u)
    torch.cuda.synchronize()
    o = types.SimpleNamespace(token=next_ids.cpu().numpy(), seq=seq.cpu().numpy(), done=done_t.cpu().numpy(), logp=logp.cpu().numpy(),
                              kept=kept.cpu().numpy(), thr=thr.cpu().numpy(), mass=mass.cpu().numpy(), u=u.cpu().numpy())
    assert np.array_equal(o.seq[:, cur_len], o.token) and np.array_equal(o.seq[:, cur_len + 1:], np.full((R, Lmax - cur_len - 1), PAD))
    return o


def warped(z, V, T):
    with np.errstate(invalid="ignore", over="ignore"):
        return (z[:, :V] / F32(T)).astype(F32) + F32(0.0)


@gpu
@pytest.mark.parametrize("V,R", [(1, 1), (7, 3), (1000, 9), (1025, 512), (50265, 9), (50265, 512)])
def test_top_k_threshold_and_count_are_exact(K, V, R):
    z = make_logits(R, V)
    for T in ((1.0, 0.5) if R <= 9 else (1.0,)):
        zp = warped(z, V, T)
        srt = np.sort(zp, axis=1)
        for k in (0, 1, 2, V // 3, V, V + 5):
            o = launch(K, z, V, T=T, top_k=k)
            thr = srt[:, V - k] if 1 <= k < V else np.full(R, -np.inf, F32)
            assert np.array_equal(o.thr, thr), (V, R, T, k)
            assert np.array_equal(o.kept, ((zp >= thr[:, None]) & np.isfinite(zp)).sum(1)), (V, R, T, k)
            chosen = zp[np.arange(R), o.token]
            assert (o.token >= 0).all() and (o.token < V).all() and np.isfinite(chosen).all() and (chosen >= thr).all(), (V, R, T, k)
            assert np.array_equal(o.mass, np.ones(R, F32))
            if k == 1:                                     # the top tie group: the token is one of the row maxima
                assert np.array_equal(chosen, srt[:, -1])


@gpu
@pytest.mark.parametrize("V,R", [(7, 512), (1000, 9), (1025, 9), (50265, 3)])
def test_top_p_keeps_what_the_float64_masses_say(K, V, R):
    z = make_logits(R, V, seed=1)
    eps = 2 * V * 2.0 ** -24
    for T in (0.5, 1.0, 2.0):
        zp = warped(z, V, T)
        for k in (0, max(1, V // 4)):
            ref = [host_warp(z[r, :V], T, k, 1.0) for r in range(R)]        # before-masses within the top-k survivors, shared by every p
            for p in (1.0, 0.9, 0.5, 1e-6):
                o = launch(K, z, V, T=T, top_k=k, top_p=p)
                for r in range(R):
                    w, tag = ref[r], (V, r, T, k, p)
                    alive = (zp[r] >= w["thr"]) & np.isfinite(zp[r])
                    got = (zp[r] >= o.thr[r]) & np.isfinite(zp[r])
                    assert int(o.kept[r]) == int(got.sum()) and got[o.token[r]], tag
                    assert not (got & ~alive).any(), tag                                     # nothing comes back after top-k
                    if p >= 1.0:
                        assert np.array_equal(got, alive) and o.thr[r] == w["thr"] and o.mass[r] == 1.0, tag
                        continue
                    assert o.thr[r] in zp[r], tag                                            # the kept set is {z' >= one of the row's values}
                    assert got[alive & (w["larger"] < p - eps)].all(), tag
                    assert not got[alive & (w["larger"] > p + eps)].any(), tag
                    assert abs(float(o.mass[r]) - w["p"][got].sum() * w["mass"]) <= eps + 2.0 ** -23, tag
                    if p == 1e-6:                                                            # the top tie group and nothing else
                        assert np.array_equal(got, zp[r] == zp[r][np.isfinite(zp[r])].max()), tag


@gpu
@pytest.mark.parametrize("V,R,equal", [(7, 512, True), (1000, 512, True), (2048, 512, True), (1025, 9, False), (50265, 9, False)])
def test_draw_replays_on_the_host(K, V, R, equal):
    z = make_logits(R, V, seed=2)
    for (T, k, p), (seed, call, cur) in (((1.0, 0, 1.0), (11, 0, 1)), ((1.5, max(1, V // 8), 0.8), (2 ** 63 + 12345, 2 ** 40 + 3, 5))):
        o = launch(K, z, V, T=T, top_k=k, top_p=p, seed=seed, call=call, cur_len=cur, history=np.full((R, cur), 7))
        miss = 0
        for r in range(R):
            m, u, u32 = host_u(seed, call, r, cur)
            assert o.u[r] == u32 and o.u[r].tobytes() == u32.tobytes(), (V, r)
            w = host_warp(z[r, :V], T, k, p)
            # the distribution the kernel drew from is over ITS kept set (top-p may differ from float64 inside the eps band)
            zp = w["zp"]
            got = (zp >= o.thr[r]) & np.isfinite(zp)
            q = np.where(got, np.exp(zp.astype(np.float64) - zp[got].max()), 0.0)
            q /= q.sum()
            tok, _ = host_choose(q, u)
            c = np.cumsum(q)
            t = int(o.token[r])
            assert got[t] and c[t] - q[t] - V * 2.0 ** -24 <= u <= c[t] + V * 2.0 ** -24, (V, r, t, tok, u)
            assert abs(float(o.logp[r, cur]) - np.log(q[t])) <= 1e-5, (V, r, float(o.logp[r, cur]), np.log(q[t]))
            miss += t != tok
        if equal:
            assert miss <= 0.05 * R, (V, miss)
        assert np.array_equal(o.logp[:, :cur], np.full((R, cur), 9.0, F32))              # only column cur_len is written


@gpu
def test_token_counts_follow_the_distribution(K):
    """20 000 rows of the same V = 64 logits in one launch: Pearson's chi-square of the token counts against the float64
    probabilities stays below the 1 - 1e-6 quantile of chi-square(kept - 1).  Deterministic given the seed.  The logits are spread
    evenly over [-2, 2] (shuffled), so the rarest token of the full distribution is still expected ~23 times and Pearson's statistic
    is in its chi-square regime."""
    V, R = 64, 20000
    row = np.random.default_rng(3).permutation(np.linspace(-2.0, 2.0, V)).astype(F32)
    z = np.full((R, V + 8), 1e30, F32)
    z[:, :V] = row
    for T, k, p in ((1.0, 0, 1.0), (1.0, 5, 1.0), (1.0, 0, 0.7), (0.7, 20, 0.9)):
        o = launch(K, z, V, T=T, top_k=k, top_p=p, seed=2024)
        w = host_warp(row, T, k, p)
        assert p >= 1.0 or np.abs(w["larger"] - p).min() > 2 * V * 2.0 ** -24          # no token inside the top-p rounding band
        counts = np.bincount(o.token, minlength=V)
        assert counts[~w["kept"]].sum() == 0, (T, k, p, np.nonzero(counts * ~w["kept"]))
        assert (o.kept == w["kept"].sum()).all() and (o.thr == w["thr"]).all()
        exp = w["p"][w["kept"]] * R
        assert exp.min() > 20
        chi2 = float((((counts[w["kept"]] - exp) ** 2) / exp).sum())
        limit = chi2_quantile(int(w["kept"].sum()) - 1)
        print(f"T={T} top_k={k} top_p={p}: kept {int(w['kept'].sum())} chi2 {chi2:.1f} limit {limit:.1f}")
        assert chi2 < limit, (T, k, p, chi2, limit)


@gpu
def test_processors_and_bookkeeping(K):
    V, R = 50, 512
    z = np.full((R, 56), 1e30, F32)
    z[:, :V] = np.random.default_rng(4).normal(0, 2, size=(R, V)).astype(F32)
    # forced token: chosen whatever u is, log-prob 0; forcing eos finishes the row
    for forced in (0, EOS, V - 1):
        o = launch(K, z, V, forced=forced, cur_len=2, history=np.full((R, 2), 9))
        assert (o.token == forced).all() and (o.logp[:, 2] == 0).all() and (o.done == (forced == EOS)).all() and (o.kept == 1).all()
        assert len(np.unique(o.u)) > R // 2
    # suppress_eos (MinLength): eos would take nearly every draw, and never appears
    ze = z.copy()
    ze[:, EOS] = 12.0
    o = launch(K, ze, V)
    assert (o.token == EOS).mean() > 0.9 and np.array_equal(o.done, (o.token == EOS).astype(np.int32))
    o = launch(K, ze, V, suppress_eos=True)
    assert (o.token != EOS).all() and (o.done == 0).all()
    for r in range(0, R, 37):
        w = host_warp(host_processors(ze[r, :V], eos=EOS, suppress_eos=True))
        assert int(o.kept[r]) == int(w["kept"].sum()) == V - 1 and abs(o.logp[r, 1] - np.log(w["p"][o.token[r]])) <= 1e-5
    # finished rows write pad and log-prob 0 and stay finished; the others are untouched by them
    done = (np.arange(R) % 3 == 0).astype(np.int32)
    o = launch(K, z, V, done=done)
    live = launch(K, z, V)
    assert (o.token[done == 1] == PAD).all() and (o.logp[done == 1, 1] == 0).all() and (o.done[done == 1] == 1).all()
    assert np.array_equal(o.token[done == 0], live.token[done == 0]) and np.array_equal(o.logp[done == 0], live.logp[done == 0])
    # NoRepeatNGram, size 2: history 2 5 9 5 -> after "5" came "9": 9 is banned.  Unbanned it would take > 50 % of the draws.
    zn = z.copy()
    zn[:, 9] = 10.0
    hist = np.tile(np.array([2, 5, 9, 5]), (R, 1))
    free = launch(K, zn, V, cur_len=4, history=hist)
    assert all(host_warp(zn[r, :V])["p"][9] > 0.5 for r in range(R)) and (free.token == 9).mean() > 0.5
    o = launch(K, zn, V, cur_len=4, history=hist, ngram=2)
    assert (o.token != 9).all()
    for r in range(0, R, 37):
        w = host_warp(host_processors(zn[r, :V], history=hist[r], ngram=2))
        assert int(o.kept[r]) == int(w["kept"].sum()) == V - 1 and abs(o.logp[r, 4] - np.log(w["p"][o.token[r]])) <= 1e-5
    # size 3 needs both previous tokens to match: "9 5" occurred nowhere before -> nothing banned; size 1 bans every seen token
    o3 = launch(K, zn, V, cur_len=4, history=hist, ngram=3)
    assert np.array_equal(o3.token, free.token)
    o1 = launch(K, zn, V, cur_len=4, history=hist, ngram=1)
    assert not np.isin(o1.token, [2, 5, 9]).any() and (o1.kept == V - 3).all()
    # a row without a finite logit ends with eos
    zi = np.full((3, 56), -np.inf, F32)
    o = launch(K, zi, V)
    assert (o.token == EOS).all() and (o.done == 1).all() and (o.kept == 0).all() and (o.logp[:, 1] == 0).all()


@gpu
def test_two_launches_give_identical_outputs(K):
    for V, R in ((50265, 9), (1025, 512)):
        z = make_logits(R, V, seed=5)
        a = launch(K, z, V, T=0.8, top_k=V // 5, top_p=0.9, seed=77, call=4)
        b = launch(K, z, V, T=0.8, top_k=V // 5, top_p=0.9, seed=77, call=4)
        for name in ("token", "seq", "done", "logp", "kept", "thr", "mass", "u"):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), (V, name)
        c = launch(K, z, V, T=0.8, top_k=V // 5, top_p=0.9, seed=77, call=5)
        assert not np.array_equal(a.u, c.u) and np.array_equal(a.thr, c.thr) and np.array_equal(a.kept, c.kept)
