"""CPU: sampling decode — the argument checks of generate(do_sample=True), the unchanged do_sample=False path, the status codes of
vacnic_sample_step, and the HOST MODEL of the kernel that the GPU tests import (tests/test_sample_gpu.py,
tests/test_generate_sample_gpu.py).

The host model is written from the comment at vacnic_sample_step in include/vacnic_hip.h alone: processors -> z' = z / T (fp32
IEEE division) -> top-k (k-th largest, ties kept) -> top-p (keep v iff the probability of the STRICTLY larger tokens is <= top_p) ->
u from Philox4x32-10 -> first kept token in ascending id whose inclusive cumulative probability exceeds u.  Probabilities are
float64 here; the kernel's are integers q = rint(expf(z' - max) * 2^31), so the GPU tests compare with the bounds their docstrings
derive, and exactly wherever no rounding is involved (top-k threshold and count, u, processors)."""
import math

import numpy as np
import pytest
import torch

F32, F64 = np.float32, np.float64
SAMPLE_TAG = 0x53414D50
GOLDEN = 0x9E3779B97F4A7C15
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ host model
def philox4x32_10(ctr, key):
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def host_u(seed, call, row, cur_len):
    """(m, u exact as float64, u as the kernel's fp32 diagnostic) of (row, position) — header step 5"""
    k = (int(seed) + GOLDEN * int(call)) & (2 ** 64 - 1)
    m = philox4x32_10((row & M32, cur_len & M32, SAMPLE_TAG, 0), (k & M32, k >> 32))[0] >> 8
    u = (m + 0.5) * 2.0 ** -24                            # exact in float64
    return m, u, F32(u)


def host_banned(history, n):
    """NoRepeatNGram: tokens that followed an earlier occurrence of the last n - 1 tokens"""
    h = [int(t) for t in history]
    if n <= 0 or len(h) + 1 < n:
        return []
    prefix = h[len(h) - (n - 1):] if n > 1 else []
    return [h[i + n - 1] for i in range(len(h) - n + 1) if h[i:i + n - 1] == prefix]


def host_processors(z, history=None, ngram=0, eos=2, suppress_eos=False, forced=-1):
    """step 1 on one row of raw fp32 logits (already cut to V columns)"""
    z = np.array(z, dtype=F32)
    if forced >= 0:
        out = np.full_like(z, -np.inf)
        out[forced] = 0.0
        return out
    if history is not None:
        for t in host_banned(history, ngram):
            if 0 <= t < len(z):
                z[t] = -np.inf
    if suppress_eos and 0 <= eos < len(z):
        z[eos] = -np.inf
    return z


def host_warp(z, T=1.0, top_k=0, top_p=1.0):
    """steps 2-4 on one processed row.  Returns dict(zp fp32, thr, kept bool mask of finite kept tokens, p float64 probabilities
    over the kept set, larger float64 = probability (within the top-k survivors) of the strictly larger tokens, mass = kept share)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        zp = (np.asarray(z, F32) / F32(T)).astype(F32)
    zp[np.isnan(zp)] = -np.inf
    zp = np.minimum(zp, np.finfo(F32).max).astype(F32) + F32(0.0)
    V = len(zp)
    alive = np.ones(V, bool)
    thr = F32(-np.inf)
    if 1 <= top_k < V:
        thr = np.sort(zp)[V - top_k]
        alive = zp >= thr
    finite = np.isfinite(zp)
    if not finite.any():
        return dict(zp=zp, thr=thr, kept=np.zeros(V, bool), p=np.zeros(V), larger=np.zeros(V), mass=0.0)
    zmax = zp[finite].max().astype(F64)
    w = np.where(alive & finite, np.exp(np.where(finite, zp.astype(F64) - zmax, 0.0)), 0.0)
    w = w / w.sum()
    vals, inv = np.unique(zp, return_inverse=True)                    # ascending
    per_val = np.bincount(inv, weights=w, minlength=len(vals))
    above = np.concatenate([np.cumsum(per_val[::-1])[::-1][1:], [0.0]])      # mass of strictly larger values
    larger = above[inv]
    keep = alive.copy()
    if 0.0 < top_p < 1.0:
        keep = alive & (larger <= top_p)
        thr = zp[keep].min()
    kept = keep & finite
    p = np.where(kept, w, 0.0)
    mass = p.sum()
    return dict(zp=zp, thr=F32(thr), kept=kept, p=p / mass, larger=larger, mass=mass)


def host_choose(p, u):
    """step 5: first token in ascending id whose inclusive cumulative probability exceeds u; also its CDF interval [lo, hi)"""
    c = np.cumsum(p)
    c[-1] = max(c[-1], 1.0)
    tok = int(np.searchsorted(c, u, side="right"))
    tok = min(tok, len(p) - 1)
    while p[tok] == 0.0:                                   # (u beyond the last kept token through rounding of the total)
        tok -= 1
    return tok, (c[tok] - p[tok], c[tok])


def wilson_hilferty(dof):
    """the 1 - 1e-6 quantile of chi-square(dof), Wilson-Hilferty's cube approximation"""
    zq = 4.753424308822899                                 # standard normal 1 - 1e-6 quantile
    return dof * (1.0 - 2.0 / (9.0 * dof) + zq * math.sqrt(2.0 / (9.0 * dof))) ** 3


def chi2_quantile(dof):
    """the 1 - 1e-6 quantile of chi-square(dof): scipy, else Wilson-Hilferty"""
    try:
        from scipy.stats import chi2
        return float(chi2.isf(1e-6, dof))
    except ImportError:
        return wilson_hilferty(dof)


# ------------------------------------------------------------------------------------------------ the host model on hand-made rows
def test_philox_known_answer():
    # Random123 known-answer vectors of Philox4x32-10
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox4x32_10((M32, M32, M32, M32), (M32, M32)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    m, u, u32 = host_u(7, 3, 5, 9)
    assert 0 <= m < 2 ** 24 and 0.0 < u < 1.0 and u == (2 * m + 1) / 2.0 ** 25
    assert host_u(7, 3, 5, 9) == (m, u, u32) and host_u(7, 4, 5, 9)[0] != m and host_u(8, 3, 5, 9)[0] != m


def test_host_model_hand_rows():
    z = np.array([1.0, 3.0, 3.0, -np.inf, 2.0, 0.0, 2.0], F32)
    # k = 1: the top value and its tie
    w = host_warp(z, top_k=1)
    assert w["thr"] == 3.0 and w["kept"].tolist() == [False, True, True, False, False, False, False]
    assert np.allclose(w["p"][[1, 2]], 0.5)
    # k = 3 lands inside the tie group at 2.0: the whole group stays (3, 3, 2, 2)
    w = host_warp(z, top_k=3)
    assert w["thr"] == 2.0 and int(w["kept"].sum()) == 4
    # k = 6 of 7: the 6-th largest is 0.0; k = V and beyond: off; -inf is never "kept"
    assert host_warp(z, top_k=6)["thr"] == 0.0 and int(host_warp(z, top_k=6)["kept"].sum()) == 6
    for k in (0, 7, 12):
        w = host_warp(z, top_k=k)
        assert w["thr"] == -np.inf and int(w["kept"].sum()) == 6
    # banned up to all but one: the k-th largest is -inf, nothing is cut, one finite token is kept with probability 1
    zb = np.full(7, -np.inf, F32); zb[4] = -2.5
    w = host_warp(zb, top_k=2)
    assert w["thr"] == -np.inf and w["kept"].tolist() == [i == 4 for i in range(7)] and w["p"][4] == 1.0
    # top-p -> 0 keeps the top tie group only; the top token always stays
    w = host_warp(z, top_p=1e-6)
    assert w["thr"] == 3.0 and int(w["kept"].sum()) == 2
    # top-p on a tie-free row: p = softmax([2, 1, 0]) = [.665, .245, .090]; before-mass = [0, .665, .910]
    zt = np.array([0.0, 2.0, 1.0], F32)
    assert host_warp(zt, top_p=0.5)["kept"].tolist() == [False, True, False]
    assert host_warp(zt, top_p=0.7)["kept"].tolist() == [False, True, True]
    assert host_warp(zt, top_p=0.95)["kept"].tolist() == [True, True, True]
    assert abs(host_warp(zt, top_p=0.7)["mass"] - (1 - 0.09003057)) < 1e-6
    # temperature is an fp32 division before everything else; top-p after top-k renormalises over the survivors
    w = host_warp(zt, T=0.5, top_k=2, top_p=0.85)
    assert np.array_equal(w["zp"], np.array([0.0, 4.0, 2.0], F32)) and w["kept"].tolist() == [False, True, False]      # .881 | .119
    w = host_warp(zt, T=2.0, top_k=2, top_p=0.85)
    assert w["kept"].tolist() == [False, True, True]                                                                  # .622 | .378
    # the draw walks ascending token ids
    p = np.array([0.0, 0.25, 0.0, 0.5, 0.25])
    assert [host_choose(p, u)[0] for u in (1e-9, 0.2499, 0.25, 0.5, 0.7499, 0.75, 1 - 1e-9)] == [1, 1, 3, 3, 3, 4, 4]
    assert host_choose(p, 0.3)[1] == (0.25, 0.75)
    # processors
    assert host_banned([5, 6, 7, 5, 6], 3) == [7] and host_banned([5, 6], 3) == [] and host_banned([4, 9, 4], 1) == [4, 9, 4]
    zz = host_processors(np.zeros(8, F32), history=[2, 5, 6, 5], ngram=2, eos=2, suppress_eos=True)
    assert np.isinf(zz[[2, 6]]).all() and np.isfinite(np.delete(zz, [2, 6])).all()
    zz = host_processors(np.ones(8, F32), forced=3)
    assert zz[3] == 0.0 and np.isinf(np.delete(zz, 3)).all()
    # chi-square(1) has its 1 - 1e-6 quantile at z^2 = 23.93; this far out the cube approximation errs high: 15 % at 1 degree of
    # freedom, 6 % at 4, 0.3 % at 63
    assert 23.9 < chi2_quantile(1) < 27.6
    assert all(0.0 <= wilson_hilferty(d) / chi2_quantile(d) - 1.0 < 0.06 for d in (4, 10, 63, 1000))


def test_host_model_against_transformers_warpers():
    """guards the test's own model: HF's warpers on tie-free rows keep the same sets (the host model stays the authority)"""
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(5)
    for V, T, k, p in ((50, 1.0, 0, 0.9), (50, 0.5, 7, 1.0), (200, 2.0, 20, 0.5), (200, 1.0, 0, 0.3), (64, 1.5, 1, 0.8)):
        z = rng.normal(0, 2, size=V).astype(F32)
        assert len(np.unique(z)) == V
        s = torch.from_numpy(z)[None]
        ids = torch.zeros((1, 1), dtype=torch.long)
        if T != 1.0:
            s = lp.TemperatureLogitsWarper(float(T))(ids, s)
        if k > 0:
            s = lp.TopKLogitsWarper(k)(ids, s)
        if p < 1.0:
            s = lp.TopPLogitsWarper(p)(ids, s)
        w = host_warp(z, T, k, p)
        hf_kept = torch.isfinite(s[0]).numpy()
        # a token whose before-mass is within float32 rounding of top_p may fall either way in HF's fp32 cumsum: none here
        if p < 1.0:
            alive = np.isfinite(w["zp"]) & (w["zp"] >= (np.sort(w["zp"])[V - k] if k else -np.inf))
            assert np.abs(w["larger"][alive] - p).min() > 1e-5
        assert np.array_equal(hf_kept, w["kept"]), (V, T, k, p)
        assert np.allclose(torch.softmax(s[0].double(), -1).numpy(), w["p"], atol=1e-6)


# ------------------------------------------------------------------------------------------------ generate(): refusals, unchanged default
class _NoModel:
    """stands in for a model that was never finalized: generate() reaches `model.arena is None` only after its argument checks"""
    config = None
    arena = None


def test_generate_sampling_refusals():
    from vacnic_amd.generate import generate
    ok = dict(do_sample=True, num_beams=1)
    with pytest.raises(ValueError, match="num_beams"):
        generate(_NoModel(), do_sample=True, num_beams=2)
    with pytest.raises(ValueError, match="encoded"):
        generate(_NoModel(), encoded=object(), **ok)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError, match="temperature"):
            generate(_NoModel(), temperature=bad, **ok)
    for bad in (0, 0.0, -0.5, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="top_p"):
            generate(_NoModel(), top_p=bad, **ok)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="top_k"):
            generate(_NoModel(), top_k=bad, **ok)
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError, match="num_return_sequences"):
            generate(_NoModel(), num_return_sequences=bad, **ok)
    # valid sampling arguments pass the checks and reach the model
    with pytest.raises(RuntimeError, match="finalize"):
        generate(_NoModel(), temperature=0.7, top_k=5, top_p=0.9, num_return_sequences=3, seed=1, **ok)


def test_do_sample_false_ignores_the_new_keywords():
    """do_sample=False: the sampling keywords are ignored as **unused ignored them, whatever they hold — the call goes on to the
    beam / greedy code (here: to its first statement about the model)"""
    from vacnic_amd.generate import generate
    with pytest.raises(RuntimeError, match="finalize"):
        generate(_NoModel(), do_sample=False, num_beams=5, temperature=-1.0, top_k=-4, top_p=7.0, num_return_sequences=0, seed="x",
                 return_logprobs=True, encoded=object())


def test_sample_step_bad_arguments_return_status(built_lib):
    from vacnic_amd import _lib
    assert "vacnic_sample_step" in _lib.EXPORTED
    good = dict(logits=16, params=16, seq=16, done=16, next_ids=16, logp=16, kept=None, thr=None, mass=None, u=None, R=2, V=100, ldl=104,
                Lmax=8, cur_len=1, eos=2, pad=1, no_repeat_ngram_size=0, suppress_eos=0, forced_token=-1)

    def call(**kw):
        _lib.call_struct("vacnic_sample_step", stream=None, **dict(good, **kw))
    for name in ("logits", "params", "seq", "done", "next_ids"):
        with pytest.raises(ValueError, match="null operand"):
            call(**{name: None})
    for V in (0, -1, 65537):
        with pytest.raises(_lib.VacnicError, match="65536"):
            call(V=V, ldl=70000)
    with pytest.raises(ValueError, match="ldl"):
        call(ldl=99)
    with pytest.raises(ValueError, match="R >= 1"):
        call(R=0)
    for cur in (0, 8, -2):
        with pytest.raises(ValueError, match="cur_len"):
            call(cur_len=cur)
    with pytest.raises(ValueError, match="forced token"):
        call(forced_token=100)
    with pytest.raises(ValueError, match="n-gram"):
        call(no_repeat_ngram_size=-1)


def test_sample_params_layout():
    import struct
    from vacnic_amd import kernels as K
    w = K.sample_params(0.75, 40, 0.9, seed=(5 << 32) | 7, call=(1 << 32) | 3)
    assert w.dtype == torch.int32 and w.shape == (8,)
    raw = w.numpy().tobytes()
    assert struct.unpack("<fifiIIII", raw) == (0.75, 40, struct.unpack("<f", struct.pack("<f", 0.9))[0], 0, 7, 5, 3, 1)
