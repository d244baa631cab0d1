"""GPU: the repetition penalty and the bad-word bans on every decode path, against the host models of
tests/test_decode_processors.py (and, for sampling, the host model of tests/test_sample.py extended with them).

  * vacnic_sample_step: replayed on the host.  Processors, the penalty (one fp32 operation), the temperature division, the top-k
    threshold and the kept count involve no rounding -> equality (the threshold is the penalised value bit for bit whenever a
    history token sits at the k-th rank, which the rows arrange).  The draw and the log-prob carry the bounds of
    tests/test_sample_gpu.py: the chosen token's float64 CDF interval widened by V * 2^-24 contains u, and the token IS the float64
    choice unless u lies within that band of an interval end; |logp - log q| <= 1e-5.
  * vacnic_beam_init / vacnic_beam_step: lockstep with the host beam search of tests/test_decode_gpu.py, state bit-equal, ban
    lists compared as sets per row.
  * vacnic_beam_topk_ex (both kernels, fp32 and bf16 logits, both penalty rules) and vacnic_lmhead_topk: picks equal to a float64
    reference, scores within margin_of (tests/test_decode_gpu.py: 8x the deviation of fp32 torch from float64, no new constant), on
    rows whose picks are decidable (decidable_order asserts it on the reference alone); the fused tail also against the unfused
    chain on the logits it writes out.
  * generate(): device and host bookkeeping, eager and replayed, give the same ids as HF's loop driven on the host over the model's
    own per-position logits with the host models; no bad word occurs in them; alternating penalties never see a stale graph."""
import types

import numpy as np
import pytest
import torch

from test_decode_processors import F32, host_bad_words, host_repetition_penalty
from test_sample import host_choose, host_processors, host_u, host_warp

gpu = pytest.mark.gpu
EOS, PAD = 2, 1


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


# ------------------------------------------------------------------------------------------------ vacnic_sample_step
LMAX, CUR = 12, 6
HIST = np.array([[EOS, 5, 9, 5, 9, 5],            # start == eos, repeats; "9 5" occurred before: n-gram size 2 bans 9
                 [EOS, 7, 8, 30, 7, 3],
                 [EOS, 4, 4, 4, 4, 4]])
WORDS = [(11,), (5, 12), (9, 5, 13), (EOS, 7, 8, 30, 7, 3, 14), (EOS, 4, 4, 4, 4, 4, 15), (4, 4, 4, 4, 4, 4, 4, 18), (8, 16), (3, 17), (EOS,),
         (5, 12)]           # 14 / 15: the prefix is the whole history; 18: longer than history + 1; 16: no match; [eos]: dropped
_LOGITS = {}


def sample_rows(V):
    """fp32 [3, ldl]: normal(0, 2) with the history tokens and the bad words' last tokens planted at the top ranks (positive and
    negative values, a zero), so that the top-k thresholds of small k fall on penalised values; 1e30 in the padding columns."""
    if V not in _LOGITS:
        rng = np.random.default_rng([17, V])
        z = np.full((3, (V + 8) // 8 * 8 + 8), 1e30, F32)
        z[:, :V] = rng.normal(0, 2, size=(3, V)).astype(F32)
        for r in range(3):
            top = sorted(set(HIST[r].tolist())) + [11, 12, 13, 14, 15, 17]
            z[r, top] = (9.0 + rng.permutation(len(top)) * 0.37).astype(F32)
        z[0, 9] = -3.25                                                      # a negative history logit: multiplied, not divided
        z[1, 30] = 0.0
        z[2, 4] = np.float32(9.7)
        _LOGITS[V] = z
    return _LOGITS[V]


def run_sample(K, z, V, hist, *, penalty=1.0, words=None, T=1.0, top_k=0, top_p=1.0, seed=11, ngram=0, suppress_eos=False, forced=-1,
               done=None, LMAX=LMAX):
    R, cur = hist.shape
    dev = "cuda"
    params = K.sample_params(T, top_k, top_p, seed, 0, repetition_penalty=penalty).to(dev)
    seq = torch.full((R, LMAX), PAD, dtype=torch.int32)
    seq[:, :cur] = torch.from_numpy(hist).to(torch.int32)
    seq = seq.to(dev)
    done_t = (torch.zeros(R, dtype=torch.int32) if done is None else torch.as_tensor(done, dtype=torch.int32)).to(dev)
    next_ids = torch.full((R,), -7, dtype=torch.int64, device=dev)
    logp = torch.full((R, LMAX), 9.0, device=dev)
    kept = torch.full((R,), -7, dtype=torch.int32, device=dev)
    thr, mass, u = (torch.full((R,), 9.0, device=dev) for _ in range(3))
    table = K.bad_words_table([w for w in words if w != (EOS,)]) if words else None
    K.sample_step(torch.from_numpy(z).to(dev), V, params, seq, done_t, next_ids, cur, logp=logp, eos=EOS, pad=PAD, no_repeat_ngram_size=ngram,
                  suppress_eos=suppress_eos, forced_token=forced, kept=kept, thr=thr, mass=mass, u=u, bad_words=table)
    torch.cuda.synchronize()
    o = types.SimpleNamespace(token=next_ids.cpu().numpy(), seq=seq.cpu().numpy(), done=done_t.cpu().numpy(), logp=logp.cpu().numpy(),
                              kept=kept.cpu().numpy(), thr=thr.cpu().numpy(), mass=mass.cpu().numpy(), u=u.cpu().numpy())
    assert np.array_equal(o.seq[:, :cur], hist) and np.array_equal(o.seq[:, cur], o.token)
    assert np.array_equal(o.seq[:, cur + 1:], np.full((R, LMAX - cur - 1), PAD))
    return o


def check_sample(o, z, V, hist, *, penalty=1.0, words=None, T=1.0, top_k=0, top_p=1.0, seed=11, ngram=0, suppress_eos=False, forced=-1,
                 done=None, tag=""):
    R, cur = hist.shape
    eps = V * 2.0 ** -24
    for r in range(R):
        what = (tag, V, r)
        if done is not None and done[r]:
            assert o.token[r] == PAD and o.logp[r, cur] == 0 and o.done[r] == 1, what
            continue
        if forced >= 0:
            assert o.token[r] == forced and o.logp[r, cur] == 0 and o.done[r] == int(forced == EOS) and o.kept[r] == 1, what
            continue
        zr = host_repetition_penalty(z[r, :V], hist[r], penalty, "logits")
        zr = host_processors(zr, history=hist[r], ngram=ngram, eos=EOS, suppress_eos=suppress_eos)
        for t in (host_bad_words(hist[r], words, EOS) if words else []):
            zr[t] = -np.inf
        w = host_warp(zr, T, top_k, top_p)
        zp = w["zp"]
        if not np.isfinite(zp).any():
            assert o.token[r] == EOS and o.done[r] == 1 and o.kept[r] == 0 and o.logp[r, cur] == 0, what
            continue
        m, u, u32 = host_u(seed, 0, r, cur)
        assert o.u[r].tobytes() == u32.tobytes(), what
        if top_p >= 1.0:                                                        # nothing rounded up to here: bit-equal
            assert o.thr[r].tobytes() == F32(w["thr"]).tobytes() and int(o.kept[r]) == int(w["kept"].sum()), (what, o.thr[r], w["thr"])
        got = (zp >= o.thr[r]) & np.isfinite(zp)
        assert int(o.kept[r]) == int(got.sum()), what
        q = np.where(got, np.exp(zp.astype(np.float64) - zp[got].max()), 0.0)
        q /= q.sum()
        tok, (lo, hi) = host_choose(q, u)
        c = np.cumsum(q)
        t = int(o.token[r])
        assert got[t] and c[t] - q[t] - eps <= u <= c[t] + eps, (what, t, tok, u)
        if lo + eps < u < hi - eps:
            assert t == tok, (what, t, tok, u)
        assert abs(float(o.logp[r, cur]) - np.log(q[t])) <= 1e-5, (what, float(o.logp[r, cur]), np.log(q[t]))
        assert o.done[r] == int(t == EOS), what


SETTINGS = [dict(), dict(top_k=1), dict(top_k=3), dict(top_k=7), dict(top_p=0.8), dict(T=0.7), dict(ngram=2), dict(suppress_eos=True),
            dict(words=WORDS), dict(T=1.6, top_k=9, top_p=0.9, ngram=2, suppress_eos=True, words=WORDS)]


@gpu
@pytest.mark.parametrize("V", [37, 1025, 50265])
def test_sample_step_replays_with_penalty_and_bad_words(K, V):
    z = sample_rows(V)
    for penalty in (1.3, 0.7, 1.0):
        for i, kw in enumerate(SETTINGS):
            for seed in (11, 12):
                o = run_sample(K, z, V, HIST, penalty=penalty, seed=seed, **kw)
                check_sample(o, z, V, HIST, penalty=penalty, seed=seed, tag=(penalty, i), **kw)
    # the processors do what they are there for: the top-1 "sample" is the arg-max of the processed row
    for penalty, words in ((1.0, None), (1.3, None), (1.0, WORDS), (0.7, WORDS)):
        o = run_sample(K, z, V, HIST, penalty=penalty, words=words, top_k=1)
        for r in range(3):
            zr = host_repetition_penalty(z[r, :V], HIST[r], penalty, "logits")
            for t in (host_bad_words(HIST[r], words, EOS) if words else []):
                zr[t] = -np.inf
            assert o.token[r] == int(np.argmax(zr)) and o.thr[r] == zr.max(), (V, penalty, r)
    banned = [host_bad_words(HIST[r], WORDS, EOS) for r in range(3)]
    assert banned == [[11, 12, 13], [11, 14, 17], [11, 15]]                     # (a prefix as long as the whole history matched: 14)
    # a forced position and a done row: neither processor matters
    o = run_sample(K, z, V, HIST, penalty=1.3, words=WORDS, forced=3)
    check_sample(o, z, V, HIST, penalty=1.3, words=WORDS, forced=3)
    o = run_sample(K, z, V, HIST, penalty=1.3, words=WORDS, done=[0, 1, 0])
    check_sample(o, z, V, HIST, penalty=1.3, words=WORDS, done=[0, 1, 0])


@gpu
def test_sample_step_all_banned_and_full_table(K):
    V = 37
    # every finite token of row 1 is a bad word: the row emits eos and finishes; the other rows draw among what is left
    z = np.full((3, 48), 1e30, F32)
    z[:, :V] = -np.inf
    z[:, [20, 21, 22]] = np.array([1.0, 0.5, -0.5], F32)
    z[1, 22] = -np.inf
    hist = HIST.copy()
    words = [(20,), (7, 3, 21), (EOS, 4, 4, 4, 4, 4, 22)]                      # row 1: 20 and 21; row 2: 20 and 22; row 0: 20
    o = run_sample(K, z, V, hist, penalty=1.3, words=words)
    check_sample(o, z, V, hist, penalty=1.3, words=words)
    assert o.token.tolist()[1] == EOS and o.done.tolist() == [0, 1, 0] and o.kept.tolist() == [2, 0, 1] and o.token[2] == 21
    # the table at its capacity: BAD_WORDS_MAX words of BAD_WORD_LEN tokens; the matching ones sit at both ends and in the middle
    V = 1025
    z = sample_rows(V).copy()
    rng = np.random.default_rng(23)
    full = [tuple(rng.integers(40, V, size=K.BAD_WORD_LEN).tolist()) for _ in range(K.BAD_WORDS_MAX)]
    Lh = K.BAD_WORD_LEN - 1                                                      # the longest word's prefix is the whole history
    long_hist = np.concatenate([np.tile(np.array([[EOS]]), (3, 1)), rng.integers(40, V, size=(3, Lh - 1))], axis=1)
    full[0] = tuple(long_hist[0, -3:].tolist()) + (5,)
    full[511] = tuple(long_hist[1].tolist()) + (7,)                            # BAD_WORD_LEN tokens: the whole history of row 1
    full[512] = tuple(long_hist[2, 1:].tolist()) + (6,)
    full[K.BAD_WORDS_MAX - 1] = (9,)
    full[K.BAD_WORDS_MAX - 2] = tuple(long_hist[2, -1:].tolist()) + (4,)
    assert len(full[511]) == K.BAD_WORD_LEN and len(full) == K.BAD_WORDS_MAX
    assert [host_bad_words(long_hist[r], full, EOS) for r in range(3)] == [[5, 9], [7, 9], [4, 6, 9]]
    for r, toks in enumerate(([5, 9], [7, 9], [4, 6, 9])):
        z[r, toks] = 20.0 + np.arange(len(toks), dtype=F32)                      # unbanned, one of them is the arg-max
    free = run_sample(K, z, V, long_hist, top_k=1, LMAX=Lh + 3)
    assert free.token.tolist() == [9, 9, 9]
    o = run_sample(K, z, V, long_hist, words=full, top_k=1, LMAX=Lh + 3)
    check_sample(o, z, V, long_hist, words=full, top_k=1)
    assert not np.isin(o.token, [4, 5, 6, 7, 9]).any()
    with pytest.raises(ValueError, match="bad_words_table"):
        K.bad_words_table(full + [(3,)])


# ------------------------------------------------------------------------------------------------ vacnic_beam_init / vacnic_beam_step
def beam_lockstep(K, c, words, max_pos=None):
    """device state against the host beam search position by position; returns the host reference, how often a word of more than
    one token matched (per position: rows whose ban list holds such a word's last token), and how many rows of FINISHED items had
    their (empty) ban lists compared"""
    import test_decode_gpu as D
    from oracle import vacnic_oracle as O
    B, nb, L = c["B"], c["nb"], c["Lmax"]
    R, K2 = B * nb, min(2 * nb, D.VS)

    class Host(D.HostBeams):
        def processed(self, lp):
            lp = super().processed(lp)
            for r, s in enumerate(self.seqs):
                for tok in host_bad_words(s, words, D.EOS):
                    lp[r, tok] = D.NEG
            return lp
    table = K.bad_words_table(words) if words else None
    st = K.beam_alloc(B, nb, L, D.VS, D.EOS, D.PAD, no_repeat_ngram_size=c["ngram"], early_stopping=c["early"], length_penalty=c["lp"],
                      bad_words=table)
    n_bad = len(words)
    assert (st.bans is None) == (c["ngram"] == 0 and n_bad == 0) and (st.bans is None or st.bans.shape == (R, L + n_bad))
    if st.bans is not None:
        st.bans.fill_(77)                                                       # beam_init owns the lists
    K.beam_init(st, c["start"])
    host = Host(O, c)
    torch.cuda.synchronize()

    def check_bans(was_done):
        if st.bans is None:
            return np.zeros(2, dtype=np.int64)
        bans = st.bans.cpu().numpy()
        multi = finished = 0
        for r, s in enumerate(host.seqs):
            live = not was_done[r // nb]
            grams = O.banned_ngram_tokens(s, c["ngram"]) if live else []
            bad = host_bad_words(s, words, D.EOS) if live else []              # a finished item bans nothing
            got = bans[r][bans[r] >= 0].tolist()
            # (two words that ban the same token both write it: the lists are sets with repetition)
            assert set(got) == set(grams) | set(bad) and len(got) <= len(grams) + len(words), (host.cur_len, r, s, got, grams, bad)
            n = len(got)
            assert bool((bans[r, :n] >= 0).all()) and bool((bans[r, n:] == -1).all()), (host.cur_len, r, bans[r].tolist())
            multi += len(set(bad) - {w[0] for w in words if len(w) == 1}) > 0
            finished += not live
        return np.array([multi, finished])
    fired = check_bans([False] * B)                                             # the first position's bans come from beam_init
    shim = types.SimpleNamespace(**{k: v for k, v in vars(st).items() if k != "bans"}, bans=None)
    for cur in range(1, max_pos or L):
        lp = D.table_rows(c, host.seqs, cur)
        tv, ti = D.row_lists(lp, None if st.bans is None else st.bans.cpu(), st.beam_scores.cpu().numpy(), cur < c["min_length"], K2)
        prev = host.seqs
        K.beam_step(st, tv.cuda(), ti.cuda(), cur)
        was_done = host.step(lp)
        D.compare_state(O, shim, host, was_done, prev, c, cur)
        fired += check_bans(was_done)
        if all(host.done):
            break
    return host, int(fired[0]), int(fired[1])


@gpu
@pytest.mark.parametrize("ci", [0, 1, 3, 9])
def test_beam_step_lockstep_with_bad_words(K, ci):
    import test_decode_gpu as D
    from oracle import vacnic_oracle as O
    c = D.STEP_CASES[ci]
    free = D.run_host(O, c)
    best = free.finalize()[0][0][1]                                             # the unrestricted best hypothesis of item 0
    assert len(best) >= 3 and best[0] == c["start"]
    # bad words taken from what the unrestricted search emits: the first position (matched by beam_init: the prefix is the whole
    # history [start]), a later bigram and trigram (matched after beams were reordered), a token alone; [eos] is dropped by the
    # caller, a word that never matches and a duplicate ride along
    words = [(best[0], best[1]), (best[2],), (D.VS - 1, D.VS - 2, D.VS - 3)]
    mid, _, _ = beam_lockstep(K, c, words)
    other = mid.finalize()[0][0][1]
    assert other != best and other[1] != best[1] and best[2] not in other[1:]
    words += [tuple(other[1:3]), tuple(other[1:4]), tuple(other[1:3])]         # a later bigram, a trigram, a duplicate
    host, fired, finished = beam_lockstep(K, c, words)
    assert fired > 0                                                            # a word of several tokens matched on some row
    if c["B"] > 1 and "staggered" in c["expect"]:
        # an item finished before the others under the restricted search too: its rows' ban lists were compared (they hold nothing)
        assert finished > 0, (ci, finished)
    for b, nbest in enumerate(host.finalize()):
        for _, seq in nbest:
            for w in words:
                assert not any(tuple(seq[i:i + len(w)]) == w for i in range(len(seq) - len(w) + 1)), (b, seq, w)


# ------------------------------------------------------------------------------------------------ generate()
_MODEL = []


def generation_inputs(K):
    """the tiny generation model of tests/test_decode_gpu.py and one caption's inputs, built once"""
    if not _MODEL:
        import test_decode_gpu as D
        from vacnic_amd import synthetic
        cfg, sd, model = D.tiny_generation_model()
        batch = synthetic.make_batch(cfg, 1, S=24, T=8, F=2, seed=9, image_size=32)
        img = synthetic._normal("img_cls", (1, 768), 1.0, 3)
        dev = {k: v.cuda() for k, v in batch.items()}
        mask, _ = K.prep_ids(dev["article_ids"], 1)
        nmask, _ = K.prep_ids(dev["names_art_ids"], 1)
        kw = dict(input_ids=dev["article_ids"], attention_mask=mask, max_length=9, min_length=6, length_penalty=1.0, image_features=img.cuda(),
                  face_features=dev["face_emb"], face_mask=K.face_mask(dev["face_emb"]), name_ids=dev["names_art_ids"], name_mask=nmask,
                  add_ner_ffn=True)
        _MODEL.append((model, kw))
    return _MODEL[0]


def contains(seq, w):
    return any(tuple(seq[i:i + len(w)]) == tuple(w) for i in range(len(seq) - len(w) + 1))


@gpu
@pytest.mark.parametrize("nb", [1, 3])
def test_generate_bad_words_every_path(K, nb):
    model, kw = generation_inputs(K)
    model.__dict__.pop("_decode_sessions", None)
    free = model.generate(num_beams=nb, no_repeat_ngram_size=2, **kw)
    assert len(model._decode_sessions) == 1 and all(len(k) == 9 for k in model._decode_sessions)       # the key of before
    f = free[0].tolist()
    assert len(f) >= 6
    words = [[f[3]], [f[1], f[2]], [2], [f[3]]]                                 # tokens the unrestricted decode DOES emit
    gkw = dict(num_beams=nb, no_repeat_ngram_size=2, bad_words_ids=words, **kw)
    eager = model.generate(use_graphs=False, **gkw)
    outs = [model.generate(**gkw) for _ in range(3)]                            # eager, capture, replay
    host = [model.generate(device_beams=False, **gkw) for _ in range(3)]
    host_eager = model.generate(device_beams=False, use_graphs=False, **gkw)
    for o in outs + host + [host_eager]:
        assert torch.equal(o, eager), (nb, o.tolist(), eager.tolist())
    e = eager[0].tolist()
    assert e != f and not contains(e[1:], [f[3]]) and not contains(e, [f[1], f[2]]), (f, e)
    assert torch.equal(model.generate(num_beams=nb, no_repeat_ngram_size=2, **kw), free)               # the table did not leak into the old session


def run_host_driven(K, model, kw, nb, penalty, words, ngram):
    """HF beam_search / greedy_search on the host (oracle.beam_search_bookkeeping) over the model's own per-position fp32 logits: every
    row is decoded along its own history by a cached decoder of its own (no reorder), the two processors are the host models."""
    from oracle import vacnic_oracle as O
    from vacnic_amd import generate as G
    cfg = model.config
    mask_u8 = kw["attention_mask"].to(torch.uint8)
    enc_h = G._run_encoder(model, False, kw["add_ner_ffn"], kw["input_ids"], mask_u8, kw["image_features"], kw["name_ids"], kw["name_mask"],
                           kw["face_features"], kw["face_mask"])
    dec = G.CachedDecoder(model, nb, enc_h.shape[1], kw["max_length"], reorders=False)
    dec.begin(enc_h, mask_u8, nb)
    V = model.V

    def fn(seqs):
        for t in range(len(seqs[0])):
            ids = torch.tensor([[s[t]] for s in seqs], device="cuda")
            logits = dec.step(ids, t)
        z = logits[:, :V].float().cpu().numpy()
        out = np.empty((len(seqs), V))
        for r, s in enumerate(seqs):
            if nb == 1:                                                         # greedy_search: the processors see the raw logits
                zp = host_repetition_penalty(z[r], s, penalty, "logits").astype(np.float64)
                out[r] = zp - (zp.max() + np.log(np.exp(zp - zp.max()).sum()))
            else:                                                               # beam_search: they see log_softmax(logits)
                out[r] = host_repetition_penalty(z[r], s, penalty, "scores")
            for tok in host_bad_words(s, words, cfg.eos_token_id):
                out[r, tok] = -np.inf
        return torch.from_numpy(out)
    return O.beam_search_bookkeeping(fn, 1, nb, kw["max_length"], cfg.eos_token_id, cfg.pad_token_id, cfg.decoder_start_token_id,
                                     length_penalty=kw["length_penalty"], no_repeat_ngram_size=ngram, min_length=kw["min_length"],
                                     forced_eos_token_id=cfg.eos_token_id)


@gpu
@pytest.mark.parametrize("nb", [1, 3])
def test_generate_penalty_and_bad_words_every_path(K, nb):
    """the test that fails without the feature: the keywords used to vanish into **unused and the unrestricted ids came back"""
    model, kw = generation_inputs(K)
    model.__dict__.pop("_decode_sessions", None)
    free = model.generate(num_beams=nb, no_repeat_ngram_size=2, **kw)
    f = free[0].tolist()
    words = [[f[3]], [f[1], f[2]]]                                               # tokens the unrestricted decode DOES emit
    gkw = dict(num_beams=nb, no_repeat_ngram_size=2, repetition_penalty=1.4, bad_words_ids=words, **kw)
    eager = model.generate(use_graphs=False, **gkw)
    outs = [model.generate(**gkw) for _ in range(3)]                            # eager, capture, replay
    host = [model.generate(device_beams=False, **gkw) for _ in range(3)]
    host_eager = model.generate(device_beams=False, use_graphs=False, **gkw)
    for o in outs + host + [host_eager]:
        assert torch.equal(o, eager), (nb, o.tolist(), eager.tolist())
    e = eager[0].tolist()
    assert e != f and not contains(e[1:], [f[3]]) and not contains(e, [f[1], f[2]]), (f, e)
    want = run_host_driven(K, model, kw, nb, 1.4, words, 2)
    assert torch.equal(eager.cpu(), want), (nb, e, want.tolist())
    # the penalty alone, above and below 1, matches the host; and it matters: some pair of penalties gives two different captions.
    # (The synthetic model is sharp: where one token has all the probability its score is exactly 0 and no penalty on the scores
    # moves it, so which values differ is found among a few instead of assumed.)
    cands = (0.6, 1.4, 0.05, 2.5, 6.0, 20.0)
    okw = dict(num_beams=nb, no_repeat_ngram_size=2, **kw)
    ref = {p: model.generate(use_graphs=False, repetition_penalty=p, **okw) for p in cands}
    for p in (0.6, 1.4):
        assert torch.equal(ref[p].cpu(), run_host_driven(K, model, kw, nb, p, [], 2)), (nb, p)
    other = next(p for p in cands[1:] if not torch.equal(ref[p], ref[0.6]))
    assert torch.equal(ref[other].cpu(), run_host_driven(K, model, kw, nb, other, [], 2)), (nb, other)
    # two penalties alternating on one shape, graphs on: each gets its eager result (the value is part of the session key)
    for rnd in range(3):
        for p in (other, 0.6):
            got = model.generate(repetition_penalty=p, **okw)
            assert torch.equal(got, ref[p]), (nb, rnd, p, got.tolist(), ref[p].tolist())
    assert torch.equal(model.generate(num_beams=nb, no_repeat_ngram_size=2, **kw), free)


@gpu
def test_processor_sessions_are_capped(K):
    """the penalty is a free axis of the DecodeSession key: a model keeps the most recently used _PROCESSOR_SESSIONS_MAX sessions with
    processors; the session of the default key is not among those that go"""
    from vacnic_amd import generate as G
    model, kw = generation_inputs(K)
    model.__dict__.pop("_decode_sessions", None)
    free = model.generate(num_beams=1, **kw)
    n = G._PROCESSOR_SESSIONS_MAX
    pens = [1.1 + 0.1 * i for i in range(n + 2)]
    for p in pens:
        model.generate(num_beams=1, repetition_penalty=p, use_graphs=False, **kw)
    keys = list(model._decode_sessions)
    assert len(keys) == 1 + n and len(keys[0]) == G._DECODE_KEY_LEN
    assert [k[-1] for k in keys[1:]] == [G._f32(p) for p in pens[2:]]
    model.generate(num_beams=1, repetition_penalty=pens[2], use_graphs=False, **kw)          # used again: the most recent one now
    model.generate(num_beams=1, repetition_penalty=pens[0], use_graphs=False, **kw)          # a new one: pens[3] goes, not pens[2]
    keys = list(model._decode_sessions)
    assert len(keys) == 1 + n and [k[-1] for k in keys[-2:]] == [G._f32(pens[2]), G._f32(pens[0])]
    assert G._f32(pens[3]) not in [k[-1] for k in keys[1:]]
    assert torch.equal(model.generate(num_beams=1, **kw), free)
    model.__dict__.pop("_decode_sessions", None)


@gpu
def test_generate_sampling_with_both_processors(K):
    model, kw = generation_inputs(K)
    model.__dict__.pop("_sample_sessions", None)
    skw = dict(do_sample=True, num_return_sequences=4, top_k=50, temperature=1.2, seed=7, **kw)
    free = model.generate(**skw)
    assert all(len(k) == 7 for k in model._sample_sessions)                     # the session key of before
    f = free[0].tolist()
    words = [[f[2]], [f[1], f[2]], [free[1, 1].item(), free[1, 2].item()], [2]]
    # (the synthetic model is sharp: a penalty near 1 leaves the top token at probability 1, so the partner of 0.7 is searched for)
    ref = {p: model.generate(use_graphs=False, repetition_penalty=p, bad_words_ids=words, **skw) for p in (0.7, 1.3, 3.0, 8.0, 30.0)}
    hi = next(p for p in (1.3, 3.0, 8.0, 30.0) if not torch.equal(ref[p], ref[0.7]))
    assert len(model._sample_sessions) == 2
    for rnd in range(3):                                                        # eager, capture, replay — alternating on ONE session
        for p in (hi, 0.7):
            got, lp = model.generate(repetition_penalty=p, bad_words_ids=words, return_logprobs=True, **skw)
            assert torch.equal(got, ref[p]), (rnd, p, got.tolist(), ref[p].tolist())
            assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all())
    assert len(model._sample_sessions) == 2                                     # the penalty is a runtime parameter, the words are in the key
    for p in (hi, 0.7):
        for row in ref[p].tolist():
            row = [t for t in row if t != 1]
            assert not any(contains(row[1:] if len(w) == 1 else row, w) for w in words[:3]), (p, row, words)
    assert torch.equal(model.generate(**skw), free)


# ------------------------------------------------------------------------------------------------ vacnic_beam_topk_ex / vacnic_lmhead_topk
def penalty_reference(l64, l32, hist, pen, rule, mask, bs):
    """final scores [R, V] of vacnic_beam_topk_ex in float64 and in fp32 torch (the yardstick of the margin): penalty on the logits
    (rule "logits") or on the log-softmax of the unpenalised row ("scores"), banned tokens -inf, + beam score"""
    out = []
    for x, p in ((l64, float(F32(pen))), (l32, float(F32(pen)))):
        x = x.clone()
        p = torch.tensor(p, dtype=x.dtype)
        if rule == "scores":
            x = torch.log_softmax(x, -1)
        for r in range(x.shape[0]):
            idx = torch.tensor(sorted({int(t) for t in hist[r] if 0 <= int(t) < x.shape[1]}))
            v = x[r, idx]
            x[r, idx] = torch.where(v < 0, v * p, v / p)
        if rule == "logits":
            x = torch.log_softmax(x, -1)
        x = x.masked_fill(mask, -float("inf"))
        out.append(x + (0 if bs is None else bs.to(x.dtype)[:, None]))
    return out


def decidable_order(f64, f32, hist, K_, what):
    """the reference picks [R, K_] under (score desc, token asc) and the margin (margin_of of tests/test_decode_gpu.py: float64
    against fp32 torch).  Asserts that the picks are decidable: with kth = the K-th best score, only the tokens scoring >= kth - 4
    margins can be picked by a kernel that is within the margin; among those, every penalised token is further than 4 margins from
    every other one.  (The unpenalised tokens keep the order of their raw logits, ties included, whatever the rounding.)"""
    import test_decode_gpu as D
    margin, _ = D.margin_of(f64, f32.to(torch.float64), what)
    order = np.argsort(-f64.numpy(), axis=1, kind="stable")[:, :K_]
    for r in range(f64.shape[0]):
        row = f64[r].numpy()
        near = np.nonzero(row >= row[order[r, -1]] - 4 * margin)[0]
        pen_set = {int(t) for t in hist[r]}
        for t in sorted(pen_set & set(near.tolist())):
            # (two penalised tokens with the same raw logit — bf16 rows have many — get the same score in every arithmetic: the tie
            # is broken by the token id on both sides)
            others = [o for o in near.tolist() if o != t and not (o in pen_set and row[o] == row[t])]
            gap = np.abs(row[others] - row[t]).min()
            assert gap > 4 * margin, (what, r, t, gap, margin)
    return torch.from_numpy(order), margin


def topk_case(R, V, K_, dtype, seed, cur=7):
    """random rows whose histories hold tokens of the unpenalised top K (first, third, the last two), two from further down, one twice"""
    g = torch.Generator().manual_seed(seed)
    raw = (torch.randn(R, V, generator=g) * 2).to(dtype)
    srt = torch.argsort(raw.float(), dim=1, descending=True, stable=True)
    pick = torch.tensor([0, 2, K_ - 1, K_ - 2, min(K_ + 3, V - 1), V // 2])
    hist = torch.cat([srt[:, pick], srt[:, :1]], dim=1)[:, :cur].to(torch.int32)            # [R, 7]: the top token occurs twice
    bans = torch.randint(0, V, (R, 6), generator=g, dtype=torch.int32)
    bans[:, 0] = hist[:, 1]                                                                 # a penalised token that is also banned
    bans[:, 3] = -1
    bs = torch.randn(R, generator=g)
    return raw, hist, bans, bs


def check_topk_penalty(K, what, raw, hist, bans, bs, K_, rule, pen, suppress=False, eos=2):
    import test_decode_gpu as D
    R, V = raw.shape
    mask = torch.from_numpy(D.ban_mask(R, V, bans, eos, suppress))
    f64, f32 = penalty_reference(raw.to(torch.float64), raw.to(torch.float32), hist.tolist(), pen, rule, mask, bs)
    want_i, margin = decidable_order(f64, f32, hist.tolist(), K_, what)
    lg = D.padded(raw, (V + 7) // 8 * 8 + 8).cuda()
    tv, ti = K.beam_topk(lg, V, K_, beam_scores=bs.cuda(), bans=bans.cuda(), eos=eos, suppress_eos=suppress, history=hist.cuda(),
                         cur_len=hist.shape[1], repetition_penalty=pen, penalty_rule=rule)
    torch.cuda.synchronize()
    tv, ti = tv.cpu(), ti.cpu().long()
    assert torch.equal(ti, want_i), (what, (ti != want_i).nonzero()[:5].tolist(), ti[ti != want_i][:5].tolist(), want_i[ti != want_i][:5].tolist())
    want = f64.gather(1, want_i)
    assert bool(torch.isfinite(want).all())
    err = (tv.to(torch.float64) - want).abs().max().item()
    D.report(f"beam_topk penalty {what} {rule} p={pen} R={R} V={V} K={K_}", margin, err)
    assert err <= margin, (what, err, margin)
    # what the penalty did to the unpenalised top K: dropped out / moved / banned
    free = np.argsort(-np.where(mask.numpy(), -np.inf, raw.to(torch.float64).numpy()), axis=1, kind="stable")[:, :K_]
    ev = dict(dropped=0, moved=0, banned=0)
    for r in range(R):
        fr, wr = free[r].tolist(), want_i[r].tolist()
        for t in {int(t) for t in hist[r].tolist()}:
            ev["banned"] += bool(mask[r, t])
            if t in fr and not mask[r, t]:
                ev["dropped"] += t not in wr
                ev["moved"] += t in wr and wr.index(t) != fr.index(t)
    return ev


TOPK_SHAPES = ((5, 1000, 10, 1.3), (5, 1000, 300, 1.3), (80, 50265, 10, 1.3), (5, 50265, 300, 0.7), (5, 2048, 1025, 1.3))
TOPK_SEED = {10: 1, 300: 1, 1025: 4}      # found on the host: the references of these rows are decidable (decidable_order asserts it)


@gpu
@pytest.mark.parametrize("rule", ["logits", "scores"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_beam_topk_penalty_matches_float64(K, rule, dtype):
    tot = dict(dropped=0, moved=0, banned=0)
    for R, V, K_, pen in TOPK_SHAPES:
        raw, hist, bans, bs = topk_case(R, V, K_, dtype, seed=TOPK_SEED[K_])      # K = 1025: the generic kernel
        ev = check_topk_penalty(K, f"K{K_}", raw, hist, bans, bs, K_, rule, pen)
        for k in tot:
            tot[k] += ev[k]
    assert tot["dropped"] > 0 and tot["moved"] > 0 and tot["banned"] > 0, tot
    # penalised eos under suppress_eos: eos is in the history (BART's start token) and stays out
    raw, hist, bans, bs = topk_case(5, 1000, 10, dtype, seed=3)
    hist[:, 0] = 2
    raw[:, 2] = raw.max() + 1
    check_topk_penalty(K, "eos", raw, hist, bans, bs, 10, rule, 1.3, suppress=True)
    ev = check_topk_penalty(K, "eos free", raw, hist, bans, bs, 10, rule, 50.0)     # unsuppressed, a penalty of 50 drops it from the top
    assert ev["dropped"] >= 5
    # a forced position: the penalty is irrelevant, the result is vacnic_beam_topk's
    lg = raw.cuda()
    a = K.beam_topk(lg, 1000, 10, beam_scores=bs.cuda(), forced_token=7)
    b = K.beam_topk(lg, 1000, 10, beam_scores=bs.cuda(), forced_token=7, history=hist.cuda(), cur_len=7, repetition_penalty=1.3, penalty_rule=rule)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # penalty 1.0 through the new entry point is the old call, bit for bit
    a = K.beam_topk(lg, 1000, 10, beam_scores=bs.cuda(), bans=bans.cuda())
    b = K.beam_topk(lg, 1000, 10, beam_scores=bs.cuda(), bans=bans.cuda(), history=hist.cuda(), cur_len=7, repetition_penalty=1.0, penalty_rule=rule)
    assert torch.equal(a[1], b[1]) and (rule == "scores" or torch.equal(a[0], b[0]))
    from vacnic_amd import _lib
    for kw, exc, pat in ((dict(history=None), ValueError, "null operand"), (dict(repetition_penalty=0.0), ValueError, "finite number > 0"),
                         (dict(cur_len=0), ValueError, "cur_len"), (dict(cur_len=8), ValueError, "cur_len")):
        with pytest.raises(exc, match=pat):
            K.beam_topk(lg, 1000, 10, **dict(dict(history=hist.cuda(), cur_len=7, repetition_penalty=1.3, penalty_rule=rule), **kw))
    with pytest.raises(_lib.VacnicError, match="at most 1024"):
        K.beam_topk(lg, 1000, 10, history=torch.zeros(5, 1100, dtype=torch.int32).cuda(), cur_len=1025, repetition_penalty=1.3, penalty_rule=rule)


def tail_case(seed=5, R=2, V=1100, nban=201):
    """rows with fewer finite scores than K: nban distinct tokens are banned; the history holds the best token (twice), a token from
    the middle and a banned token -> V - nban finite scores per row"""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(R, V, generator=g) * 2
    srt = torch.argsort(raw, dim=1, descending=True, stable=True)
    bans = torch.stack([srt[r, 3:][torch.randperm(V - 3, generator=g)[:nban]] for r in range(R)]).to(torch.int32)
    live = [[t for t in srt[r].tolist() if t not in set(bans[r].tolist())] for r in range(R)]
    hist = torch.tensor([[live[r][0], live[r][len(live[r]) // 2], int(bans[r, 7]), live[r][0]] for r in range(R)], dtype=torch.int32)
    return raw, hist, bans, torch.randn(R, generator=g), V - nban


@gpu
@pytest.mark.parametrize("K_", [1000, 1050], ids=["threshold-kernel", "generic-kernel"])
def test_beam_topk_scores_rule_behind_the_last_finite_score(K, K_):
    """rule 2 with fewer finite scores than K: the finite ones in order, then (-inf, -1), from the threshold kernel (K <= 1024) and
    from the generic one alike"""
    import test_decode_gpu as D
    raw, hist, bans, bs, n = tail_case()
    R, V = raw.shape
    mask = torch.from_numpy(D.ban_mask(R, V, bans, 2, False))
    f64, f32 = penalty_reference(raw.to(torch.float64), raw.clone(), hist.tolist(), 1.3, "scores", mask, bs)
    assert bool((torch.isfinite(f64).sum(1) == n).all())
    want_i, margin = decidable_order(f64, f32, hist.tolist(), n, f"tail K{K_}")
    tv, ti = K.beam_topk(D.padded(raw, V + 12).cuda(), V, K_, beam_scores=bs.cuda(), bans=bans.cuda(), eos=2, history=hist.cuda(),
                         cur_len=hist.shape[1], repetition_penalty=1.3, penalty_rule="scores")
    torch.cuda.synchronize()
    tv, ti = tv.cpu(), ti.cpu().long()
    assert torch.equal(ti[:, :n], want_i), ((ti[:, :n] != want_i).nonzero()[:5].tolist())
    assert (tv[:, :n].to(torch.float64) - f64.gather(1, want_i)).abs().max().item() <= margin
    assert bool((ti[:, n:] == -1).all()) and bool((tv[:, n:] == -float("inf")).all()), (ti[:, n:].tolist(), tv[:, n:].tolist())


def lm_history(t, V):
    """histories for the fused tail: tokens at the edges of the part kernel's column ranges (the last column of a workgroup, the first
    of the next, 127 / 128, V - 1), three more in ONE workgroup's range, the token that heads workgroup 1's list unpenalised, and the
    row's best token twice"""
    import test_decode_gpu as D
    tpw, G, cols = D.lm_geometry(V)
    l64 = t["h"].to(torch.float64) @ t["emb"][:V, :t["d"]].to(torch.float64).t() + t["bias"].to(torch.float64)
    head = l64[:, cols:2 * cols].argmax(1) + cols
    best = l64.argmax(1)
    R = t["R"]
    fixed = torch.tensor([cols - 1, cols, 127, 128, V - 1, 3 * cols + 1, 3 * cols + 2])
    hist = torch.cat([fixed[None].expand(R, -1), head[:, None], best[:, None], best[:, None]], dim=1)
    return l64, hist.to(torch.int32)


@gpu
@pytest.mark.parametrize("rule", ["logits", "scores"])
@pytest.mark.parametrize("V,R,K2", [(1000, 1, 2), (1000, 8, 32), (50265, 8, 2), (50265, 1, 32), (50265, 8, 32)])
def test_lmhead_topk_penalty_matches_float64_and_the_chain(K, rule, V, R, K2):
    import test_decode_gpu as D
    d = 64
    t = D.lm_inputs(V, d, R, seed=V + R + K2)
    l64, hist = lm_history(t, V)
    cur = hist.shape[1]
    g = torch.Generator().manual_seed(V + K2)
    bans = torch.randint(0, V, (R, 5), generator=g, dtype=torch.int32)
    bans[:, 0] = hist[:, 2]                                                       # token 127: penalised and banned
    for pen, suppress in ((1.3, False), (0.7, True)):
        what = f"lmhead penalty {rule} p={pen} V={V} R={R} K2={K2}"
        mask = torch.from_numpy(D.ban_mask(R, V, bans, 2, suppress))
        l32 = t["h"].to(torch.float32) @ t["emb"][:V, :d].to(torch.float32).t() + t["bias"]
        f64, f32 = penalty_reference(l64, l32, hist.tolist(), pen, rule, mask, t["bs"])
        want_i, margin = decidable_order(f64, f32, hist.tolist(), K2, what)
        emb_d, h_d = t["emb"].cuda()[:, :d], t["h"].cuda()
        kw = dict(beam_scores=t["bs"].cuda(), bans=bans.cuda(), eos=2, suppress_eos=suppress, history=hist.cuda(), cur_len=cur,
                  repetition_penalty=pen, penalty_rule=rule)
        lg = torch.full((R, t["Vp"] + 8), 7.0, device="cuda")
        tv, ti = K.lmhead_topk(h_d, emb_d, V, K2, bias=t["bias"].cuda(), logits=lg, **kw)
        tv_n, ti_n = K.lmhead_topk(h_d, emb_d, V, K2, bias=t["bias"].cuda(), **kw)
        ct, ci = K.beam_topk(lg, V, K2, **kw)                                     # the unfused chain on the logits written out
        lg0 = torch.full_like(lg, 7.0)
        K.lmhead_topk(h_d, emb_d, V, K2, bias=t["bias"].cuda(), logits=lg0, beam_scores=t["bs"].cuda(), bans=bans.cuda(), eos=2, suppress_eos=suppress)
        torch.cuda.synchronize()
        assert torch.equal(lg, lg0), (what, "the logits output must stay unpenalised")
        assert torch.equal(ti, ti_n) and torch.equal(tv, tv_n), (what, "the logits output changes the result")
        assert torch.equal(ti, ci), (what, "ids differ from the unfused chain", ti.tolist(), ci.tolist())
        assert torch.equal(ti.cpu().long(), want_i), (what, ti.tolist(), want_i.tolist())
        err = (tv.cpu().to(torch.float64) - f64.gather(1, want_i)).abs().max().item()
        D.report(what, margin, err)
        assert err <= margin, (what, err, margin)
        assert (tv.cpu() - ct.cpu()).abs().max().item() <= margin, what
    assert int(__import__("vacnic_amd")._lib.lib.vacnic_lmhead_topk_supported(R, V, d, K2)) == 1
