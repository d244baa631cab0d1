"""CPU: the repetition penalty and the bad-word bans of generate() — the HOST MODELS that the GPU tests import
(tests/test_decode_processors_gpu.py), the argument checks of generate(), the unchanged defaults, and the status codes of the new
arguments of the C entry points.

The host models are written from include/vacnic_hip.h (the bad-word table comment, vacnic_sample_step step 1, vacnic_beam_topk_ex):
  * host_bad_words: transformers 4.18's NoBadWordsLogitsProcessor — a word of m tokens bans its last token when its first m - 1
    tokens end the history; a one-token word always; a prefix as long as the WHOLE history matches; the word [eos] is dropped.
  * host_repetition_penalty, rule "logits": fp32, one IEEE operation per DISTINCT history token on the raw logits (exact: the
    sampling kernel is replayed bit for bit).  Rule "scores": float64 log-softmax of the UNPENALISED row, then the same rule on the
    scores (HF beam_search); the GPU tests compare it under the float64-against-fp32 margin of tests/test_decode_gpu.py."""
import struct

import numpy as np
import pytest
import torch

F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ host models
def host_bad_words(history, words, eos):
    """the tokens NoBadWords bans for the position after `history` (its decoder input so far, start token included): sorted, distinct"""
    h = [int(t) for t in history]
    out = set()
    for w in words:
        w = [int(t) for t in w]
        if w == [eos]:
            continue
        m = len(w)
        if m - 1 <= len(h) and (m == 1 or h[len(h) - (m - 1):] == w[:-1]):
            out.add(w[-1])
    return sorted(out)


def host_repetition_penalty(z, history, p, rule):
    """one row.  rule "logits": fp32 raw logits in, fp32 penalised logits out (NaN -> -inf and +inf -> FLT_MAX for the history tokens
    first).  rule "scores": raw logits in, float64 penalised log-softmax scores out (the log-sum-exp is the unpenalised row's)."""
    hist = sorted({int(t) for t in history if 0 <= int(t) < len(z)})
    if rule == "logits":
        out = np.array(z, dtype=F32)
        pf = F32(p)
        with np.errstate(over="ignore", invalid="ignore"):
            for j in hist:
                v = out[j]
                v = F32(-np.inf) if np.isnan(v) else min(v, np.finfo(F32).max)
                out[j] = F32(v * pf) if v < 0 else F32(v / pf)
        return out
    assert rule == "scores"
    x = np.asarray(z).astype(F64)
    m = x[np.isfinite(x)].max()
    s = x - (m + np.log(np.exp(x - m).sum()))
    pd = F64(F32(p))
    for j in hist:
        s[j] = s[j] * pd if s[j] < 0 else s[j] / pd
    return s


# ------------------------------------------------------------------------------------------------ the host models on hand-made rows
def test_repetition_penalty_hand_rows():
    ninf = -np.inf
    z = np.array([2.0, -1.0, 0.0, ninf, 3.0, -4.0, 0.5], F32)
    # token 4 three times in the history: penalised ONCE; z = 0 stays 0 (0 / p); -inf stays -inf; tokens outside the history untouched
    got = host_repetition_penalty(z, [4, 1, 4, 2, 3, 4], 2.0, "logits")
    assert got.dtype == F32 and got.tolist() == [2.0, -2.0, 0.0, ninf, 1.5, -4.0, 0.5]
    # p < 1 rewards repetition: positive logits grow, negative ones shrink towards 0
    got = host_repetition_penalty(z, [0, 5], 0.5, "logits")
    assert got.tolist() == [4.0, -1.0, 0.0, ninf, 3.0, -2.0, 0.5]
    # one fp32 operation: 1 / 1.3 is the correctly rounded quotient, not a product with a rounded reciprocal
    one = host_repetition_penalty(np.array([1.0, -1.0], F32), [0, 1], 1.3, "logits")
    assert one[0] == F32(1.0) / F32(1.3) and one[1] == F32(-1.0) * F32(1.3)
    # NaN and +inf of a history token are mapped first
    odd = host_repetition_penalty(np.array([np.nan, np.inf, np.nan], F32), [0, 1], 2.0, "logits")
    assert odd[0] == ninf and odd[1] == np.finfo(F32).max / 2 and np.isnan(odd[2])
    # scores rule: log-softmax of the UNPENALISED row, then s' = s * p for s < 0 (every score of a proper row)
    zz = np.array([0.0, np.log(2.0), np.log(5.0)], F64)                     # probabilities 1/8, 2/8, 5/8
    s = host_repetition_penalty(zz, [1, 1, 2], 2.0, "scores")
    assert np.allclose(s, [np.log(1 / 8), 2 * np.log(2 / 8), 2 * np.log(5 / 8)], rtol=1e-12, atol=0)
    # a penalised token can change its rank: 5/8 -> (5/8)^2 = .39 stays first, 2/8 -> 1/16 drops below 1/8
    assert np.argsort(-s).tolist() == [2, 0, 1] and np.argsort(-host_repetition_penalty(zz, [], 2.0, "scores")).tolist() == [2, 1, 0]
    # a certain token has s = 0: 0 / p = 0; -inf stays -inf
    s = host_repetition_penalty(np.array([ninf, 7.0, ninf]), [0, 1], 1.7, "scores")
    assert s.tolist() == [ninf, 0.0, ninf]


def test_bad_words_hand_rows():
    EOS = 2
    words = [[7], [5, 6, 9], [2, 8], [6, 3], [EOS], [7], [6, 3]]             # [eos] is dropped; duplicates are harmless
    assert host_bad_words([2], words, EOS) == [7, 8]                           # the prefix [2] is the WHOLE history: it matches (4.18)
    assert host_bad_words([2, 5, 6], words, EOS) == [3, 7, 9]                   # [5, 6] -> 9 and [6] -> 3
    assert host_bad_words([2, 5], words, EOS) == [7]                            # [5, 6, 9] needs two history tokens to match
    assert host_bad_words([5, 6], words, EOS) == [3, 7, 9]                      # ... and matches a history of exactly two
    assert host_bad_words([6], [[5, 6, 9]], EOS) == []                          # a word longer than history + 1 never matches
    assert host_bad_words([2, 4], [[EOS]], EOS) == [] and host_bad_words([2, 4], [[EOS, EOS]], EOS) == []
    assert host_bad_words([2, EOS], [[EOS, EOS]], EOS) == [EOS]                 # only the one-token word [eos] is dropped
    from vacnic_amd.generate import _bad_word_bans
    rng = np.random.default_rng(0)
    for _ in range(200):                                                        # generate()'s host beam loop computes the same sets
        h = rng.integers(0, 4, size=rng.integers(1, 7)).tolist()
        ws = [tuple(rng.integers(0, 4, size=rng.integers(1, 5)).tolist()) for _ in range(5)]
        ws = [w for w in ws if w != (EOS,)]
        assert sorted(set(_bad_word_bans(h, ws))) == host_bad_words(h, ws, EOS)


def test_host_models_against_transformers_processors():
    """guards the host models on rows where 4.18 and later transformers agree: histories strictly longer than every word's prefix,
    ids below V (later versions do not match a prefix that is the whole history, and raise for ids >= V)"""
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(7)
    V, EOS = 40, 2
    for trial in range(20):
        L = int(rng.integers(5, 12))
        hist = rng.integers(0, 8, size=L).tolist()
        z = rng.normal(0, 2, size=V).astype(F32)
        z[int(rng.integers(0, V))] = 0.0
        ids, s = torch.tensor([hist]), torch.from_numpy(z)[None]
        for p in (1.3, 0.7):
            want = lp.RepetitionPenaltyLogitsProcessor(float(p))(ids, s.clone())[0].numpy()
            assert np.array_equal(host_repetition_penalty(z, hist, p, "logits"), want), (trial, p)
            lsm = torch.log_softmax(s.double(), -1)
            want = lp.RepetitionPenaltyLogitsProcessor(float(F32(p)))(ids, lsm.clone())[0].numpy()
            assert np.allclose(host_repetition_penalty(z, hist, p, "scores"), want, rtol=1e-12, atol=1e-12), (trial, p)
        words = [[int(rng.integers(0, V))], hist[-2:] + [11], hist[-1:] + [12], hist[-3:-1] + [13], [hist[-1], 14, 15], [EOS], [9, 9, 9, 16]]
        out = lp.NoBadWordsLogitsProcessor(words, eos_token_id=EOS)(ids, s.clone())[0].numpy()
        assert np.nonzero(np.isinf(out))[0].tolist() == host_bad_words(hist, words, EOS), trial
        assert {11, 12} <= set(host_bad_words(hist, words, EOS)) and 14 not in host_bad_words(hist, words, EOS)


# ------------------------------------------------------------------------------------------------ generate(): refusals, defaults
class _Cfg:
    eos_token_id, pad_token_id, decoder_start_token_id, vocab_size = 2, 1, 2, 100


class _NoModel:
    """a model that was never finalized: generate() reaches `model.arena is None` only after its argument checks"""
    config, V, arena = _Cfg(), 100, None


@pytest.mark.parametrize("mode", [dict(do_sample=False, num_beams=1), dict(do_sample=False, num_beams=4), dict(do_sample=True, num_beams=1)],
                         ids=["greedy", "beams", "sample"])
def test_generate_processor_refusals(mode):
    from vacnic_amd import kernels as K
    from vacnic_amd.generate import generate
    # (1e39 is inf and 1e-50 is 0 as the float32 the kernels take)
    for bad in (0, 0.0, -1.5, float("nan"), float("inf"), "1.2", None, True, 1e39, 1e-50, 10 ** 400, np.float32(0), np.float64("inf"), 1 + 2j):
        with pytest.raises(ValueError, match="repetition_penalty"):
            generate(_NoModel(), repetition_penalty=bad, **mode)
    for bad in ([], (), "ab", 5, {}):
        with pytest.raises(ValueError, match="non-empty list"):
            generate(_NoModel(), bad_words_ids=bad, **mode)
    for bad in ([[]], [[3], []], [3, 4], [[3], 4], ["ab"]):
        with pytest.raises(ValueError, match="list of non-empty lists"):
            generate(_NoModel(), bad_words_ids=bad, **mode)
    for bad in ([[-1]], [[3, 100]], [[3.0]], [[True]], [[3], ["4"]]):
        with pytest.raises(ValueError, match=r"integers in \[0, 100\)"):
            generate(_NoModel(), bad_words_ids=bad, **mode)
    # capacity: BAD_WORDS_MAX words of BAD_WORD_LEN tokens pass the checks (and reach the model), one more of either does not
    assert K.BAD_WORDS_MAX >= 256 and K.BAD_WORD_LEN >= 16
    full = [[i // 100, i % 100] + [7] * (i % (K.BAD_WORD_LEN - 1)) for i in range(K.BAD_WORDS_MAX)]
    assert max(len(w) for w in full) == K.BAD_WORD_LEN
    assert len({tuple(w) for w in full}) == K.BAD_WORDS_MAX
    with pytest.raises(RuntimeError, match="finalize"):
        generate(_NoModel(), bad_words_ids=full, **mode)
    with pytest.raises(RuntimeError, match="finalize"):                          # [eos] and duplicates do not count
        generate(_NoModel(), bad_words_ids=full + [[2]] + full[:5], **mode)
    with pytest.raises(ValueError, match="at most"):
        generate(_NoModel(), bad_words_ids=full + [[99, 98, 97]], **mode)
    with pytest.raises(ValueError, match="at most"):
        generate(_NoModel(), bad_words_ids=[[5] * (K.BAD_WORD_LEN + 1)], **mode)
    # valid values pass the checks and reach the model; values below 1 are legal
    import fractions
    for p in (1.3, 0.7, 2, 1.0, np.float32(1.3), np.float64(0.7), np.int64(2), fractions.Fraction(13, 10), 1e38, 1e-38):
        with pytest.raises(RuntimeError, match="finalize"):
            generate(_NoModel(), repetition_penalty=p, bad_words_ids=[[50], [3, 4]], **mode)


def test_defaults_write_the_parameter_block_of_before():
    import struct
    from vacnic_amd import kernels as K
    a = K.sample_params(0.75, 40, 0.9, seed=(5 << 32) | 7, call=(1 << 32) | 3)
    b = K.sample_params(0.75, 40, 0.9, seed=(5 << 32) | 7, call=(1 << 32) | 3, repetition_penalty=1.0)
    assert torch.equal(a, b) and int(a[3]) == 0                                 # word [3] stays the reserved 0: "off"
    c = K.sample_params(0.75, 40, 0.9, seed=(5 << 32) | 7, call=(1 << 32) | 3, repetition_penalty=1.3)
    assert torch.equal(c[[0, 1, 2, 4, 5, 6, 7]], a[[0, 1, 2, 4, 5, 6, 7]])
    assert struct.unpack("<f", struct.pack("<i", int(c[3])))[0] == struct.unpack("<f", struct.pack("<f", 1.3))[0]


def test_defaults_keep_the_session_keys_of_before():
    from vacnic_amd import generate as G
    lp = (2.0, False)
    assert G._decode_session_key(5, 512, 50, 5, 3, 0, 2, None, lp, None, 1.0) == (5, 512, 50, 5, 3, 0, 2, None, lp)
    assert G._decode_session_key(5, 512, 50, 5, 3, 0, 2, None, None, None, G._f32(1 + 1e-12)) == (5, 512, 50, 5, 3, 0, 2, None, None)
    assert len(G._decode_session_key(5, 512, 50, 5, 3, 0, 2, None, lp, None, 1.0)) == G._DECODE_KEY_LEN
    assert G._decode_session_key(5, 512, 50, 5, 3, 0, 2, None, lp, None, G._f32(1.3)) == (5, 512, 50, 5, 3, 0, 2, None, lp, None, G._f32(1.3))
    assert G._decode_session_key(5, 512, 50, 5, 3, 0, 2, None, lp, ((7,),), 1.0) == (5, 512, 50, 5, 3, 0, 2, None, lp, ((7,),), 1.0)
    assert G._sample_session_key(4, 512, 50, 3, 0, 2, None, None) == (4, 512, 50, 3, 0, 2, None)
    assert G._sample_session_key(4, 512, 50, 3, 0, 2, None, ((7,), (3, 4))) == (4, 512, 50, 3, 0, 2, None, ((7,), (3, 4)))
    assert G._f32(1.3) == struct.unpack("<f", struct.pack("<f", 1.3))[0] and G._f32(1e39) == float("inf") and G._f32(1e-50) == 0.0


def test_bad_words_table_layout():
    from vacnic_amd import kernels as K
    tab, lens = K.bad_words_table([(7,), (5, 6, 9)], device="cpu")
    assert tab.dtype == torch.int32 and tab.shape == (2, K.BAD_WORD_LEN) and lens.tolist() == [1, 3]
    assert tab[0].tolist() == [7] + [-1] * (K.BAD_WORD_LEN - 1) and tab[1, :4].tolist() == [5, 6, 9, -1]
    for bad in ([], [()], [(1,) * (K.BAD_WORD_LEN + 1)], [(1,)] * (K.BAD_WORDS_MAX + 1)):
        with pytest.raises(ValueError, match="bad_words_table"):
            K.bad_words_table(bad, device="cpu")
    import re
    hdr = open(__file__.replace("tests/test_decode_processors.py", "include/vacnic_hip.h")).read()
    assert int(re.search(r"#define VACNIC_BAD_WORDS_MAX (\d+)", hdr).group(1)) == K.BAD_WORDS_MAX
    assert int(re.search(r"#define VACNIC_BAD_WORD_LEN (\d+)", hdr).group(1)) == K.BAD_WORD_LEN


# ------------------------------------------------------------------------------------------------ C entry points: status, no abort
def test_new_arguments_return_status(built_lib):
    from vacnic_amd import _lib
    good = dict(logits=16, params=16, seq=16, done=16, next_ids=16, logp=16, kept=None, thr=None, mass=None, u=None, R=2, V=100, ldl=104,
                Lmax=8, cur_len=1, eos=2, pad=1, no_repeat_ngram_size=0, suppress_eos=0, forced_token=-1)

    def sample(**kw):
        _lib.call_struct("vacnic_sample_step", stream=None, **dict(good, **kw))
    for n in (-1, 1025):
        with pytest.raises(_lib.VacnicError, match="bad words"):
            sample(bad_words=16, bad_len=16, n_bad=n)
    for kw in (dict(bad_words=None, bad_len=16), dict(bad_words=16, bad_len=None)):
        with pytest.raises(ValueError, match="null operand"):
            sample(n_bad=3, **kw)
    beam = dict(seq0=16, seq1=16, beam_scores=16, done=16, hyp_cnt=16, hyp_worst=16, hyp_score=16, hyp_len=16, hyp_seq=16, next_ids=16,
                src_idx=16, bans=16, B=1, nb=2, Lmax=8, V=100, eos=2, pad=1, no_repeat_ngram_size=0, early_stopping=0, length_penalty=1.0)

    def init(**kw):
        _lib.check(_lib.lib.vacnic_beam_init(_lib.C.byref(_lib.BeamState(**dict(beam, **kw))), 2, None))

    def step(**kw):
        _lib.check(_lib.lib.vacnic_beam_step(_lib.C.byref(_lib.BeamState(**dict(beam, **kw))), 16, 16, 4, 1, None))
    for fn in (init, step):
        for n in (-1, 1025):
            with pytest.raises(_lib.VacnicError, match="bad words"):
                fn(bad_words=16, bad_len=16, n_bad=n)
        for kw in (dict(bad_words=None, bad_len=16), dict(bad_words=16, bad_len=None), dict(bad_words=16, bad_len=16, bans=None)):
            with pytest.raises(ValueError, match="null operand"):
                fn(n_bad=3, **kw)


def test_penalty_arguments_return_status(built_lib):
    from vacnic_amd import _lib
    assert "vacnic_beam_topk_ex" in _lib.EXPORTED
    good = dict(logits=16, beam_scores=None, bans=None, top_val=16, top_idx=16, history=16, R=2, V=100, ldl=104, hist_stride=8, n_ban=0, eos=2,
                suppress_eos=0, forced_token=-1, K=4, logits_f32=1, cur_len=3, penalty_rule=2, penalty=1.3)

    def topk(**kw):
        _lib.call_struct("vacnic_beam_topk_ex", stream=None, **dict(good, **kw))
    for kw, pat in ((dict(logits=None), "null operand"), (dict(history=None), "null operand"), (dict(K=101), "bad V/ldl/K"),
                    (dict(penalty_rule=3), "penalty_rule"), (dict(penalty_rule=-1), "penalty_rule"), (dict(penalty=0.0), "finite number > 0"),
                    (dict(penalty=-1.0), "finite number > 0"), (dict(penalty=float("inf")), "finite number > 0"),
                    (dict(penalty=float("nan")), "finite number > 0"), (dict(cur_len=0), "cur_len"), (dict(cur_len=9), "cur_len")):
        with pytest.raises(ValueError, match=pat):
            topk(**kw)
    with pytest.raises(_lib.VacnicError, match="at most 1024"):
        topk(cur_len=1025, hist_stride=2000)
    topk(R=0)                                                                   # nothing to do: no launch, no error
    lm = dict(h=16, emb=16, bias=None, logits=None, workspace=16, beam_scores=None, bans=None, top_val=16, top_idx=16, R=2, V=100, d=64, ldw=64,
              ldl=0, workspace_floats=10 ** 6, n_ban=0, eos=2, suppress_eos=0, forced_token=-1, K2=4, cur_len=3, penalty_rule=2, penalty=1.3,
              history=16, hist_stride=8)

    def lmhead(**kw):
        _lib.call_struct("vacnic_lmhead_topk", stream=None, **dict(lm, **kw))
    for kw, pat in ((dict(history=None), "null operand"), (dict(penalty_rule=3), "penalty_rule"), (dict(penalty=0.0), "finite number > 0"),
                    (dict(cur_len=0), "cur_len"), (dict(cur_len=9), "cur_len")):
        with pytest.raises(ValueError, match=pat):
            lmhead(**kw)
    with pytest.raises(_lib.VacnicError, match="at most 1024"):
        lmhead(cur_len=1025, hist_stride=2000)
    # the scores rule parks the history tokens' logits behind the partial results: R * hist_stride more floats of workspace
    base = int(_lib.lib.vacnic_lmhead_topk_workspace(2, 100, 4))
    with pytest.raises(ValueError, match="workspace of"):
        lmhead(workspace_floats=base + 2 * 8 - 1)
    for shape in ((5, 50265, 1024, 10), (8, 50265, 1024, 45), (8, 50265, 1024, 46), (9, 50265, 1024, 10), (1, 17, 8, 1)):
        assert int(_lib.lib.vacnic_lmhead_topk_supported(*shape)) == int(shape[0] <= 8 and shape[3] <= 45)      # the answers of before
