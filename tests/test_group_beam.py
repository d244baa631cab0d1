"""Group (diverse) beam search, CPU side: the host model of vacnic_group_beam_init / vacnic_group_beam_step (include/vacnic_hip.h
has the rules; transformers 4.18 group_beam_search + HammingDiversityLogitsProcessor), the argument checks of generate(), the
session key, nbest_to_sequences and the C-ABI's refusals.  tests/test_group_beam_gpu.py runs the device against this model.

HostGroupBeams is written from the header's rules alone and advances over the scripted table of tests/test_decode_gpu.py (table_rows:
scores -q / 256): with lambda in {0.25, 0.5, 1.0} and P in {1, 2, 0.5} every product and sum is exact in fp32, so scores compare
bitwise with the device.  The cases were found by a host-only seed search; what each of them is there for is asserted on the host
model alone (GROUP_EVENTS), as STEP_CASES do it."""
import math

import numpy as np
import pytest
import torch

from test_decode_gpu import EOS, PAD, STEP_CASES, VS, HostBeams, case, make_hyps, run_host, table_rows

NEG = -float("inf")
F = np.float32


def gcase(nb, G, B, lam, P=1.0, lp=1.0, early=False, ngram=0, min_length=0, Lmax=12, seed=0, forced_eos=True, expect=(), **kw):
    c = case(nb, B, lp, early, ngram, min_length, Lmax, seed, expect=expect, **kw)
    c.update(G=G, lam=lam, P=P, forced_eos=forced_eos)
    return c


def gcase_id(c):
    return "nb%d-G%d-B%d-lam%s-P%s-lp%s-%s-ng%d-min%d-L%d" % (c["nb"], c["G"], c["B"], c["lam"], c["P"], c["lp"], "early" if c["early"] else "full",
                                                             c["ngram"], c["min_length"], c["Lmax"])


class HostGroupBeams:
    """vacnic_group_beam_init / vacnic_group_beam_step on the host: the groups of an item in order, one shared hypothesis list and done
    flag per item.  `full=True` merges over the whole [gs, V] score matrix of a group instead of the per-row lists of K2 = min(2 nb, V)
    (the sufficiency argument of the header says both give the same)."""

    def __init__(self, O, c, full=False):
        self.O, self.c, self.B, self.nb, self.G, self.full = O, c, c["B"], c["nb"], c["G"], full
        self.gs = self.nb // self.G
        R = self.B * self.nb
        self.seqs = [[c["start"]] for _ in range(R)]
        self.scores = np.where(np.arange(R) % self.gs == 0, 0.0, -1e9).astype(F)          # slot 0 of every group is live
        self.hyps = [make_hyps(O, self.nb, c["lp"], c["early"]) for _ in range(self.B)]   # ONE list of capacity nb per item
        self.done = [False] * self.B
        self.cur_len = 1
        self.src = list(range(R))
        self.padded = [False] * R                 # the row's group was padded along in the last position: it bans nothing
        self.new_tokens = []                      # per position: {(item, group): tokens} of the groups that were not padded
        self.ev = dict(changed=0, f2=0, done_mid=0, two_groups_add=0, pen_hist=0, forced_skip=0, distinct=True, staggered=False)

    def forced(self):
        return EOS if (self.c["forced_eos"] and self.cur_len == self.c["Lmax"] - 1) else -1

    def penalised(self, lp):
        """the scores-rule repetition penalty and the forced token: what the top-k kernels apply besides bans and MinLength"""
        x = lp.copy()
        P = F(self.c["P"])
        if P != 1:
            for r, s in enumerate(self.seqs):
                for t in set(s):
                    x[r, t] = x[r, t] * P if x[r, t] < 0 else x[r, t] / P
        if self.forced() >= 0:
            x[:] = NEG
            x[:, self.forced()] = 0.0
        return x

    def bans(self):
        return [[] if self.padded[r] else self.O.banned_ngram_tokens(s, self.c["ngram"]) for r, s in enumerate(self.seqs)]

    def processed(self, lp):
        x = self.penalised(lp)
        if self.forced() < 0:
            for r, toks in enumerate(self.bans()):
                for t in toks:
                    x[r, t] = NEG
            if self.cur_len < self.c["min_length"]:
                x[:, EOS] = NEG
        return x

    def process(self, cand, b, r0, commit):
        """BeamSearchScorer.process with group_size gs over the merged candidates (v', key, slot, token), in rank order"""
        gs = self.gs
        chosen, adds = [], []
        for rank, (v, _, i, tok) in enumerate(cand[:2 * gs]):
            if tok == EOS:
                if rank >= gs:
                    continue
                adds.append((r0 + i, v))
                if commit:
                    self.hyps[b].add(self.seqs[r0 + i], float(v))
            else:
                chosen.append((v, tok, r0 + i))
            if len(chosen) == gs:
                break
        return chosen, adds

    def step(self, lp):
        B, nb, G, gs, c = self.B, self.nb, self.G, self.gs, self.c
        lam, P = F(c["lam"]), F(c["P"])
        was_done = list(self.done)
        forced = self.forced() >= 0
        s = self.processed(lp) + self.scores[:, None]                                  # fp32, exact
        Kk = VS if self.full else min(2 * nb, VS)
        order = np.argsort(-s, axis=1, kind="stable")[:, :Kk]                           # (score desc, token asc)
        vals = np.take_along_axis(s, order, 1)
        seqs, scores, src, padded, toks_here = [], [], [], [], {}
        for b in range(B):
            new_tok, adders = [], 0
            for g in range(G):
                r0 = b * nb + g * gs
                if self.done[b]:
                    self.ev["done_mid"] += not was_done[b]                            # an earlier group of this position finished the item
                    seqs += [self.seqs[r0] + [PAD]] * gs; scores += [0.0] * gs; src += [r0] * gs; padded += [True] * gs
                    continue
                cand, plain = [], []
                for i in range(gs):
                    r = r0 + i
                    for k in range(Kk):
                        tok, v = int(order[r, k]), vals[r, k]
                        f = new_tok.count(tok)
                        v2 = v
                        if f > 0 and forced:
                            self.ev["forced_skip"] += 1
                        elif f > 0:
                            h = F(lam * F(f))
                            if P != 1 and tok in self.seqs[r]:
                                h = F(h * P)
                                self.ev["pen_hist"] += bool(np.isfinite(v))
                            v2 = F(v - h)
                            self.ev["f2"] += bool(f >= 2 and np.isfinite(v))
                        cand.append((float(v2), i * VS + tok, i, tok)); plain.append((float(v), i * VS + tok, i, tok))
                cand.sort(key=lambda x: (-x[0], x[1])); plain.sort(key=lambda x: (-x[0], x[1]))
                head = [x[0] for x in cand[:2 * gs + 1]]
                self.ev["distinct"] = self.ev["distinct"] and (forced or len(set(head)) == len(head))
                pick = lambda res: ([(t, r) for _, t, r in res[0]], [r for r, _ in res[1]])
                self.ev["changed"] += pick(self.process(plain, b, r0, False)) != pick(self.process(cand, b, r0, False))
                chosen, adds = self.process(cand, b, r0, True)
                adders += bool(adds)
                self.done[b] = self.done[b] or self.hyps[b].is_done(cand[0][0], self.cur_len)
                while len(chosen) < gs:                                                # fewer than 2 gs candidates only
                    chosen.append((-1e9, PAD, r0))
                for v, tok, row in chosen:
                    seqs.append(self.seqs[row] + [tok]); scores.append(v); src.append(row); padded.append(False); new_tok.append(tok)
                toks_here[(b, g)] = [tok for _, tok, _ in chosen]
            self.ev["two_groups_add"] += adders >= 2
        self.ev["staggered"] = self.ev["staggered"] or (any(self.done) and not all(self.done))
        self.new_tokens.append((forced, toks_here))
        self.seqs, self.scores, self.src, self.padded = seqs, np.asarray(scores, dtype=F), src, padded
        self.cur_len += 1
        return was_done

    def events(self):
        ev = dict(self.ev)
        ev["evict"] = sum(len(h.evicted) for h in self.hyps)
        return ev

    def finalize(self):
        out = []
        for b in range(self.B):
            if not self.done[b]:
                for j in range(self.nb):
                    self.hyps[b].add(self.seqs[b * self.nb + j], float(self.scores[b * self.nb + j]))
            out.append([(float(s), list(q)) for s, q in reversed(sorted(self.hyps[b].beams, key=lambda x: x[0]))])
        return out


def run_group_host(O, c, full=False):
    host = HostGroupBeams(O, c, full=full)
    while True:
        host.step(table_rows(c, host.seqs, host.cur_len))
        if all(host.done) or host.cur_len >= c["Lmax"]:
            return host


# what the cases are there for; every name is asserted on the host model for the cases that list it
GROUP_EVENTS = ("changed", "f2", "done_mid", "two_groups_add", "evict", "pen_hist", "forced_skip", "staggered")
# seeds found by a host-only search (as STEP_CASES were): the events in `expect` happen and every position keeps the best 2 gs + 1
# scores of every group pairwise distinct
GROUP_CASES = [
    gcase(2, 2, 1, 0.5, P=2.0, seed=27, eos_boost=0.05, expect=("changed", "two_groups_add", "evict", "forced_skip")),
    gcase(4, 2, 3, 1.0, lp=2.0, ngram=2, min_length=3, seed=11, start=2,
          expect=("changed", "f2", "two_groups_add", "evict", "forced_skip", "staggered")),
    gcase(6, 3, 1, 0.25, P=0.5, ngram=3, seed=1, eos_boost=0.05, expect=("changed", "f2", "done_mid", "two_groups_add", "evict", "pen_hist")),
    gcase(8, 4, 3, 0.5, lp=0.5, early=True, min_length=2, seed=13, start=2, eos_from=3, eos_boost=0.05,
          expect=("changed", "f2", "done_mid", "two_groups_add", "evict", "staggered")),
    gcase(8, 2, 1, 1.0, P=2.0, lp=2.0, seed=13, eos_boost=0.05, expect=("changed", "f2", "two_groups_add", "evict", "pen_hist", "forced_skip")),
    gcase(8, 8, 1, 0.25, ngram=2, seed=3, eos_from=3, eos_boost=0.05, expect=("changed", "f2", "done_mid", "two_groups_add", "evict")),
    gcase(4, 2, 1, 0.5, P=0.5, lp=2.0, ngram=3, Lmax=64, seed=4, eos_boost=0.05,          # 63 positions
          expect=("changed", "f2", "two_groups_add", "evict", "pen_hist", "forced_skip")),
]
LONG_CASE = gcase(2, 2, 1, 0.5, ngram=3, min_length=512, Lmax=512, seed=25, start=2, good=0.1,          # 511 positions (GPU lockstep)
                  expect=("changed", "forced_skip"))


@pytest.fixture(scope="module")
def O():
    from oracle import vacnic_oracle
    return vacnic_oracle


@pytest.mark.parametrize("c", GROUP_CASES, ids=gcase_id)
def test_group_cases_meet_their_events(O, c):
    host = run_group_host(O, c)
    ev = host.events()
    assert ev["distinct"], "tied group scores inside the best 2 gs + 1"
    for name in c["expect"]:
        assert ev[name], (name, ev)
    nbest = host.finalize()
    assert all(len(item) >= 1 for item in nbest)


def test_group_cases_cover_every_event_and_shape():
    assert set(GROUP_EVENTS) <= {e for c in GROUP_CASES for e in c["expect"]}
    assert {(c["nb"], c["G"]) for c in GROUP_CASES} >= {(2, 2), (4, 2), (6, 3), (8, 4), (8, 2), (8, 8)}
    assert {c["B"] for c in GROUP_CASES} == {1, 3} and {c["Lmax"] for c in GROUP_CASES} == {12, 64}
    assert {c["lam"] for c in GROUP_CASES} == {0.25, 0.5, 1.0} and {c["P"] for c in GROUP_CASES} == {1.0, 2.0, 0.5}


@pytest.mark.parametrize("c", [STEP_CASES[1], STEP_CASES[3], STEP_CASES[4], STEP_CASES[7]], ids=lambda c: "nb%d-B%d" % (c["nb"], c["B"]))
def test_one_group_is_ordinary_beam_search(O, c):
    """G = 1: captions, n-best lists and scores of HostBeams (itself pinned against the oracle's bookkeeping), position by position"""
    g = dict(c, G=1, lam=0.0, P=1.0, forced_eos=False)
    a, h = HostBeams(O, c), HostGroupBeams(O, g)
    while True:
        lp = table_rows(c, a.seqs, a.cur_len)
        a.step(lp); h.step(lp)
        assert a.seqs == h.seqs and a.src == h.src and a.done == h.done
        assert np.array_equal(a.scores.view(np.int32), h.scores.view(np.int32))
        assert [x.beams for x in a.hyps] == [x.beams for x in h.hyps]
        if all(a.done) or a.cur_len >= c["Lmax"]:
            break
    nbest = a.finalize()                                                         # (finalize adds the open beams: once per model)
    assert nbest == h.finalize() and nbest == run_host(O, c).finalize()


@pytest.mark.parametrize("c", GROUP_CASES, ids=gcase_id)
def test_row_lists_of_two_nb_suffice(O, c):
    """the merge over the per-row lists of K2 = 2 nb equals the merge over the whole [gs, V] score matrix of every group"""
    a, b = run_group_host(O, c), run_group_host(O, c, full=True)
    assert a.cur_len == b.cur_len and a.seqs == b.seqs and a.done == b.done
    assert np.array_equal(a.scores.view(np.int32), b.scores.view(np.int32))
    assert a.finalize() == b.finalize()
    assert a.events()["distinct"] and b.events()["distinct"]


@pytest.mark.parametrize("c", GROUP_CASES[:6], ids=gcase_id)
def test_a_large_penalty_keeps_the_groups_apart(O, c):
    """lambda = 1024 outweighs every score difference of the table: away from a forced position no group picks a token an earlier
    group of the same item picked in that position"""
    c = dict(c, lam=1024.0, ngram=0, min_length=0)
    host = run_group_host(O, c)
    seen = 0
    for forced, toks in host.new_tokens:
        if forced:
            continue
        for (b, g), mine in toks.items():
            earlier = {t for (b2, g2), ts in toks.items() if b2 == b and g2 < g for t in ts}
            assert not (set(mine) & earlier), (b, g, mine, earlier)
            seen += g > 0
    assert seen > 0


# ------------------------------------------------------------------------------------------ generate(): arguments, key, n-best layout
class _Cfg:
    eos_token_id, pad_token_id, decoder_start_token_id, vocab_size = 2, 1, 2, 100


class _NoModel:
    """a model that was never finalized: generate() reaches `model.arena is None` only after its argument checks"""
    config, V, arena = _Cfg(), 100, None


def test_generate_checks_the_group_arguments_before_the_model():
    from vacnic_amd.generate import generate
    for bad in (0, -1, 2.0, "2", None, True, np.float32(2)):
        with pytest.raises(ValueError, match="num_beam_groups"):
            generate(_NoModel(), num_beams=4, num_beam_groups=bad, diversity_penalty=0.0)
    with pytest.raises(ValueError, match="`num_beam_groups` has to be smaller or equal to `num_beams`"):
        generate(_NoModel(), num_beams=2, num_beam_groups=4, diversity_penalty=1.0)
    with pytest.raises(ValueError, match="`num_beams` should be divisible by `num_beam_groups`"):
        generate(_NoModel(), num_beams=6, num_beam_groups=4, diversity_penalty=1.0)
    with pytest.raises(ValueError, match="Diverse beam search cannot be used in sampling mode"):
        generate(_NoModel(), num_beams=2, num_beam_groups=2, diversity_penalty=1.0, do_sample=True)
    for bad in (-0.5, float("nan"), float("inf"), -float("inf"), "1.0", None, True, 1e39, 1 + 2j):
        with pytest.raises(ValueError, match="diversity_penalty"):
            generate(_NoModel(), num_beams=4, num_beam_groups=2, diversity_penalty=bad)
    for lam in (1.0, 0.25, np.float32(0.5), 1e-40):              # without groups a penalty would be ignored: an error here
        with pytest.raises(ValueError, match="diversity_penalty"):
            generate(_NoModel(), num_beams=4, diversity_penalty=lam)
    with pytest.raises(ValueError, match="staged encoding"):
        generate(_NoModel(), num_beams=4, num_beam_groups=2, diversity_penalty=1.0, encoded=object())
    # valid arguments pass the checks and reach the model (lambda == 0 with groups is legal, 1e-50 is 0 as float32)
    for kw in (dict(num_beams=6, num_beam_groups=3, diversity_penalty=1.0), dict(num_beams=4, num_beam_groups=2, diversity_penalty=0.0),
               dict(num_beams=4, num_beam_groups=4, diversity_penalty=np.float32(0.5)), dict(num_beams=4, num_beam_groups=1, diversity_penalty=0.0),
               dict(num_beams=4, diversity_penalty=1e-50), dict(num_beams=1), dict(num_beams=8, num_beam_groups=2, diversity_penalty=2,
                                                                                   repetition_penalty=1.3, bad_words_ids=[[5]])):
        with pytest.raises(RuntimeError, match="finalize"):
            generate(_NoModel(), **kw)


def test_one_group_keeps_the_session_key_of_before():
    from vacnic_amd import generate as G
    lp = (2.0, False)
    base = (5, 512, 50, 5, 3, 0, 2, None, lp)
    assert G._decode_session_key(*base, None, 1.0) == base
    assert G._decode_session_key(*base, None, 1.0, None) == base and G._decode_session_key(*base, None, 1.0, (1, 0.0)) == base
    assert len(G._decode_session_key(*base, None, 1.0, (1, 0.0))) == G._DECODE_KEY_LEN
    k = G._decode_session_key(6, 512, 50, 6, 3, 0, 2, None, lp, None, 1.0, (3, 1.3))
    assert k == (6, 512, 50, 6, 3, 0, 2, None, lp, 3, G._f32(1.3)) and len(k) > G._DECODE_KEY_LEN       # counts among the processor sessions
    assert G._decode_session_key(6, 512, 50, 6, 3, 0, 2, None, lp, ((7,),), G._f32(1.3), (3, 0.5)) == \
        (6, 512, 50, 6, 3, 0, 2, None, lp, ((7,),), G._f32(1.3), 3, 0.5)
    assert k != G._decode_session_key(6, 512, 50, 6, 3, 0, 2, None, lp, None, 1.0, (3, 1.0))            # lambda is part of the launches


def test_nbest_to_sequences_layout():
    from vacnic_amd.generate import nbest_to_sequences
    nbest = [[(-0.25, [2, 7, 8, 9]), (-0.5, [2, 7]), (-0.75, [2, 5, 6])],
             [(-0.125, [2, 4]), (-1.5, [2, 4, 4, 4, 4]), (-2.0, [2])]]
    ids, sc = nbest_to_sequences(nbest, 2, pad=1, eos=2, max_length=20)
    assert ids.dtype == torch.int64 and sc.dtype == torch.float32
    assert ids.tolist() == [[2, 7, 8, 9, 2, 1], [2, 7, 2, 1, 1, 1], [2, 4, 2, 1, 1, 1], [2, 4, 4, 4, 4, 2]]
    assert sc.tolist() == [-0.25, -0.5, -0.125, -1.5]
    ids, sc = nbest_to_sequences(nbest, 3, pad=1, eos=2, max_length=5)                 # the longest fills max_length: no eos behind it
    assert ids.tolist() == [[2, 7, 8, 9, 2], [2, 7, 2, 1, 1], [2, 5, 6, 2, 1], [2, 4, 2, 1, 1], [2, 4, 4, 4, 4], [2, 2, 1, 1, 1]]
    assert sc.tolist() == [-0.25, -0.5, -0.75, -0.125, -1.5, -2.0]
    ids, _ = nbest_to_sequences(nbest, 1, pad=0, eos=3, max_length=20)
    assert ids.tolist() == [[2, 7, 8, 9, 3], [2, 4, 3, 0, 0]]
    for bad in (0, 4, True, 1.0):
        with pytest.raises(ValueError):
            nbest_to_sequences(nbest, bad, 1, 2, 20)


# ------------------------------------------------------------------------------------------ C ABI
def test_group_entry_points_are_exported():
    from vacnic_amd import _lib
    assert "vacnic_group_beam_init" in _lib.EXPORTED and "vacnic_group_beam_step" in _lib.EXPORTED
    assert _lib.GroupBeamArgs.__name__ == "vacnic_group_beam_args"


def test_group_bad_arguments_return_a_status_without_a_launch():
    """every refusal is decided from the arguments alone (the pointers below are never read: 16 is no address)"""
    import ctypes as C
    from vacnic_amd import _lib

    def state(nb=4, Lmax=12, n_bad=0, bans=None):
        return _lib.BeamState(seq0=16, seq1=16, beam_scores=16, done=16, hyp_cnt=16, hyp_worst=16, hyp_score=16, hyp_len=16, hyp_seq=16,
                              next_ids=16, src_idx=16, bans=bans, B=1, nb=nb, Lmax=Lmax, V=40, eos=2, pad=1, no_repeat_ngram_size=0,
                              early_stopping=0, length_penalty=1.0, bad_words=16 if n_bad else None, bad_len=16 if n_bad else None, n_bad=n_bad)

    def args(G=2, lam=0.5, P=1.0, rule=0, forced=-1):
        return _lib.GroupBeamArgs(num_beam_groups=G, diversity_penalty=lam, repetition_penalty=P, penalty_rule=rule, forced_token=forced)

    def init(st, ga):
        _lib.call("vacnic_group_beam_init", C.byref(st), C.byref(ga), 2, None)

    def step(st, ga, K2=8, cur=1):
        _lib.call("vacnic_group_beam_step", C.byref(st), C.byref(ga), 16, 16, K2, cur, None)

    for fn in (init, step):
        for bad in (dict(G=0), dict(G=-2), dict(G=3), dict(G=8)):
            with pytest.raises(ValueError, match="num_beam_groups"):
                fn(state(), args(**bad))
        for lam in (-0.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="diversity penalty"):
                fn(state(), args(lam=lam))
        for P in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="repetition penalty"):
                fn(state(), args(P=P, rule=2))
        for rule in (1, 3, -1):
            with pytest.raises(ValueError, match="penalty_rule"):
                fn(state(), args(rule=rule))
        with pytest.raises(ValueError, match="null operand"):
            fn(state(n_bad=3, bans=None), args())
    with pytest.raises(ValueError, match="null operand"):
        _lib.call("vacnic_group_beam_step", C.byref(state()), None, 16, 16, 8, 1, None)
    with pytest.raises(ValueError, match="null operand"):
        _lib.call("vacnic_group_beam_init", C.byref(state()), None, 2, None)
    # the shapes vacnic_beam_step refuses are refused with the same status: unsupported, never an abort
    for nb, K2 in ((32, 2), (16, 9), (16, 32), (2, 65)):
        with pytest.raises(_lib.VacnicError, match="nb <= 16"):
            step(state(nb=nb), args(G=2), K2=K2)
    for cur, L in ((0, 12), (12, 12), (1, 513)):
        with pytest.raises(ValueError, match="outside"):
            step(state(Lmax=L), args(), cur=cur)
