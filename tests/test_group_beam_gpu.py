"""Group (diverse) beam search on the device: vacnic_group_beam_init / vacnic_group_beam_step in lockstep with the host model of
tests/test_group_beam.py (bit-equal state after every position), the G == 1 identity with vacnic_beam_init / vacnic_beam_step, and
generate(num_beam_groups=, diversity_penalty=) against transformers 4.18's group loop driven on the host in float64 over the model's
own per-position logits.  No margin is taken from the code under test: the float64 loop's decisions must be decidable by more than
margin_of of tests/test_decode_gpu.py (8x the deviation of fp32 torch from float64 on the same rows; the margins of the positions
behind a decision are added to its own, since it compares running sums), asserted on the reference alone."""
import numpy as np
import pytest
import torch

import test_decode_gpu as D
from test_decode_gpu import EOS, PAD, STEP_CASES, VS, bits, row_lists, table_rows
from test_decode_processors import host_bad_words
from test_group_beam import GROUP_CASES, LONG_CASE, HostGroupBeams, gcase_id

gpu = pytest.mark.gpu
NEG = -float("inf")


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


STATE = ("seq", "beam_scores", "done", "hyp_cnt", "hyp_worst", "hyp_score", "hyp_len", "hyp_seq", "next_ids", "src_idx")


def fill(st):
    for name in STATE:
        if name != "hyp_worst":
            getattr(st, name).fill_(77)                                          # init owns all of it


def compare_group_state(st, host, prev_seqs, c, cur):
    """device state after vacnic_group_beam_step(cur) against HostGroupBeams after the same position, bit for bit"""
    B, nb = c["B"], c["nb"]
    torch.cuda.synchronize()
    seq = st.seq.cpu().numpy()
    live, prev = seq[cur & 1], seq[(cur - 1) & 1]
    for r, s in enumerate(host.seqs):
        assert live[r, :cur + 1].tolist() == s and bool((live[r, cur + 1:] == PAD).all()), (cur, r, live[r, :cur + 2].tolist(), s)
        assert prev[r, :cur].tolist() == prev_seqs[r], (cur, r, "the input histories changed")
    assert np.array_equal(bits(st.beam_scores.cpu().numpy()), bits(host.scores)), (cur, st.beam_scores.cpu().tolist(), host.scores.tolist())
    assert st.next_ids.cpu().tolist() == [s[-1] for s in host.seqs], cur
    assert st.src_idx.cpu().tolist() == host.src, (cur, st.src_idx.cpu().tolist(), host.src)
    assert all(host.src[r] // host.gs == r // host.gs for r in range(B * nb))     # a row continues a row of its own group
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
        for r, want in enumerate(host.bans()):                                   # the rows of a padded group ban nothing
            assert sorted(bans[r, :len(want)].tolist()) == sorted(want) and bool((bans[r, len(want):] == -1).all()), (cur, r, bans[r, :len(want) + 2].tolist(), want)


def same_state(a, g, where):
    """every state tensor equal (the slots neither init nor step has written still hold the 77 of fill()); the order inside a ban list
    is unspecified, so those compare as sorted rows"""
    for name in STATE:
        assert torch.equal(getattr(a, name), getattr(g, name)), (where, name)
    if a.bans is not None:
        assert torch.equal(a.bans.sort(dim=1).values, g.bans.sort(dim=1).values), (where, "bans")


def group_lockstep(K, c):
    from oracle import vacnic_oracle as O
    B, nb, L = c["B"], c["nb"], c["Lmax"]
    R, K2 = B * nb, min(2 * nb, VS)
    rule = None if c["P"] == 1 else "scores"
    st = K.beam_alloc(B, nb, L, VS, EOS, PAD, no_repeat_ngram_size=c["ngram"], early_stopping=c["early"], length_penalty=c["lp"],
                      groups=(c["G"], c["lam"]))
    fill(st)
    K.group_beam_init(st, c["start"])
    host = HostGroupBeams(O, c)
    torch.cuda.synchronize()
    assert st.seq[0].cpu().tolist() == [[c["start"]] + [PAD] * (L - 1)] * R
    assert np.array_equal(bits(st.beam_scores.cpu().numpy()), bits(host.scores)) and st.next_ids.cpu().tolist() == [c["start"]] * R
    assert st.beam_scores.cpu().tolist() == [0.0 if r % host.gs == 0 else -1e9 for r in range(R)]
    assert st.done.cpu().tolist() == [0] * B and st.hyp_cnt.cpu().tolist() == [0] * B and st.hyp_worst.cpu().tolist() == [1e9] * B
    assert st.bans is None or bool((st.bans == -1).all())
    for cur in range(1, L):
        lp = table_rows(c, host.seqs, cur)
        forced = host.forced()
        # what the top-k call of the position hands over: the penalty on the scores and the forced token applied on the host, the
        # device's own bans and beam scores (a forced position overrides bans and MinLength)
        tv, ti = row_lists(host.penalised(lp), None if (st.bans is None or forced >= 0) else st.bans.cpu(), st.beam_scores.cpu().numpy(),
                           cur < c["min_length"] and forced < 0, K2)
        prev = host.seqs
        K.group_beam_step(st, tv.cuda(), ti.cuda(), cur, forced_token=forced, repetition_penalty=c["P"], penalty_rule=rule)
        host.step(lp)
        compare_group_state(st, host, prev, c, cur)
        if all(host.done):
            break
    ev = host.events()
    assert ev["distinct"] and all(ev[name] for name in c["expect"]), ev
    assert all(host.done) or host.cur_len == L                                  # no position skipped
    return host


@gpu
@pytest.mark.parametrize("c", GROUP_CASES, ids=gcase_id)
def test_group_beam_step_lockstep(K, c):
    group_lockstep(K, c)


@gpu
def test_group_beam_step_lockstep_511_positions(K):
    host = group_lockstep(K, LONG_CASE)
    assert host.cur_len == 512 and host.events()["changed"]


@gpu
@pytest.mark.parametrize("c", [STEP_CASES[3], STEP_CASES[4]], ids=D.case_id)
def test_one_group_leaves_the_state_of_beam_step(K, c):
    """G == 1 through the new entry points: every state tensor equals vacnic_beam_init / vacnic_beam_step's after every position"""
    from oracle import vacnic_oracle as O
    B, nb, L = c["B"], c["nb"], c["Lmax"]
    K2 = min(2 * nb, VS)
    mk = lambda **kw: K.beam_alloc(B, nb, L, VS, EOS, PAD, no_repeat_ngram_size=c["ngram"], early_stopping=c["early"], length_penalty=c["lp"], **kw)
    a, g = mk(), mk(groups=(1, 0.0))
    fill(a); fill(g)
    a.hyp_worst.fill_(5.0); g.hyp_worst.fill_(5.0)
    K.beam_init(a, c["start"]); K.group_beam_init(g, c["start"])
    host = D.HostBeams(O, c)
    for cur in range(1, L):
        same_state(a, g, cur)
        lp = table_rows(c, host.seqs, cur)
        tv, ti = row_lists(lp, None if a.bans is None else a.bans.cpu(), a.beam_scores.cpu().numpy(), cur < c["min_length"], K2)
        K.beam_step(a, tv.cuda(), ti.cuda(), cur)
        K.group_beam_step(g, tv.cuda(), ti.cuda(), cur)
        host.step(lp)
        if all(host.done):
            break
    same_state(a, g, "end")
    assert all(host.events()[name] for name in c["expect"])


@gpu
def test_group_beam_step_sixteen_beams_four_groups(K):
    """nb = 16, G = 4 with K2 = 8 (nb * K2 <= 128), the shape of test_beam_step_sixteen_beams: 32 candidates per group, the best
    min(2 gs, K2) = 8 kept.  Hand-written distinct scores against the rules restated here."""
    from oracle import vacnic_oracle as O
    B, nb, G, V, L, K2, start, lam = 2, 16, 4, 50, 16, 8, 7, 0.5
    gs, n = nb // G, B * nb * K2
    tv = (-(1 + (np.arange(n) * 37) % 256) / 16.0).astype(np.float32).reshape(B, nb, K2)
    assert len(set(tv.reshape(-1).tolist())) == n
    tv = -np.sort(-tv, axis=2)                                                      # every row's list best first
    ti = (3 + (np.arange(n) * 11) % 8).astype(np.int32).reshape(B, nb, K2)          # 8 tokens: the groups collide
    ti[0, 0, 0] = EOS; ti[0, 5, 0] = EOS                                            # item 0: EOS at the head of rows of groups 0 and 1
    st = K.beam_alloc(B, nb, L, V, EOS, PAD, no_repeat_ngram_size=2, length_penalty=1.0, groups=(G, lam))
    K.group_beam_init(st, start)
    K.group_beam_step(st, torch.from_numpy(tv).view(B * nb, K2).cuda(), torch.from_numpy(ti).view(B * nb, K2).cuda(), 1)
    torch.cuda.synchronize()
    seq, bans = st.seq[1].cpu().numpy(), st.bans.cpu().numpy()
    penalised = 0
    for b in range(B):
        new_tok, hyps, want = [], [], []
        for g in range(G):
            cand = []
            for i in range(gs):
                for k in range(K2):
                    tok, v = int(ti[b, g * gs + i, k]), tv[b, g * gs + i, k]
                    f = new_tok.count(tok)
                    penalised += f > 0
                    cand.append((float(np.float32(v - np.float32(lam * f)) if f else v), i * V + tok, g * gs + i, tok))
            cand = sorted(cand, key=lambda x: (-x[0], x[1]))[:min(2 * gs, K2)]
            chosen = []
            for rank, (v, _, j, tok) in enumerate(cand):
                if tok == EOS:
                    if rank < gs:
                        hyps.append(v)
                elif len(chosen) < gs:
                    chosen.append((v, tok, b * nb + j))
            assert len(chosen) == gs
            want += chosen
            new_tok += [t for _, t, _ in chosen]
        rows = slice(b * nb, (b + 1) * nb)
        assert st.next_ids[rows].tolist() == [t for _, t, _ in want], (b, st.next_ids[rows].tolist(), want)
        assert st.src_idx[rows].tolist() == [r for _, _, r in want]
        assert st.beam_scores[rows].tolist() == [v for v, _, _ in want]
        assert int(st.hyp_cnt[b]) == len(hyps) and st.hyp_score[b, :len(hyps)].tolist() == hyps
        assert (len(hyps) > 0) == (b == 0)                                      # only item 0 holds EOS: at rank 0 of its group 0
        for j, (_, t, _) in enumerate(want):
            r = b * nb + j
            assert seq[r].tolist() == [start, t] + [PAD] * (L - 2), r
            ban = O.banned_ngram_tokens([start, t], 2)
            assert bans[r, :len(ban)].tolist() == ban and bool((bans[r, len(ban):] == -1).all()), (r, bans[r, :3].tolist(), ban)
    assert penalised > 0


@gpu
def test_group_beam_refusals_on_the_device(K):
    from vacnic_amd import _lib

    def step(nb, G, K2, lam=0.5, **kw):
        st = K.beam_alloc(1, nb, 12, VS, EOS, PAD)
        K.group_beam_step(st, torch.zeros(nb, K2, device="cuda"), torch.zeros(nb, K2, device="cuda", dtype=torch.int32), 1, groups=(G, lam), **kw)
    for nb, G in ((4, 3), (4, 8), (4, 0)):
        with pytest.raises(ValueError, match="num_beam_groups"):
            step(nb, G, 8)
    with pytest.raises(ValueError, match="diversity penalty"):
        step(4, 2, 8, lam=-1.0)
    with pytest.raises(ValueError, match="repetition penalty"):
        step(4, 2, 8, repetition_penalty=0.0, penalty_rule="scores")
    with pytest.raises(ValueError, match="never on the logits"):
        step(4, 2, 8, repetition_penalty=1.3, penalty_rule="logits")
    for nb, G, K2 in ((16, 4, 32), (16, 4, 9), (2, 2, 65)):
        with pytest.raises(_lib.VacnicError, match="nb <= 16"):
            step(nb, G, K2)
    with pytest.raises(ValueError, match="num_beam_groups"):
        K.beam_alloc(1, 4, 12, VS, EOS, PAD, groups=(3, 1.0))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ generate()
def generation_inputs(K, B=1, seed=9):
    """the tiny generation model of tests/test_decode_gpu.py (shared with tests/test_decode_processors_gpu.py) and B captions' inputs"""
    from test_decode_processors_gpu import generation_inputs as one
    model, kw = one(K)
    kw = dict(kw, max_length=7, min_length=3)
    if B > 1 or seed != 9:
        from vacnic_amd import synthetic
        batch = synthetic.make_batch(model.config, B, S=24, T=8, F=2, seed=seed, image_size=32)
        dev = {k: v.cuda() for k, v in batch.items()}
        mask, _ = K.prep_ids(dev["article_ids"], 1)
        nmask, _ = K.prep_ids(dev["names_art_ids"], 1)
        kw = dict(kw, input_ids=dev["article_ids"], attention_mask=mask, image_features=synthetic._normal("img_cls", (B, 768), 1.0, 3).cuda(),
                  face_features=dev["face_emb"], face_mask=K.face_mask(dev["face_emb"]), name_ids=dev["names_art_ids"], name_mask=nmask)
    return model, kw


def group_reference(K, model, kw, nb, G, lam, penalty=1.0, words=(), ngram=0):
    """transformers 4.18 group_beam_search + BeamSearchScorer (one BeamHypotheses(num_beams=nb) and one done flag per item) for one
    caption, on the host in float64 over the model's own fp32 logits: every row is decoded along its own history by a cached decoder
    of its own (no reorder).  The processors run in HF's order: HammingDiversity, RepetitionPenalty, NoRepeatNGram, NoBadWords,
    MinLength, ForcedEOS; then + beam score.  Returns (best ids, n-best [(score, ids)], the group that gave each hypothesis,
    [(gap, margin, where)] of every decision: the adjacent gaps inside the best 2 gs + 1 scores of every group merge, every add to
    a full list, and best against second best at the end).  The ORDER of the n-best list behind its head is not among the decisions
    (hypotheses of nearly equal score may swap), so callers compare the head exactly and the rest as a set."""
    from oracle import vacnic_oracle as O
    from vacnic_amd import generate as GEN
    cfg = model.config
    eos, pad, start = cfg.eos_token_id, cfg.pad_token_id, cfg.decoder_start_token_id
    Lmax, min_length, V, gs = kw["max_length"], kw.get("min_length", 0), model.V, nb // G
    mask_u8 = kw["attention_mask"].to(torch.uint8)
    enc_h = GEN._run_encoder(model, False, kw["add_ner_ffn"], kw["input_ids"], mask_u8, kw["image_features"], kw["name_ids"], kw["name_mask"],
                             kw["face_features"], kw["face_mask"])
    dec = GEN.CachedDecoder(model, nb, enc_h.shape[1], Lmax, reorders=False)
    dec.begin(enc_h, mask_u8, nb)
    F64 = torch.float64
    P64, P32 = float(np.float32(penalty)), torch.tensor(penalty, dtype=torch.float32)
    seqs = [[start] for _ in range(nb)]
    bs = [0.0 if r % gs == 0 else -1e9 for r in range(nb)]
    hyps, done, owner, decisions = O._BeamHyps(nb, kw["length_penalty"], False), False, {}, []
    lp_ = kw["length_penalty"]

    def add(hyp, v, margin, where):
        # a full list takes the hypothesis iff its score beats the worst, and then drops its lowest: which entry that is, is a decision
        # too (the gap between the two lowest of list + newcomer, brought to units of summed log-probabilities by the shorter length)
        if len(hyps.beams) == nb:
            low = sorted([(sc, len(q)) for sc, q in hyps.beams] + [(v / len(hyp) ** lp_, len(hyp))])[:2]
            decisions.append(((low[1][0] - low[0][0]) * min(low[0][1], low[1][1]) ** lp_, margin, where))
        hyps.add(hyp, v)

    cur, carried = 1, 0.0                        # carried: the margins of the positions behind, summed
    while True:
        for t in range(cur):
            logits = dec.step(torch.tensor([[s[t]] for s in seqs], device="cuda"), t)
        z = logits[:, :V].float().cpu()
        s64, s32 = torch.log_softmax(z.to(F64), 1), torch.log_softmax(z, 1)
        forced = eos if cur == Lmax - 1 else -1
        new_tok, new_seqs, new_bs = [], [], []
        worst_here = 0.0
        for g in range(G):
            rows = list(range(g * gs, (g + 1) * gs))
            if done:
                new_seqs += [seqs[rows[0]] + [pad]] * gs; new_bs += [0.0] * gs
                continue
            a64, a32 = s64[rows].clone(), s32[rows].clone()
            if g > 0 and new_tok:
                f = torch.bincount(torch.tensor(new_tok), minlength=V)
                a64 -= float(np.float32(lam)) * f.to(F64); a32 -= torch.tensor(lam, dtype=torch.float32) * f.float()
            for i, r in enumerate(rows):
                if penalty != 1.0:
                    h = sorted(set(seqs[r]))
                    a64[i, h] = torch.where(a64[i, h] < 0, a64[i, h] * P64, a64[i, h] / P64)
                    a32[i, h] = torch.where(a32[i, h] < 0, a32[i, h] * P32, a32[i, h] / P32)
                for tok in O.banned_ngram_tokens(seqs[r], ngram) + host_bad_words(seqs[r], words, eos):
                    a64[i, tok] = NEG; a32[i, tok] = NEG
            if cur < min_length:
                a64[:, eos] = NEG; a32[:, eos] = NEG
            if forced >= 0:
                a64[:] = NEG; a32[:] = NEG
                a64[:, forced] = 0.0; a32[:, forced] = 0.0
            b64 = torch.tensor([bs[r] for r in rows], dtype=F64)
            a64 += b64[:, None]; a32 += b64.float()[:, None]
            # the yardstick: fp32 torch against float64 on the rows that can reach the merge (a beam at -1e9 cannot: its fp32 sums
            # are rounded to multiples of 64, and every score of a live row lies far above them)
            live = [i for i, r in enumerate(rows) if bs[r] > -1e8]
            assert live and all(bs[rows[i]] < -1e8 + 1 for i in range(gs) if i not in live)
            # The scores compared are running sums: the beam score carried into this position is a sum of cur - 1 fp32 scores, each
            # off by up to its own position's margin, so a decision here has to clear those margins plus this position's.
            here, _ = D.margin_of(a64[live], a32[live].to(F64), f"group {g} position {cur}")
            worst_here = max(worst_here, here)
            margin = carried + here
            top, order = torch.sort(a64.reshape(-1), descending=True, stable=True)
            top, order = top[:2 * gs + 1], order[:2 * gs + 1]
            for k in range(2 * gs):
                if bool(torch.isfinite(top[k + 1])) and float(top[k + 1]) > -1e8:
                    decisions.append((float(top[k] - top[k + 1]), margin, (cur, g, k)))
            chosen = []
            for rank in range(2 * gs):
                i, tok, v = int(order[rank]) // V, int(order[rank]) % V, float(top[rank])
                if tok == eos:
                    if rank >= gs:
                        continue
                    add(seqs[rows[i]], v, margin, (cur, g, "add"))
                    owner.setdefault(tuple(seqs[rows[i]]), g)
                else:
                    chosen.append((v, tok, rows[i]))
                if len(chosen) == gs:
                    break
            done = done or hyps.is_done(float(top[0]), cur)
            for v, tok, r in chosen:
                new_seqs.append(seqs[r] + [tok]); new_bs.append(v); new_tok.append(tok)
        seqs, bs = new_seqs, new_bs
        carried += worst_here
        cur += 1
        if done or cur >= Lmax:
            break
    if not done:
        for r in range(nb):
            add(seqs[r], bs[r], margin, (cur, r // gs, "finalize"))
            owner.setdefault(tuple(seqs[r]), r // gs)
    ranked = [(float(s), list(q)) for s, q in reversed(sorted(hyps.beams, key=lambda x: x[0]))]
    if len(ranked) > 1 and ranked[0][1] != ranked[1][1]:                         # which hypothesis is the best one: the last decision
        n0 = min(len(ranked[0][1]), len(ranked[1][1])) ** lp_
        decisions.append(((ranked[0][0] - ranked[1][0]) * n0, margin, (cur, -1, "best")))
    return ranked[0][1], ranked, owner, decisions


def assert_decidable(decisions, what):
    assert decisions
    worst = min(decisions, key=lambda d: d[0] / d[1])
    print(f"GROUPCHK {what}: {len(decisions)} decisions, narrowest gap={worst[0]:.3e} margin={worst[1]:.3e} at (position, group, rank) {worst[2]}")
    assert worst[0] > worst[1], (what, worst)


def ids_of(res, pad, eos):
    """a generate() row without its padding and closing eos: what the n-best lists hold"""
    row = res.tolist()
    while row and row[-1] == pad:
        row.pop()
    return row


@gpu
@pytest.mark.parametrize("nb,G,fused", [(4, 2, True), (6, 3, True), (16, 4, False)])
def test_generate_groups_match_the_float64_group_loop(K, nb, G, fused):
    """the test that fails without the feature: the keywords used to vanish into **unused and ordinary beams came back.
    (Inputs: the synthetic model is sharp and repeats its first token, so ordinary beams differ in their first token alone and
    the groups would pick the same captions; with no_repeat_ngram_size=2 the beams of ordinary search share prefixes.  Seed and
    n-gram size were chosen on the float64 reference alone: its diverse n-best differs from its ordinary one, all decisions decidable.)"""
    model, kw = generation_inputs(K, seed=17)
    kw = dict(kw, no_repeat_ngram_size=2)
    model.__dict__.pop("_decode_sessions", None)
    plain, plain_nbest = model.generate(num_beams=nb, return_nbest=True, **kw)
    gkw = dict(num_beams=nb, num_beam_groups=G, diversity_penalty=2.0, return_nbest=True, **kw)
    eager, eager_nbest = model.generate(use_graphs=False, **gkw)
    ses = [s for k, s in model._decode_sessions.items() if len(k) > 9]
    assert len(ses) == 1 and ses[0].fused_tail is fused and ses[0].groups == (G, 2.0)
    assert (ses[0].beam is not None) == (nb <= 8)                                # 16 beams: 2 nb candidates per row, host bookkeeping
    runs = [model.generate(**gkw) for _ in range(3)]                              # eager, capturing, replaying
    runs += [model.generate(device_beams=False, **gkw) for _ in range(3)]
    runs.append(model.generate(device_beams=False, use_graphs=False, **gkw))
    for res, nbest in runs:
        assert torch.equal(res, eager), (res.tolist(), eager.tolist())
        assert nbest == eager_nbest                                              # ids and scores: device and host round alike
    want, ranked, owner, decisions = group_reference(K, model, kw, nb, G, 2.0, ngram=2)
    assert_decidable(decisions, f"nb={nb} G={G}")
    cfg = model.config
    got = eager[0].tolist()
    assert got[:len(want)] == want and set(got[len(want):]) <= {cfg.eos_token_id, cfg.pad_token_id}, (got, want)
    assert eager_nbest[0][0][1] == ranked[0][1] and sorted(q for _, q in eager_nbest[0]) == sorted(q for _, q in ranked)
    # diversity: the n-best list is not the one of ordinary beams
    assert sorted(q for _, q in eager_nbest[0]) != sorted(q for _, q in plain_nbest[0])
    assert torch.equal(model.generate(num_beams=nb, **kw), plain)                # the groups did not leak into the old session


@gpu
def test_generate_groups_differ_from_one_another(K):
    """with lambda = 2.0 the best captions of the groups (which group gave which hypothesis: from the float64 loop) differ from one
    another in at least one of the three shapes, and generate() hands those captions out"""
    model, kw = generation_inputs(K, seed=17)
    kw = dict(kw, no_repeat_ngram_size=2)
    differ = {}
    for nb, G in ((4, 2), (6, 3), (16, 4)):
        _, ranked, owner, decisions = group_reference(K, model, kw, nb, G, 2.0, ngram=2)
        assert_decidable(decisions, f"nb={nb} G={G}")
        best = {}
        for _, q in ranked:
            best.setdefault(owner[tuple(q)], q)
        differ[(nb, G)] = len(best) > 1 and len({tuple(q) for q in best.values()}) == len(best)
        _, nbest = model.generate(num_beams=nb, num_beam_groups=G, diversity_penalty=2.0, return_nbest=True, **kw)
        assert all(q in [h for _, h in nbest[0]] for q in best.values()), (nb, G)
    assert any(differ.values()), differ


@gpu
def test_generate_alternating_penalties_and_processors(K):
    model, kw = generation_inputs(K)
    model.__dict__.pop("_decode_sessions", None)
    okw = dict(num_beams=4, num_beam_groups=2, return_nbest=True, **kw)
    ref = {lam: model.generate(use_graphs=False, diversity_penalty=lam, **okw) for lam in (2.0, 0.5, 0.0)}
    for rnd in range(3):                                                          # never a stale graph: lambda is part of the session key
        for lam in (2.0, 0.5):
            res, nbest = model.generate(diversity_penalty=lam, **okw)
            assert torch.equal(res, ref[lam][0]) and nbest == ref[lam][1], (rnd, lam)
    want, ranked, _, decisions = group_reference(K, model, kw, 4, 2, 0.5)
    assert_decidable(decisions, "lambda=0.5")
    assert ref[0.5][1][0][0][1] == ranked[0][1] and sorted(q for _, q in ref[0.5][1][0]) == sorted(q for _, q in ranked)
    # lambda == 0 is legal: the groups run without the Hamming term, so both groups of an item follow the same beams (device and host alike)
    res, nbest = model.generate(device_beams=False, diversity_penalty=0.0, **okw)
    assert torch.equal(res, ref[0.0][0]) and nbest == ref[0.0][1]
    half = len(ref[0.0][1][0]) // 2
    assert sorted(q for _, q in ref[0.0][1][0])[0::2] == sorted(q for _, q in ref[0.0][1][0])[1::2] and half >= 1
    # with RepetitionPenalty, NoRepeatNGram and one bad word: the word is a token the plain group search emits
    words = [[ref[2.0][0][0].tolist()[2]]]
    pkw = dict(diversity_penalty=2.0, repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=words, **okw)
    eager = model.generate(use_graphs=False, **pkw)
    for run in [model.generate(**pkw) for _ in range(3)] + [model.generate(device_beams=False, **pkw) for _ in range(2)]:
        assert torch.equal(run[0], eager[0]) and run[1] == eager[1]
    want, ranked, _, decisions = group_reference(K, model, kw, 4, 2, 2.0, penalty=1.3, words=words, ngram=2)
    assert_decidable(decisions, "with processors")
    assert eager[1][0][0][1] == ranked[0][1] and sorted(q for _, q in eager[1][0]) == sorted(q for _, q in ranked)
    assert all(words[0][0] not in q[1:] for _, q in eager[1][0])


@gpu
def test_generate_groups_two_captions(K):
    model, kw = generation_inputs(K, B=2)
    model.__dict__.pop("_decode_sessions", None)
    gkw = dict(num_beams=4, num_beam_groups=2, diversity_penalty=2.0, return_nbest=True, **kw)
    res, nbest = model.generate(**gkw)
    host, host_nbest = model.generate(device_beams=False, **gkw)
    assert res.shape[0] == 2 and torch.equal(res, host) and nbest == host_nbest
    from vacnic_amd.generate import nbest_to_sequences
    cfg = model.config
    ids, sc = nbest_to_sequences(nbest, 2, cfg.pad_token_id, cfg.eos_token_id, kw["max_length"])
    assert ids.shape[0] == 4 and torch.equal(ids[0::2, :res.shape[1]].cuda(), res[:, :ids.shape[1]]) and sc.shape == (4,)
