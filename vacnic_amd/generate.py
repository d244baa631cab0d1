"""Caption generation on gfx950 kernels: encoder once, then a KV-cached single-token decoder loop with beam
search — the `model.generate(input_ids, attention_mask, num_beams=5, max_length=50, image_features=..., face_features=...,
name_ids=..., add_ner_ffn=True[, length_penalty=2.0])` call of TRAIN:513-520 / DDPINF:758-842.

What runs where
  * device (hand-written kernels): embed+pos+LN of the new token, fused k|v|q projection, KV-cache append, fused
    attention over the cache (self) and over the per-layer cross K/V computed once from the encoder states, FFN,
    LM head, log-softmax + logits processors + top-2k (`beam_topk`), cache reorder for all layers in one launch
    (`gather_rows`; _reorder_cache MFULL:2066-2074 — cross K/V are never reordered, as in the reference).
  * beam bookkeeping (transformers 4.18 BeamSearchScorer.process: n-best lists, EOS handling, done flags) and the
    NoRepeatNGram ban lists: `vacnic_beam_step`, one wave per batch item, in the same per-position graph; the
    host reads the state ONCE after the last position (and polls the done flags every 8th position to stop early).
    `device_beams=False` keeps the host-side scorer (one device->host copy of the [B*beams, 2*beams] candidates per token).
  * sampling (`do_sample=True`, one beam): the same cached decoder, then the fp32 [rows, V] logits and `vacnic_sample_step` —
    processors, temperature, top-k, top-p, one Philox draw, histories / done flags / log-probs — per position (SampleSession).
  * `repetition_penalty` / `bad_words_ids` (transformers 4.18 RepetitionPenalty / NoBadWords): the bad-word bans of the next position
    are appended to the ban lists by `vacnic_beam_init` / `vacnic_beam_step` (host loop: `_bad_word_bans`) and matched in place by
    `vacnic_sample_step`; the penalty is applied by the top-k kernels from the token histories (on the logits for one beam and for
    sampling, on the log-softmax scores for more beams).  Off (1.0 / None) the calls are the ones of before.
  * group (diverse) beam search (`num_beam_groups` > 1, `diversity_penalty`; 4.18's group_beam_search + HammingDiversity): the same
    per-position tail over all rows, then `vacnic_group_beam_step` in place of `vacnic_beam_step` — the groups of an item in order
    inside one launch (host loop: the same rules in generate()).  One group (the default): the calls are the ones of before.

The cache is preallocated ([layers, B*beams, max_length, 2d] bf16, k|v interleaved per row) instead of the reference's
per-step torch.cat (MFULL:489-492).
"""
import numbers
import os
import struct

import torch

from . import _lib, kernels as K

BF16 = torch.bfloat16


class GraphedCall:
    """fn(*tensors) -> tensor(s), captured as a hipGraph per input signature (shapes + dtypes) and replayed: at batch 1 the
    encoder / ViT of a caption are ~600 launches of a few microseconds of work each, i.e. bound by the Python launch path
    (5.5 + 2.5 ms per caption eagerly).  First sighting of a signature runs eagerly (warms kernels and lazy buffers), the second
    captures, later ones copy the inputs into the graph's static buffers and replay.  The outputs live in the graph's pool and
    are overwritten by the next replay — callers consume (or clone) them before calling again.  A body that stream capture
    rejects (host synchronisation inside) stays eager for that signature, with a warning; any other error is raised."""

    def __init__(self, fn, max_entries=8):
        self.fn, self.cache, self.max_entries = fn, {}, max_entries

    def __call__(self, *args):
        from . import streams
        # the captured launches depend on the stream schedule in force; weights are read in place from the arenas (same
        # addresses after an optimizer step or a reload), so they are not part of the key
        key = (streams.enabled(),) + tuple((tuple(a.shape), a.dtype) if a is not None else None for a in args)
        ent = self.cache.get(key)
        if ent is None:
            if len(self.cache) >= self.max_entries:
                self.cache.pop(next(iter(self.cache)))
            self.cache[key] = "seen"
            return self.fn(*args)
        if ent == "eager":
            return self.fn(*args)
        if ent == "seen":
            static = [a.clone() if a is not None else None for a in args]
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            try:
                # (this graph may replay beside other graphs — CaptionPipeline — so its split-K fix-up buffers are its own)
                with K.capture_scope(("graphed-call", id(g))), torch.cuda.graph(g):
                    out = self.fn(*static)
            except _lib.VacnicError:
                raise                                     # a kernel / argument error is a bug, not a capture limitation
            except RuntimeError as e:
                # only what stream capture itself rejects (a host synchronisation inside the body, an unsupported call while
                # capturing) makes the signature eager; anything else is passed on
                torch.cuda.synchronize()
                msg = str(e).lower()
                if not any(w in msg for w in ("captur", "hipgraph", "cudagraph", "graph")):
                    raise
                import warnings
                warnings.warn(f"GraphedCall: {getattr(self.fn, '__name__', 'fn')} stays eager for signature {key}: {e}")
                self.cache[key] = "eager"
                return self.fn(*args)
            ent = self.cache[key] = (g, static, out)
        g, static, out = ent
        for st, a in zip(static, args):
            if st is not None:
                st.copy_(a, non_blocking=True)
        g.replay()
        return out


class _BeamHyps:
    """n-best list of finished hypotheses, scored sum_logprobs / len**length_penalty (len counts the decoder start token,
    not the closing EOS) — transformers==4.18 BeamHypotheses."""

    def __init__(self, n, length_penalty, early_stopping):
        self.n, self.lp, self.early = n, length_penalty, early_stopping
        self.beams, self.worst = [], 1e9

    def add(self, hyp, sum_logprobs):
        score = sum_logprobs / (len(hyp) ** self.lp)
        if len(self.beams) < self.n or score > self.worst:
            self.beams.append((score, list(hyp)))
            if len(self.beams) > self.n:
                srt = sorted((s, i) for i, (s, _) in enumerate(self.beams))
                del self.beams[srt[0][1]]
                self.worst = srt[1][0]
            else:
                self.worst = min(score, self.worst)

    def is_done(self, best_sum_logprobs, cur_len):
        if len(self.beams) < self.n:
            return False
        if self.early:
            return True
        return self.worst >= best_sum_logprobs / cur_len ** self.lp


def _banned(seq, n):
    if n <= 0 or len(seq) + 1 < n:
        return []
    prefix = tuple(seq[len(seq) - (n - 1):]) if n > 1 else ()
    return [seq[i + n - 1] for i in range(len(seq) - n + 1) if tuple(seq[i:i + n - 1]) == prefix]


def _bad_word_bans(seq, words):
    """NoBadWordsLogitsProcessor of transformers 4.18 for one history: the last token of every word whose other tokens end the
    history (a one-token word always; a prefix as long as the whole history matches)."""
    out = []
    for w in words:
        m = len(w)
        if m - 1 <= len(seq) and (m == 1 or tuple(seq[len(seq) - (m - 1):]) == tuple(w[:-1])):
            out.append(w[-1])
    return out


def _f32(x):
    """x rounded to float32, as the kernels receive it (inf where it overflows)"""
    try:
        return struct.unpack("<f", struct.pack("<f", float(x)))[0]
    except OverflowError:
        return float("inf") if x > 0 else float("-inf")


def _check_processor_args(model, repetition_penalty, bad_words_ids):
    """the checks of RepetitionPenaltyLogitsProcessor / NoBadWordsLogitsProcessor (transformers 4.18) plus this library's capacity;
    returns the bad words as a tuple of tuples without [eos] and without duplicates, or None"""
    p = repetition_penalty
    # the kernels take the penalty as fp32: it has to be finite and > 0 after that rounding (1e39 would be inf, 1e-50 would be 0)
    ok = isinstance(p, numbers.Real) and not isinstance(p, bool)
    if ok:
        ok = 0.0 < _f32(p) < float("inf")
    if not ok:
        raise ValueError(f"`repetition_penalty` has to be a strictly positive, finite float (as float32), but is {p!r}")
    if bad_words_ids is None:
        return None
    if not isinstance(bad_words_ids, (list, tuple)) or len(bad_words_ids) == 0:
        raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bad_words_ids!r}.")
    if any(not isinstance(w, (list, tuple)) or len(w) == 0 for w in bad_words_ids):
        raise ValueError(f"`bad_words_ids` has to be a list of non-empty lists, but is {bad_words_ids!r}.")
    V = int(model.V) if getattr(model, "V", None) is not None else int(model.config.vocab_size)
    if any(isinstance(t, bool) or not isinstance(t, int) or t < 0 or t >= V for w in bad_words_ids for t in w):
        raise ValueError(f"Each list in `bad_words_ids` has to be a list of integers in [0, {V}), but is {bad_words_ids!r}.")
    eos = model.config.eos_token_id
    words = tuple(dict.fromkeys(tuple(w) for w in bad_words_ids if tuple(w) != (eos,)))       # [eos] is dropped, as 4.18 drops it
    if len(words) > K.BAD_WORDS_MAX or any(len(w) > K.BAD_WORD_LEN for w in words):
        raise ValueError(f"`bad_words_ids`: at most {K.BAD_WORDS_MAX} words of at most {K.BAD_WORD_LEN} tokens each are supported, "
                         f"got {len(words)} words, the longest of {max(len(w) for w in words)} tokens")
    return words or None


class CachedDecoder:
    """Single-token decoder over preallocated KV caches (eval mode, no autograd).  All buffers are allocated once and the
    cache in use at position t is `cache[t & 1]` when beams are reordered every step (no hidden toggle), so a step is a pure
    function of (static buffers, t) and can be captured as a hipGraph."""

    def __init__(self, model, rows, S, max_length, reorders):
        self.m = model
        dec = model.model.decoder
        self.dec = dec
        self.L = len(dec.layers)
        d = model.config.d_model
        self.d, self.H = d, model.config.decoder_attention_heads
        self.rows, self.Tmax, self.S, self.reorders = rows, max_length, S, reorders
        dev = model.emb16_pad.device
        # one extra position per row: the fused k|v|q projection of position t is written IN PLACE at [row, t, 0:3d] — k|v
        # land in their cache slot, q parks in the first d columns of position t+1 (overwritten by that position's own k
        # before anything reads it), so no append copy is needed (MFULL:489-492 does torch.cat per step)
        self.cache = [torch.zeros((self.L, rows, max_length + 1, 2 * d), device=dev, dtype=BF16) for _ in range(2 if reorders else 1)]
        self.enc_b = torch.empty((rows, S, d), device=dev, dtype=BF16)
        self.enc_mask = torch.empty((rows, S), device=dev, dtype=torch.uint8)
        self.cross_all = torch.empty((self.L, rows, S, 2 * d), device=dev, dtype=BF16)      # one block: a staged caption arrives in one copy
        self.cross = [self.cross_all[li] for li in range(self.L)]
        self.lidx = (torch.arange(self.L, device=dev)[:, None] * rows).contiguous()
        # persistent decoder-step kernel (vacnic_decoder_step): all layers of a position in one launch, G = max(d/4, F/16)
        # co-resident workgroups exchanging through tagged slots.  Every other shape, and VACNIC_DECODE_PER_OP=1, takes the
        # kernel-per-op chain (the reference the step kernel is tested against).
        F = dec.layers[0].fc1.weight.shape[0]
        self.F = F
        G = max(d // 4, F // 16)
        self.step_kernel = (os.environ.get("VACNIC_DECODE_PER_OP", "0") != "1" and rows <= 8 and d <= 1024 and d % 16 == 0 and F <= 4096
                            and F % 16 == 0 and self.H * 64 == d and max_length <= 8191 and self.L <= 120 and rows * self.H <= min(128, G)
                            and G <= min(256, torch.cuda.get_device_properties(dev).multi_processor_count))
        self.step_table = None
        self.trace, self.trace_wg = None, 0       # tools/decstep_trace.py: per-phase time stamps of one workgroup
        self.last_hidden = None
        self.slots = None
        if self.step_kernel:
            self.sync = torch.zeros(int(_lib.lib.vacnic_decoder_step_sync_bytes()) // 4, device=dev, dtype=torch.int32)
            self.slots = torch.zeros(int(_lib.lib.vacnic_decoder_step_slots_bytes(self.L)), device=dev, dtype=torch.uint8)
            self.obuf = torch.zeros((rows, d), device=dev, dtype=BF16)

    def begin(self, enc_h, mask_u8, nb):
        """expand the encoder states to beams (HF _expand_inputs_for_generation: row b*nb + j <- batch b) and compute the
        cross-attention K/V of every layer once (the decoder's largest GEMMs: M = rows*S)."""
        B, S, d = enc_h.shape
        for j in range(nb):
            K.copy3d(enc_h, self.enc_b[j::nb], B, S, d)
        self.enc_mask.copy_(mask_u8.repeat_interleave(nb, dim=0))
        # one caption (B == 1): all beams attend to the SAME source, so the cross-attention K/V are projected once for the single
        # row and every beam reads them through a batch stride of 0 (5x fewer bytes per token, L2-resident after the first beam)
        self.shared_kv = B == 1
        src, M = (enc_h, S) if self.shared_kv else (self.enc_b, self.rows * S)
        for li, layer in enumerate(self.dec.layers):
            a = layer.encoder_attn
            K.gemm(src.reshape(M, d), a.s_kv.w16, M, 2 * d, d, bias=a.s_kv.bias, out=self.cross[li].view(self.rows * S, 2 * d)[:M])

    def begin_staged(self, stage):
        """begin() for a caption whose encoder side ran ahead of time (EncodeStage, B == 1): the cross-attention K/V of every layer
        and the key mask are copied from the staging buffers (24 MB device to device at BART-large: ~15 us)."""
        if self.rows != stage.nb or self.S != stage.S:
            raise ValueError("begin_staged: the stage was encoded for another decode shape")
        self.shared_kv = True
        S, d = self.S, self.d
        K.copy3d(stage.cross_all, self.cross_all[:, 0], self.L, S, 2 * d)
        self.enc_mask.copy_(stage.mask.expand(self.rows, S))

    def cache_at(self, t):
        return self.cache[t & 1] if self.reorders else self.cache[0]

    def _layer_table(self):
        """device array of vacnic_decoder_layer (weights / biases / LayerNorm parameters / cross K|V of every layer)."""
        if self.step_table is None or self.step_table[1] != self.shared_kv:
            d, S = self.d, self.S
            arr = (_lib.DecoderLayer * self.L)()
            for li, layer in enumerate(self.dec.layers):
                a, c = layer.self_attn, layer.encoder_attn
                mats = {"w_kvq": (a.s_kvq.w16, 3 * d, d), "w_so": (a.s_out.w16, d, d), "w_cq": (c.s_q.w16, d, d), "w_co": (c.s_out.w16, d, d),
                        "w_fc1": (layer.s_fc1.w16, self.F, d), "w_fc2": (layer.s_fc2.w16, d, self.F)}
                for name, (w, n, k) in mats.items():
                    if tuple(w.shape) != (n, k) or not w.is_contiguous():
                        raise ValueError(f"decoder_step: {name} of layer {li} must be a contiguous [{n}, {k}] matrix, got {tuple(w.shape)}")
                    setattr(arr[li], name, w.data_ptr())
                for name, b in (("b_kvq", a.s_kvq.bias), ("b_so", a.s_out.bias), ("b_cq", c.s_q.bias), ("b_co", c.s_out.bias),
                                ("b_fc1", layer.s_fc1.bias), ("b_fc2", layer.s_fc2.bias)):
                    setattr(arr[li], name, b.data_ptr() if b is not None else None)
                for name, ln in (("ln_self", layer.self_attn_layer_norm), ("ln_cross", layer.encoder_attn_layer_norm),
                                 ("ln_final", layer.final_layer_norm)):
                    setattr(arr[li], name + "_g", ln.weight.data.data_ptr())
                    setattr(arr[li], name + "_b", ln.bias.data.data_ptr())
                arr[li].cross_kv = self.cross[li].data_ptr()
                arr[li].cross_bs = 0 if self.shared_kv else S * 2 * d
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            self.step_table = (host.to(self.cache[0].device), self.shared_kv)
        return self.step_table[0]

    def _step_all_layers(self, h, t):
        """every decoder layer of position t in one launch; returns the decoder's final hidden rows [rows, d] (after the last
        layer's LayerNorm)."""
        lay = self.dec.layers[0]
        _lib.call_struct("vacnic_decoder_step", stream=K._stream(), layers=self._layer_table().data_ptr(), cache=self.cache_at(t).data_ptr(),
                         h0=h.data_ptr(), obuf=self.obuf.data_ptr(), enc_mask=self.enc_mask.data_ptr(), sync=self.sync.data_ptr(),
                         slots=self.slots.data_ptr(), L=self.L, R=self.rows, d=self.d, H=self.H, F=self.F, S=self.S, t=t, Tmax=self.Tmax,
                         eps=lay.final_layer_norm.eps, scale=0.125, trace=self.trace.data_ptr() if self.trace is not None else None,
                         trace_wg=self.trace_wg)
        return self.obuf

    def check_step_kernel(self):
        """after the results were read back: did a wait of the step kernel for another workgroup's slot time out?"""
        if self.step_kernel and int(self.sync[-64].item()) != 0:
            # a timed-out launch left the error word, the launch nonce and units tagged with that nonce behind: clear BOTH buffers,
            # so that a later launch can never match stale tags, and take this decoder off the step kernel — whoever keeps using
            # it (a cached DecodeSession) continues on the kernel-per-op chain
            self.sync.zero_()
            self.slots.zero_()
            self.step_kernel = False
            self.step_table = None
            raise RuntimeError("vacnic_decoder_step: a wait inside the step kernel timed out (workgroups not co-resident?); results of "
                               "this caption are invalid; this decoder falls back to the kernel-per-op chain")

    def step(self, ids_t, t, hidden_only=False):
        """ids_t int64 [rows, 1] (token at position t) -> fp32 logits [rows, V_pad]; hidden_only: the decoder's final hidden rows
        [rows, d] (bf16, after the last layer's LayerNorm) instead — the input of kernels.lmhead_topk."""
        m, dec, d, H, R = self.m, self.dec, self.d, self.H, self.rows
        ln = dec.layernorm_embedding
        h, _, _ = K.embed_ln_fwd(ids_t, dec.embed_tokens.weight.w16, dec.embed_positions.weight.w16, ln.weight.data, ln.bias.data,
                                 embed_scale=dec.embed_scale, pos_offset=2 + t)
        if self.step_kernel:
            hn = self._step_all_layers(h.view(R, d), t)
            self.last_hidden = hn
            if hidden_only:
                return hn
            logits = torch.empty((R, m.V_pad), device=h.device, dtype=torch.float32)
            K.gemm(hn, m.emb16_pad, R, m.V, d, bias=m.final_logits_bias.view(-1), out=logits, ldo=m.V_pad, out_mode=1)
            return logits
        cache = self.cache_at(t)
        # R <= 8 rows (one caption, <= 8 beams): every post-LN (residual add + LayerNorm) rides as a prologue on the projection
        # that consumes it (vacnic_gemv_ln_bf16) — 36 fewer launches per token, bit-identical values.  `pend` = the block output
        # and residual whose LayerNorm has not been applied yet.
        fuse = R <= 8 and d <= 1024 and d % 8 == 0
        pend = None

        def ln_then(lnm, w, N, bias, out=None, ldo=None, act=None, out_mode=0):
            o_, res_ = pend
            hn = torch.empty((R, d), device=o_.device, dtype=BF16)
            y = K.gemv_ln(o_.view(R, d), res_.view(R, d), lnm.weight.data, lnm.bias.data, w, R, N, d, bias=bias, out=out, ln_out=hn,
                          ldw=w.stride(0), ldo=ldo, act=act, out_mode=out_mode, eps=lnm.eps)
            return y, hn

        for li, layer in enumerate(dec.layers):
            a = layer.self_attn
            row = cache[li][:, t]                                                               # [R, 2d] view, row stride (Tmax+1)*2d
            if pend is None:
                K.gemm(h.view(R, d), a.s_kvq.w16, R, 3 * d, d, bias=a.s_kvq.bias, out=row, ldo=row.stride(0))   # k|v|q in place
            else:
                _, h = ln_then(pend_ln, a.s_kvq.w16, 3 * d, a.s_kvq.bias, out=row, ldo=row.stride(0))
            q = cache[li][:, t + 1:t + 2, :d]
            ctx, _ = K.attn_fwd(q, cache[li][:, :t + 1, :d], cache[li][:, :t + 1, d:], R, H, 1, t + 1, need_lse=False)
            o = K.gemm(ctx.view(R, d), a.s_out.w16, R, d, d, bias=a.s_out.bias)
            c = layer.encoder_attn
            if fuse:
                pend = (o, h)
                q, h = ln_then(layer.self_attn_layer_norm, c.s_q.w16, d, c.s_q.bias)
                q = q.view(R, 1, d)
            else:
                h, _, _ = K.add_ln_fwd(o.view(R, 1, d), h, layer.self_attn_layer_norm.weight.data, layer.self_attn_layer_norm.bias.data,
                                       need_stats=False)
                q = K.gemm(h.view(R, d), c.s_q.w16, R, d, d, bias=c.s_q.bias).view(R, 1, d)
            kv = self.cross[li][:1].expand(R, -1, -1) if self.shared_kv else self.cross[li]
            ctx, _ = K.attn_fwd(q, kv[..., :d], kv[..., d:], R, H, 1, kv.shape[1], key_mask=self.enc_mask, need_lse=False)
            o = K.gemm(ctx.view(R, d), c.s_out.w16, R, d, d, bias=c.s_out.bias)
            if fuse:
                pend = (o, h)
                f, h = ln_then(layer.encoder_attn_layer_norm, layer.s_fc1.w16, layer.s_fc1.N, layer.s_fc1.bias, act="gelu")
            else:
                h, _, _ = K.add_ln_fwd(o.view(R, 1, d), h, layer.encoder_attn_layer_norm.weight.data, layer.encoder_attn_layer_norm.bias.data,
                                       need_stats=False)
                f = K.gemm(h.view(R, d), layer.s_fc1.w16, R, layer.s_fc1.N, d, bias=layer.s_fc1.bias, act="gelu")
            o = K.gemm(f, layer.s_fc2.w16, R, d, layer.s_fc2.K, bias=layer.s_fc2.bias)
            if fuse:
                pend, pend_ln = (o, h), layer.final_layer_norm
            else:
                h, _, _ = K.add_ln_fwd(o.view(R, 1, d), h, layer.final_layer_norm.weight.data, layer.final_layer_norm.bias.data, need_stats=False)
        if hidden_only:
            if fuse and pend is not None:
                o_, res_ = pend
                hn, _, _ = K.add_ln_fwd(o_.view(R, 1, d), res_.view(R, 1, d), pend_ln.weight.data, pend_ln.bias.data, need_stats=False)
                self.last_hidden = hn.view(R, d)
            else:
                self.last_hidden = h.view(R, d)
            return self.last_hidden
        logits = torch.empty((R, m.V_pad), device=h.device, dtype=torch.float32)
        # last_hidden: the final hidden rows [R, d] behind these logits (diagnostics / fixture construction; overwritten every step)
        if fuse and pend is not None:
            _, self.last_hidden = ln_then(pend_ln, m.emb16_pad, m.V, m.final_logits_bias.view(-1), out=logits, ldo=m.V_pad, out_mode=1)
        else:
            K.gemm(h.view(R, d), m.emb16_pad, R, m.V, d, bias=m.final_logits_bias.view(-1), out=logits, ldo=m.V_pad, out_mode=1)
            self.last_hidden = h.view(R, d)
        return logits

    def reorder(self, beam_idx, t):
        """before step t: the self-attention caches of all layers follow their beams (one launch; _reorder_cache
        MFULL:2066-2074): cache[(t-1)&1] gathered into cache[t&1]."""
        L, R = self.L, self.rows
        # one permutation for every layer's block of R rows (period = R), and only the t positions filled so far (+ the slot where
        # the per-op path parks q) travel: half the bytes of whole rows on average, no index arithmetic on the host side
        K.gather_rows(self.cache[(t - 1) & 1], self.cache[t & 1], beam_idx, L * R, (t + 1) * 2 * self.d * 2,
                      row_stride_bytes=(self.Tmax + 1) * 2 * self.d * 2, period=R)


class DecodeSession:
    """Everything device-side of one decode shape (rows, S, max_length, logits-processor options): static buffers, the
    cached decoder, and one hipGraph per position t = {cache reorder, 12-layer single-token decoder, LM head, log-softmax +
    processors + top-2k}.  The first caption of a shape runs eagerly (it also warms every kernel); from the second on each
    position is captured on first use and replayed afterwards, which removes the ~170 Python->HIP launches per token that
    bound the eager loop."""

    def __init__(self, model, R, S, max_length, nb, ngram, min_length, forced_eos, eos, forced_bos=None, bad_words=None, penalty=1.0,
                 groups=None):
        self.model, self.R, self.nb, self.max_length = model, R, nb, max_length
        # group (diverse) beam search: (num_beam_groups, diversity_penalty) with more than one group, else None — the position's tail is
        # the same call; vacnic_group_beam_step takes the place of vacnic_beam_step behind it
        self.groups = (int(groups[0]), float(groups[1])) if groups and int(groups[0]) > 1 else None
        self.ngram, self.min_length, self.forced_eos, self.eos = ngram, min_length, forced_eos, eos
        self.forced_bos = forced_bos
        dev = model.emb16_pad.device
        # NoBadWords: the table is uploaded once; its bans ride in the ban lists behind the n-gram bans (max_length + n_bad wide)
        self.bad = K.bad_words_table(bad_words, dev) if bad_words else None
        self.n_bad = len(bad_words) if bad_words else 0
        banned = ngram > 0 or self.n_bad > 0
        # RepetitionPenalty: on the logits for one beam (HF greedy_search), on the log-softmax scores for more (HF beam_search); the
        # top-k kernels read the histories from the beam state (device bookkeeping) or from hist_s (host loop: uploaded per position)
        self.penalty = float(penalty)
        self.pen_rule = None if self.penalty == 1.0 else ("logits" if nb == 1 else "scores")
        self.hist_s = self.h_hist = None
        if self.pen_rule:
            self.hist_s = torch.zeros((R, max_length), device=dev, dtype=torch.int32)
            self.h_hist = torch.zeros((R, max_length), dtype=torch.int32).pin_memory()
        self.dec = CachedDecoder(model, R, S, max_length, reorders=nb > 1)
        self.ids_s = torch.zeros((R, 1), device=dev, dtype=torch.long)
        self.scores_s = torch.zeros(R, device=dev, dtype=torch.float32)
        self.src_s = torch.zeros(R, device=dev, dtype=torch.long)
        self.bans_s = torch.full((R, max_length + self.n_bad), -1, device=dev, dtype=torch.int32) if banned else None
        self.h_ids = torch.zeros((R, 1), dtype=torch.long).pin_memory()
        self.h_scores = torch.zeros(R, dtype=torch.float32).pin_memory()
        self.h_src = torch.zeros(R, dtype=torch.long).pin_memory()
        self.h_bans = torch.full((R, max_length + self.n_bad), -1, dtype=torch.int32).pin_memory() if banned else None
        self.graphs, self.outs, self.pool = {}, {}, None
        # few rows (one caption's beams): the fused LM head + top-k; other shapes: skinny GEMM -> vacnic_beam_topk
        # (the library's own predicate: at V = 50265 the merge's LDS admits 2 nb <= 45, wider beams take the chain)
        self.fused_tail = bool(_lib.lib.vacnic_lmhead_topk_supported(R, model.V, model.emb16_pad.shape[1], min(2 * nb, model.V)))
        self.captions = 0
        self.beam = None                  # device-side beam bookkeeping (enable_device_beams)

    def enable_device_beams(self, B, length_penalty, early_stopping, pad):
        """state of vacnic_beam_step: token histories, n-best lists and done flags live in HBM; the step kernel
        also writes this session's next-token / beam-score / reorder-index / ban buffers, so a position needs no host round trip."""
        from . import _lib
        dev = self.ids_s.device
        R, nb, L = self.R, self.nb, self.max_length
        i32 = dict(device=dev, dtype=torch.int32)
        if self.bans_s is None and self.ngram > 0:
            self.bans_s = torch.full((R, L), -1, **i32)
        self.seq = torch.zeros((2, R, L), **i32)
        self.done_d = torch.zeros(B, **i32)
        self.h_done = torch.zeros(B, dtype=torch.int32).pin_memory()
        self.hyp_cnt = torch.zeros(B, **i32)
        self.hyp_worst = torch.zeros(B, device=dev, dtype=torch.float64)
        self.hyp_score = torch.zeros((B, nb), device=dev, dtype=torch.float64)
        self.hyp_len = torch.zeros((B, nb), **i32)
        self.hyp_seq = torch.zeros((B, nb, L), **i32)
        self.B, self.lp, self.early, self.pad = B, length_penalty, early_stopping, pad
        self.beam = _lib.BeamState(seq0=self.seq[0].data_ptr(), seq1=self.seq[1].data_ptr(), beam_scores=self.scores_s.data_ptr(),
                                   done=self.done_d.data_ptr(), hyp_cnt=self.hyp_cnt.data_ptr(), hyp_worst=self.hyp_worst.data_ptr(),
                                   hyp_score=self.hyp_score.data_ptr(), hyp_len=self.hyp_len.data_ptr(), hyp_seq=self.hyp_seq.data_ptr(),
                                   next_ids=self.ids_s.data_ptr(), src_idx=self.src_s.data_ptr(),
                                   bans=self.bans_s.data_ptr() if self.bans_s is not None else None,
                                   B=B, nb=nb, Lmax=L, V=self.model.V, eos=self.eos, pad=pad, no_repeat_ngram_size=self.ngram,
                                   early_stopping=int(bool(early_stopping)), length_penalty=float(length_penalty),
                                   bad_words=self.bad[0].data_ptr() if self.bad else None, bad_len=self.bad[1].data_ptr() if self.bad else None,
                                   n_bad=self.n_bad)

    def run_device(self, start, use_graphs):
        """the whole beam search of one batch without per-token host synchronisation; returns the host-side tensors finalize needs."""
        from . import _lib
        st = K._stream()
        if self.groups:
            ga = K.group_beam_args(self.groups)
            _lib.check(_lib.lib.vacnic_group_beam_init(_lib.C.byref(self.beam), _lib.C.byref(ga), int(start), st))
        else:
            _lib.check(_lib.lib.vacnic_beam_init(_lib.C.byref(self.beam), int(start), st))
        steps = 0
        pending = None                                       # (event, pinned copy of the done flags): polled without blocking the launches
        for t in range(self.max_length - 1):
            if use_graphs and self.captions > 0:
                g = self.graphs.get(t)
                if g is None:
                    g = torch.cuda.CUDAGraph()
                    torch.cuda.synchronize()
                    with K.capture_scope(("decode-session", id(self))), torch.cuda.graph(g, pool=self.pool):
                        self.body(t)
                    if self.pool is None:
                        self.pool = g.pool()
                    self.graphs[t] = g
                g.replay()
            else:
                self.body(t)
            steps = t + 1
            # early stop: the done flags are copied out every 8th position and looked at when the copy has landed, so the launch
            # path never waits; positions enqueued in the meantime only pad finished items (BeamSearchScorer.process on done batches)
            if pending is not None and pending[0].query():
                if bool(pending[1].all()):
                    break
                pending = None
            if pending is None and t % 8 == 7 and t + 1 < self.max_length - 1:
                self.h_done.copy_(self.done_d, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                pending = (ev, self.h_done)
        cur_len = steps + 1                                  # tokens in every live history
        seqs = self.seq[steps & 1].cpu()
        self.dec.check_step_kernel()
        return (cur_len, seqs, self.scores_s.cpu(), self.done_d.cpu(), self.hyp_cnt.cpu(), self.hyp_score.cpu(), self.hyp_len.cpu(),
                self.hyp_seq.cpu())

    def forced_at(self, cur_len):
        """the forced token of the position whose histories hold cur_len tokens, or -1"""
        forced = self.forced_eos if (self.forced_eos is not None and cur_len == self.max_length - 1) else -1
        if self.forced_bos is not None and cur_len == 1:             # ForcedBOSTokenLogitsProcessor (runs before ForcedEOS in HF)
            forced = self.forced_bos if forced < 0 else forced
        return forced

    def body(self, t):
        if self.nb > 1 and t > 0:
            self.dec.reorder(self.src_s, t)
        cur_len = t + 1
        forced = self.forced_at(cur_len)
        V = self.model.V
        pen = {}
        if self.pen_rule:
            pen = dict(history=self.seq[t & 1] if self.beam is not None else self.hist_s, cur_len=cur_len, repetition_penalty=self.penalty,
                       penalty_rule=self.pen_rule)
        if self.fused_tail:
            # LM head + log_softmax + processors + top-2nb in one C call, no [R, V] logits (a forced position needs no LM head at all)
            hid = self.dec.step(self.ids_s, t, hidden_only=True)
            tv, ti = K.lmhead_topk(hid, self.model.emb16_pad, V, min(2 * self.nb, V), bias=self.model.final_logits_bias.view(-1),
                                   beam_scores=self.scores_s, bans=self.bans_s, eos=self.eos, suppress_eos=cur_len < self.min_length,
                                   forced_token=forced, **pen)
        else:
            logits = self.dec.step(self.ids_s, t)
            tv, ti = K.beam_topk(logits, V, min(2 * self.nb, V), beam_scores=self.scores_s, bans=self.bans_s, eos=self.eos,
                                 suppress_eos=cur_len < self.min_length, forced_token=forced, **pen)
        if self.beam is not None:
            from . import _lib
            if self.groups:
                ga = K.group_beam_args(self.groups, forced, self.penalty, self.pen_rule)
                _lib.check(_lib.lib.vacnic_group_beam_step(_lib.C.byref(self.beam), _lib.C.byref(ga), tv.data_ptr(), ti.data_ptr(), tv.shape[1],
                                                           cur_len, K._stream()))
            else:
                _lib.check(_lib.lib.vacnic_beam_step(_lib.C.byref(self.beam), tv.data_ptr(), ti.data_ptr(), tv.shape[1], cur_len, K._stream()))
        return tv, ti

    def step(self, t, last_tokens, scores, src, bans, use_graphs, seqs=None):
        """host lists in, (top values, top ids) on the host out — the one device->host sync of the position."""
        if self.pen_rule:
            self.h_hist[:, :t + 1] = torch.as_tensor(seqs, dtype=torch.int32)
            self.hist_s.copy_(self.h_hist, non_blocking=True)
        self.h_ids[:, 0] = torch.as_tensor(last_tokens)
        self.ids_s.copy_(self.h_ids, non_blocking=True)
        self.h_scores.copy_(torch.as_tensor(scores, dtype=torch.float32))
        self.scores_s.copy_(self.h_scores, non_blocking=True)
        if self.nb > 1 and t > 0:
            self.h_src.copy_(torch.as_tensor(src))
            self.src_s.copy_(self.h_src, non_blocking=True)
        if self.bans_s is not None:
            self.h_bans.fill_(-1)
            for r, bl in enumerate(bans):
                if bl:
                    self.h_bans[r, :len(bl)] = torch.as_tensor(bl, dtype=torch.int32)
            self.bans_s.copy_(self.h_bans, non_blocking=True)
        if use_graphs and self.captions > 0:
            g = self.graphs.get(t)
            if g is None:
                g = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                with K.capture_scope(("decode-session", id(self))), torch.cuda.graph(g, pool=self.pool):
                    self.outs[t] = self.body(t)
                if self.pool is None:
                    self.pool = g.pool()
                self.graphs[t] = g
            g.replay()
            tv, ti = self.outs[t]
        else:
            tv, ti = self.body(t)
        tv, ti = tv.cpu(), ti.cpu()
        self.dec.check_step_kernel()
        return tv, ti


class SampleSession:
    """Device side of sampling decode for one shape (rows, S, max_length, logits-processor options): the cached decoder, the token
    histories / log-probs / done flags, and one hipGraph per position t = {single-token decoder, LM-head logits, vacnic_sample_step}.
    Temperature, top-k, top-p, seed and call counter live in an 8-word device buffer the kernel reads at run time, so the graphs of
    a shape serve every setting.  As in DecodeSession the first caption runs eagerly and later ones replay."""

    def __init__(self, model, R, S, max_length, ngram, min_length, forced_eos, eos, pad, forced_bos=None, bad_words=None):
        self.model, self.R, self.max_length = model, R, max_length
        self.ngram, self.min_length, self.forced_eos, self.eos, self.pad, self.forced_bos = ngram, min_length, forced_eos, eos, pad, forced_bos
        dev = model.emb16_pad.device
        self.bad = K.bad_words_table(bad_words, dev) if bad_words else None      # uploaded once; its address is part of the captured launches
        self.dec = CachedDecoder(model, R, S, max_length, reorders=False)
        self.ids_s = torch.zeros((R, 1), device=dev, dtype=torch.long)
        self.state = torch.zeros((2, R, max_length), device=dev, dtype=torch.int32)     # histories | log-probs: one copy out at the end
        self.seq, self.logp = self.state[0], self.state[1].view(torch.float32)
        self.done_d = torch.zeros(R, device=dev, dtype=torch.int32)
        self.h_done = torch.zeros(R, dtype=torch.int32).pin_memory()
        self.params = torch.zeros(8, device=dev, dtype=torch.int32)
        self.h_params = torch.zeros(8, dtype=torch.int32).pin_memory()
        self.graphs, self.pool, self.captions = {}, None, 0

    def body(self, t):
        cur_len = t + 1
        forced = self.forced_eos if (self.forced_eos is not None and cur_len == self.max_length - 1) else -1
        if self.forced_bos is not None and cur_len == 1:             # ForcedBOS runs before ForcedEOS, as in DecodeSession.body
            forced = self.forced_bos if forced < 0 else forced
        logits = self.dec.step(self.ids_s, t)
        K.sample_step(logits, self.model.V, self.params, self.seq, self.done_d, self.ids_s, cur_len, logp=self.logp, eos=self.eos,
                      pad=self.pad, no_repeat_ngram_size=self.ngram, suppress_eos=cur_len < self.min_length, forced_token=forced,
                      bad_words=self.bad)

    def run(self, start, use_graphs, temperature, top_k, top_p, seed, call, repetition_penalty=1.0):
        """every position enqueued back to back; returns (tokens per row, histories int32 [R, L], log-probs fp32 [R, L]) on the host"""
        K.sample_params(temperature, top_k, top_p, seed, call, out=self.h_params, repetition_penalty=repetition_penalty)
        self.params.copy_(self.h_params, non_blocking=True)
        self.state.zero_()
        self.seq.fill_(self.pad)
        self.seq[:, 0] = start
        self.ids_s.fill_(start)
        self.done_d.zero_()
        steps, pending = 0, None
        for t in range(self.max_length - 1):
            if use_graphs and self.captions > 0:
                g = self.graphs.get(t)
                if g is None:
                    g = torch.cuda.CUDAGraph()
                    torch.cuda.synchronize()
                    with K.capture_scope(("sample-session", id(self))), torch.cuda.graph(g, pool=self.pool):
                        self.body(t)
                    if self.pool is None:
                        self.pool = g.pool()
                    self.graphs[t] = g
                g.replay()
            else:
                self.body(t)
            steps = t + 1
            # early stop as in DecodeSession.run_device: the done flags travel every 8th position and are looked at once they landed
            if pending is not None and pending[0].query():
                if bool(pending[1].all()):
                    break
                pending = None
            if pending is None and t % 8 == 7 and t + 1 < self.max_length - 1:
                self.h_done.copy_(self.done_d, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                pending = (ev, self.h_done)
        host = self.state.cpu()
        self.dec.check_step_kernel()
        return steps + 1, host[0], host[1].view(torch.float32)


_SAMPLE_CALLS = 0          # per-process count of generate(do_sample=True, seed=None) calls: successive calls draw differently
_SAMPLE_SESSIONS_MAX = 8   # sampling sessions (KV cache, cross K/V, position graphs) a model keeps: rows = B * num_return_sequences is a
                           # free axis of the key, so the least recently used session goes when a ninth shape arrives
_DECODE_KEY_LEN = 9        # entries of a DecodeSession key without processors; (bad words, penalty) follow when either is on
_PROCESSOR_SESSIONS_MAX = 8   # beam / greedy sessions with processors a model keeps (each holds a KV cache and position graphs)


def _decode_session_key(R, S, max_length, nb, ngram, min_length, forced_eos, forced_bos, beams, bad_words, penalty, groups=None):
    """what a DecodeSession is kept under: the shape and the options baked into its launches; the processors join it only when one
    is on (the penalty as the float32 the kernels see), and (num_beam_groups, diversity_penalty as float32) only with more than one
    group, so that the default key is the one of before"""
    key = (R, S, max_length, nb, ngram, min_length, forced_eos, forced_bos, beams)
    if bad_words or penalty != 1.0:
        key = key + (bad_words, penalty)
    if groups and groups[0] > 1:
        key = key + (int(groups[0]), _f32(groups[1]))
    return key


def _check_group_args(num_beams, num_beam_groups, diversity_penalty, do_sample, encoded):
    """the checks of transformers 4.18 on num_beam_groups / diversity_penalty, plus this library's: a diversity penalty without groups
    is an error here (HF ignores it), and groups do not combine with staged encoding.  Returns (G, penalty as float32)."""
    G, lam = num_beam_groups, diversity_penalty
    if isinstance(G, bool) or not isinstance(G, int) or G < 1:
        raise ValueError(f"`num_beam_groups` has to be an integer >= 1, but is {G!r}")
    ok = isinstance(lam, numbers.Real) and not isinstance(lam, bool)
    if ok:
        ok = 0.0 <= _f32(lam) < float("inf")
    if not ok:
        raise ValueError(f"`diversity_penalty` has to be a finite float >= 0 (as float32), but is {lam!r}")
    if G > num_beams:
        raise ValueError("`num_beam_groups` has to be smaller or equal to `num_beams`")
    if num_beams % G != 0:
        raise ValueError("`num_beams` should be divisible by `num_beam_groups`")
    if G > 1 and do_sample:
        raise ValueError("Diverse beam search cannot be used in sampling mode. Make sure that `do_sample` is set to `False`.")
    if G == 1 and _f32(lam) != 0.0:
        raise ValueError(f"`diversity_penalty` = {lam!r} needs `num_beam_groups` > 1 (it would be ignored: pass 0.0 or ask for groups)")
    if G > 1 and encoded is not None:
        raise ValueError("generate(encoded=...): staged encoding is not supported with `num_beam_groups` > 1")
    return G, _f32(lam)


def nbest_to_sequences(nbest, n, pad, eos, max_length):
    """the n best hypotheses of every item of a return_nbest list as BeamSearchScorer.finalize(num_beam_hyps_to_keep=n) of transformers
    4.18 lays them out: int64 [B * n, L] (row b * n + j = the j-th best of item b; its ids, eos behind a hypothesis shorter than L, then
    pad) and the float32 scores [B * n]; L = min(longest + 1, max_length).  The n-best list of a (diverse) beam search goes through
    this into training.sequences_to_labels -> model.score."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"nbest_to_sequences: n has to be an integer >= 1, but is {n!r}")
    if any(len(item) < n for item in nbest):
        raise ValueError(f"nbest_to_sequences: n = {n}, but an item has only {min(len(item) for item in nbest)} hypotheses")
    rows = [(sc, sq) for item in nbest for sc, sq in item[:n]]
    L = min(max(len(sq) for _, sq in rows) + 1, max_length)
    ids = torch.full((len(rows), L), pad, dtype=torch.long)
    for r, (_, sq) in enumerate(rows):
        ids[r, :len(sq)] = torch.tensor(sq, dtype=torch.long)
        if len(sq) < L:
            ids[r, len(sq)] = eos
    return ids, torch.tensor([sc for sc, _ in rows], dtype=torch.float32)


def _sample_session_key(R, S, max_length, ngram, min_length, forced_eos, forced_bos, bad_words):
    """what a SampleSession is kept under: no T / top_k / top_p / seed / penalty (run-time parameters of the kernel); the bad-word
    table's address is part of the captured launches, so the word set joins the key when there is one"""
    key = (R, S, max_length, ngram, min_length, forced_eos, forced_bos)
    return key + (bad_words,) if bad_words else key


def _check_sampling_args(num_beams, encoded, temperature, top_k, top_p, num_return_sequences):
    if num_beams != 1:
        raise ValueError(f"generate(do_sample=True): num_beams must be 1, got {num_beams} (beam-sample is not supported)")
    if encoded is not None:
        raise ValueError("generate(do_sample=True): encoded= (staged encoding) is not supported with sampling")
    if not (isinstance(temperature, (int, float)) and temperature > 0 and temperature != float("inf")):
        raise ValueError(f"generate(do_sample=True): temperature must be a finite number > 0, got {temperature!r}")
    if not (isinstance(top_p, (int, float)) and 0 < top_p <= 1):
        raise ValueError(f"generate(do_sample=True): top_p must be in (0, 1], got {top_p!r}")
    if not (isinstance(top_k, int) and not isinstance(top_k, bool) and top_k >= 0):
        raise ValueError(f"generate(do_sample=True): top_k must be an integer >= 0, got {top_k!r}")
    if not (isinstance(num_return_sequences, int) and not isinstance(num_return_sequences, bool) and num_return_sequences >= 1):
        raise ValueError(f"generate(do_sample=True): num_return_sequences must be an integer >= 1, got {num_return_sequences!r}")


def _generate_sample(model, input_ids, attention_mask, max_length, no_repeat_ngram_size, min_length, forced_eos_token_id,
                     forced_bos_token_id, enc_args, add_ner_ffn, use_graphs, temperature, top_k, top_p, n, seed, return_logprobs,
                     repetition_penalty=1.0, bad_words=None):
    """GenerationMixin.sample of transformers 4.18 (generate(do_sample=True, num_beams=1)): rows b * n + j = sample j of item b."""
    global _SAMPLE_CALLS
    cfg = model.config
    eos, pad, start = cfg.eos_token_id, cfg.pad_token_id, cfg.decoder_start_token_id
    if seed is None:
        _SAMPLE_CALLS += 1
        seed, call = torch.initial_seed(), _SAMPLE_CALLS
    else:
        seed, call = int(seed), 0
    if max_length < 2:
        raise ValueError(f"generate(do_sample=True): max_length must be >= 2, got {max_length}")
    B = input_ids.shape[0]
    R = B * n
    mask_u8 = attention_mask.to(torch.uint8) if attention_mask.dtype != torch.uint8 else attention_mask
    enc_h = _run_encoder(model, use_graphs, add_ner_ffn, input_ids, mask_u8, *enc_args)
    S = enc_h.shape[1]
    key = _sample_session_key(R, S, max_length, no_repeat_ngram_size, min_length, forced_eos_token_id, forced_bos_token_id, bad_words)
    sessions = model.__dict__.setdefault("_sample_sessions", {})
    ses = sessions.pop(key, None)
    if ses is None:
        while len(sessions) >= _SAMPLE_SESSIONS_MAX:
            sessions.pop(next(iter(sessions)))           # (dicts keep insertion order: the first key is the least recently used)
        ses = SampleSession(model, R, S, max_length, no_repeat_ngram_size, min_length, forced_eos_token_id, eos, pad,
                            forced_bos=forced_bos_token_id, bad_words=bad_words)
    sessions[key] = ses                                  # most recently used last
    ses.dec.begin(enc_h, mask_u8, n)
    try:
        cur_len, seqs, logps = ses.run(start, use_graphs, float(temperature), int(top_k), float(top_p), seed, call,
                                       repetition_penalty=float(repetition_penalty))
    except Exception:
        sessions.pop(key, None)                          # its graphs / buffers may hold a half-finished caption
        raise
    ses.captions += 1
    seqs, logps = seqs[:, :cur_len], logps[:, :cur_len]
    # a row ends at its first eos after the start token (everything behind it is pad, log-prob 0); L = the longest row
    is_eos = seqs[:, 1:] == eos
    ends = torch.where(is_eos.any(1), is_eos.int().argmax(1) + 2, torch.full((R,), cur_len))
    L = int(ends.max())
    dev = model.emb16_pad.device
    ids = seqs[:, :L].to(torch.long).to(dev)
    return (ids, logps[:, :L].contiguous().to(dev)) if return_logprobs else ids


def _run_encoder(model, use_graphs, add_ner_ffn, input_ids, mask_u8, image_features, name_ids, name_mask, face_features, face_mask):
    """the encoder pass of one generate() call: a hipGraph per input signature (GraphedCall) unless use_graphs is off"""
    def run_encoder(ids, m8, img, nids, nmask, faces, fmask, add_ner_ffn=add_ner_ffn):
        return model.model.encoder(input_ids=ids, attention_mask=m8, image_features=img, name_ids=nids, name_mask=nmask,
                                   face_features=faces, face_mask=fmask, add_ner_ffn=add_ner_ffn,
                                   output_attentions=False)["last_hidden_state"]      # no maps in decoding, whatever the config says
    if not use_graphs:
        return run_encoder(input_ids, mask_u8, image_features, name_ids, name_mask, face_features, face_mask)
    ge = model.__dict__.setdefault("_graphed_encoders", {})
    if add_ner_ffn not in ge:
        ge[add_ner_ffn] = GraphedCall(run_encoder)
    return ge[add_ner_ffn](input_ids, mask_u8, image_features, name_ids, name_mask, face_features, face_mask)


class EncodeStage:
    """Everything the beam search of ONE caption (B == 1) needs from the encoder side, in buffers of its own: the cross-attention K/V
    of every decoder layer and the source key mask.  Filled by encode() on whatever stream is current — CaptionPipeline runs it on
    a side stream for caption i + 1 while caption i is being decoded — and consumed by generate(encoded=stage)."""

    def __init__(self, model, S, nb):
        dec = model.model.decoder
        d = model.config.d_model
        dev = model.emb16_pad.device
        self.S, self.d, self.nb = S, d, nb
        self.cross_all = torch.empty((len(dec.layers), S, 2 * d), device=dev, dtype=BF16)
        self.cross = [self.cross_all[li] for li in range(len(dec.layers))]
        self.mask = torch.empty((1, S), device=dev, dtype=torch.uint8)

    @torch.no_grad()
    def encode(self, model, input_ids, attention_mask, image_features=None, face_features=None, face_mask=None, name_ids=None, name_mask=None,
               add_ner_ffn=True, use_graphs=True):
        if input_ids.shape[0] != 1 or input_ids.shape[1] != self.S:
            raise ValueError("EncodeStage.encode: one caption of the staged source length")
        mask_u8 = attention_mask.to(torch.uint8) if attention_mask.dtype != torch.uint8 else attention_mask
        enc_h = _run_encoder(model, use_graphs, add_ner_ffn, input_ids, mask_u8, image_features, name_ids, name_mask, face_features, face_mask)
        S, d = self.S, self.d
        for li, layer in enumerate(model.model.decoder.layers):
            a = layer.encoder_attn
            K.gemm(enc_h.reshape(S, d), a.s_kv.w16, S, 2 * d, d, bias=a.s_kv.bias, out=self.cross[li])
        self.mask.copy_(mask_u8)
        return self


class CaptionPipeline:
    """model.generate over a stream of single captions (test_batch_size 1, the reference's generation loop TRAIN:480-530) as a
    pipeline of three stages on three streams: while caption i is in its beam search (a chain of latency-bound launches that
    leaves most of the GPU idle), the encoder and the cross-attention K/V projection of caption i + 1 run on a second stream and the
    masks + image tower of caption i + 2 on a third — none of them depends on the beam search.  Same ids as the sequential loop
    (the kernels are the same, only their streams differ).  `inputs_fn(batch)` -> (input_ids, attention_mask, image_features, kw)
    builds the masks and runs the image tower (training._model_inputs).  Batches with more than one caption decode through the
    plain generate() with their inputs_fn ahead."""

    def __init__(self, model, inputs_fn, num_beams, **gen_kw):
        self.model, self.inputs_fn, self.nb, self.gen_kw = model, inputs_fn, num_beams, gen_kw
        # (stream priorities change nothing: 34.7-34.8 ms per caption with one side stream either way)
        self.s_img, self.s_enc = torch.cuda.Stream(), torch.cuda.Stream()
        self.stages = {}

    def _inputs(self, batch, after):
        """stage A (image stream): masks + image tower of `batch`, not before event `after` (its tensors are on the device)"""
        with torch.cuda.stream(self.s_img):
            self.s_img.wait_event(after)
            src, src_mask, feats, kw = self.inputs_fn(batch)
            if feats is not None:
                feats = feats.clone()                       # a graphed image tower overwrites its output at its next call (which runs ahead)
            ev = torch.cuda.Event()
            ev.record(self.s_img)
        return {"batch": batch, "inputs": (src, src_mask, feats, kw), "a": ev, "stage": None, "b": ev}

    def _encode(self, ent, after):
        """stage B (encoder stream): encoder + cross K/V of one caption into the EncodeStage, not before `after` (the previous caption's
        staged data have been copied into the decoder's buffers)"""
        src, src_mask, feats, kw = ent["inputs"]
        # (sampling and group beam search decode through the plain generate(): no staging)
        if src.shape[0] != 1 or self.gen_kw.get("do_sample") or self.gen_kw.get("num_beam_groups", 1) != 1:
            return
        with torch.cuda.stream(self.s_enc):
            self.s_enc.wait_event(ent["a"])
            if after is not None:
                self.s_enc.wait_event(after)
            S = src.shape[1]
            stage = self.stages.get(S)
            if stage is None:
                stage = self.stages[S] = EncodeStage(self.model, S, self.nb)
            stage.encode(self.model, src, src_mask, image_features=feats, add_ner_ffn=self.gen_kw.get("add_ner_ffn", True), **kw)
            ev = torch.cuda.Event()
            ev.record(self.s_enc)
        ent["stage"], ent["b"] = stage, ev

    def __call__(self, batches):
        """yields (batch, generated ids) in order"""
        main = torch.cuda.current_stream()
        it = iter(batches)

        def fetch():
            b = next(it, None)
            if b is None:
                return None
            ready = torch.cuda.Event()
            ready.record(main)                              # the caller's host-to-device copies of this batch were enqueued on `main`
            return self._inputs(b, ready)

        cur = fetch()
        if cur is None:
            return
        self._encode(cur, None)
        nxt = fetch()
        while cur is not None:
            main.wait_event(cur["b"])
            src, src_mask, feats, kw = cur["inputs"]
            ahead = {}

            def advance(copied):
                # the next caption's encoder side may overwrite the stage once this caption's copy out of it is enqueued (`copied`);
                # the caption after that gets its image tower
                if nxt is not None:
                    self._encode(nxt, copied)
                    ahead["e"] = fetch()

            if cur["stage"] is not None:
                def hook():
                    ev = torch.cuda.Event()
                    ev.record(main)
                    advance(ev)
                gen = self.model.generate(input_ids=src, attention_mask=src_mask, num_beams=self.nb, encoded=cur["stage"], _after_begin=hook,
                                          **self.gen_kw)
            else:
                advance(None)
                gen = self.model.generate(input_ids=src, attention_mask=src_mask, num_beams=self.nb, image_features=feats, **kw, **self.gen_kw)
            yield cur["batch"], gen
            cur, nxt = nxt, ahead.get("e")


@torch.no_grad()
def generate(model, input_ids=None, attention_mask=None, num_beams=1, max_length=20, length_penalty=1.0, early_stopping=False,
             no_repeat_ngram_size=0, min_length=0, forced_eos_token_id="config", forced_bos_token_id=None, image_features=None,
             face_features=None, face_mask=None, name_ids=None, name_mask=None, add_ner_ffn=True, use_graphs=True, device_beams=True,
             return_nbest=False, encoded=None, _after_begin=None, do_sample=False, temperature=1.0, top_k=0, top_p=1.0,
             num_return_sequences=1, seed=None, return_logprobs=False, repetition_penalty=1.0, bad_words_ids=None, num_beam_groups=1,
             diversity_penalty=0.0, **unused):
    """GenerationMixin.generate(do_sample=False) semantics of transformers 4.18 for this model (greedy = 1 beam).
    Returns int64 [B, L] starting with decoder_start_token_id, padded with pad_token_id.
    Keyword defaults are the LIBRARY defaults; the defaults a hub checkpoint's config.json adds on top (what the reference's
    `model.generate(num_beams, max_length)` inherits after from_pretrained, TRAIN:513-520) are config.HUB_GENERATION_DEFAULTS and
    are passed explicitly by the trainer-level callers (training.gen_caption_from_loader_bart, utils/test_mmbart_clip_ddp.py).
    return_nbest: also return, per batch item, the finalized n-best list [(length-normalised score, ids)], best first — what
    `num_return_sequences=num_beams, output_scores=True` exposes as sequences / sequences_scores (the bookkeeping of ALL beams).

    do_sample=True: GenerationMixin.sample instead (num_beams must be 1): logits processors, then temperature -> top_k -> top_p, then
    one draw per row and position, all in vacnic_sample_step (include/vacnic_hip.h has the exact rules).  Returns int64
    [B * num_return_sequences, L], row b * n + j = sample j of item b: start token, tokens, eos (drawn, or forced at
    max_length - 1), then pad; with return_logprobs also fp32 [B * n, L], the log-probability of every token under the distribution
    it was drawn from (0 at the start token and at padding).  seed: an int makes the call reproducible (same inputs, weights and
    seed: same tokens, eager or replayed); None derives one from torch.initial_seed() and a per-process call counter.  With
    do_sample=False these keywords are ignored.

    bad_words_ids (NoBadWordsLogitsProcessor of 4.18; every path): a list of token-id lists that must not be generated; [eos] is
    dropped, at most kernels.BAD_WORDS_MAX words of kernels.BAD_WORD_LEN tokens.  repetition_penalty (a finite number > 0, below 1
    rewards repetition; RepetitionPenaltyLogitsProcessor): on the raw logits with do_sample=True and with one beam, on the
    log-softmax scores with more beams, as HF's sample / greedy_search / beam_search apply it (include/vacnic_hip.h has the rules).

    num_beam_groups=G > 1, diversity_penalty: group (diverse) beam search, 4.18's group_beam_search with HammingDiversityLogitsProcessor:
    the beams of an item are G groups of num_beams / G, handled in order at every position; a token that f beams of the earlier groups
    chose in this position scores diversity_penalty * f less (include/vacnic_hip.h at vacnic_group_beam_step has the exact rules).  One
    n-best list per item, shared by its groups: return_nbest / nbest_to_sequences hand out the diverse candidates.  With G == 1 (the
    default; diversity_penalty must then be 0) the call is the one of before."""
    _check_group_args(num_beams, num_beam_groups, diversity_penalty, do_sample, encoded)
    if do_sample:
        _check_sampling_args(num_beams, encoded, temperature, top_k, top_p, num_return_sequences)
    bad_words = None
    if bad_words_ids is not None or not (type(repetition_penalty) in (int, float) and repetition_penalty == 1):
        bad_words = _check_processor_args(model, repetition_penalty, bad_words_ids)
    cfg = model.config
    if model.arena is None:
        raise RuntimeError("call model.finalize(device) first")
    was_training = model.training
    if was_training:
        model.eval()                              # (walks ~1000 modules: 1 ms — skipped when the model already is in eval mode)
    if do_sample:
        try:
            return _generate_sample(model, input_ids, attention_mask, max_length, no_repeat_ngram_size, min_length,
                                    cfg.eos_token_id if forced_eos_token_id == "config" else forced_eos_token_id, forced_bos_token_id,
                                    (image_features, name_ids, name_mask, face_features, face_mask), add_ner_ffn, use_graphs,
                                    temperature, top_k, top_p, num_return_sequences, seed, return_logprobs,
                                    repetition_penalty=repetition_penalty, bad_words=bad_words)
        finally:
            if was_training:
                model.train()
    eos, pad, start = cfg.eos_token_id, cfg.pad_token_id, cfg.decoder_start_token_id
    if forced_eos_token_id == "config":
        forced_eos_token_id = eos                     # BartConfig default forced_eos_token_id=2
    B = input_ids.shape[0]
    nb = num_beams
    R = B * nb
    dev = model.emb16_pad.device
    if encoded is not None:
        # the encoder side of this caption ran ahead on another stream (EncodeStage / CaptionPipeline): K/V and mask are staged
        if B != 1 or encoded.nb != nb:
            raise ValueError("generate(encoded=...): staged encoding is for one caption and the same beam count")
        enc_h, mask_u8, S, d = None, None, encoded.S, encoded.d
    else:
        mask_u8 = attention_mask.to(torch.uint8) if attention_mask.dtype != torch.uint8 else attention_mask
        enc_h = _run_encoder(model, use_graphs, add_ner_ffn, input_ids, mask_u8, image_features, name_ids, name_mask, face_features, face_mask)
        S, d = enc_h.shape[1], enc_h.shape[2]
    device_beams = bool(device_beams) and nb <= 16 and 2 * nb * nb <= 128 and max_length <= 512
    penalty = _f32(repetition_penalty)                   # the value the kernels see: 1 + 1e-12 is "off"
    groups = (num_beam_groups, _f32(diversity_penalty)) if num_beam_groups > 1 else None
    G = num_beam_groups
    gs = nb // G                                         # beams per group (all of them without groups)
    key = _decode_session_key(R, S, max_length, nb, no_repeat_ngram_size, min_length, forced_eos_token_id, forced_bos_token_id,
                              (float(length_penalty), bool(early_stopping)) if device_beams else None, bad_words, penalty, groups)
    processors = len(key) > _DECODE_KEY_LEN
    sessions = model.__dict__.setdefault("_decode_sessions", {})
    ses = sessions.get(key)
    if ses is not None and processors:
        sessions[key] = sessions.pop(key)                # most recently used last
    if ses is None:
        if processors:
            # the penalty is a free axis of the key: the least recently used processor session goes when a ninth arrives (the
            # sessions of the default key, which is the shape alone, stay as before)
            keyed = [k for k in sessions if len(k) > _DECODE_KEY_LEN]
            for k in keyed[:max(0, len(keyed) - _PROCESSOR_SESSIONS_MAX + 1)]:
                del sessions[k]
        ses = sessions[key] = DecodeSession(model, R, S, max_length, nb, no_repeat_ngram_size, min_length, forced_eos_token_id, eos,
                                            forced_bos=forced_bos_token_id, bad_words=bad_words, penalty=penalty, groups=groups)
        if device_beams:
            ses.enable_device_beams(B, length_penalty, early_stopping, pad)
    if encoded is not None:
        ses.dec.begin_staged(encoded)
    else:
        ses.dec.begin(enc_h, mask_u8, nb)
    if _after_begin is not None:
        _after_begin()                                 # CaptionPipeline: the next caption's encoder side goes out before this beam search
    if device_beams:
        # on-device bookkeeping: the positions are enqueued back to back; ONE device->host copy of the final state
        try:
            cur_len, seqs_t, scores_t, done_t, hcnt, hscore, hlen, hseq = ses.run_device(start, use_graphs)
        except Exception:
            sessions.pop(key, None)                      # its graphs / buffers may hold a half-finished caption
            if was_training:
                model.train()
            raise
        ses.captions += 1
        out, nbest = [], []
        for b in range(B):
            hy = _BeamHyps(nb, length_penalty, early_stopping)
            for i in range(int(hcnt[b])):
                hy.beams.append((float(hscore[b, i]), hseq[b, i, :int(hlen[b, i])].tolist()))
            if hy.beams:
                hy.worst = min(sc for sc, _ in hy.beams)
            if not bool(done_t[b]):
                for j in range(nb):                       # BeamSearchScorer.finalize: open beams join the n-best list
                    hy.add(seqs_t[b * nb + j, :cur_len].tolist(), float(scores_t[b * nb + j]))
            ranked = sorted(hy.beams, key=lambda x: x[0])
            out.append(ranked[-1][1])
            nbest.append([(float(sc), list(sq)) for sc, sq in reversed(ranked)])
        L = min(max(len(o) for o in out) + 1, max_length)
        res = torch.full((B, L), pad, dtype=torch.long)
        for b, o in enumerate(out):
            res[b, :len(o)] = torch.tensor(o)
            if len(o) < L:
                res[b, len(o)] = eos
        if was_training:
            model.train()
        return (res.to(dev), nbest) if return_nbest else res.to(dev)

    seqs = [[start] for _ in range(R)]
    beam_scores = [0.0 if (r % gs) == 0 else -1e9 for r in range(R)]    # the first beam of every group is live
    hyps = [_BeamHyps(nb, length_penalty, early_stopping) for _ in range(B)]
    done = [False] * B
    cur_len = 1
    Kc = 2 * gs
    lam = groups[1] if groups else 0.0
    pen_scores = penalty if ses.pen_rule == "scores" else 1.0
    new_src = list(range(R))
    while True:
        t = cur_len - 1
        bans = [_banned(s_, no_repeat_ngram_size) for s_ in seqs] if no_repeat_ngram_size > 0 else None
        if bad_words:
            bans = [(bans[r] if bans else []) + _bad_word_bans(s_, bad_words) for r, s_ in enumerate(seqs)]
        try:
            tv, ti = ses.step(t, [s_[-1] for s_ in seqs], beam_scores, new_src, bans, use_graphs, seqs=seqs if ses.pen_rule else None)
        except Exception:
            sessions.pop(key, None)
            if was_training:
                model.train()
            raise
        tv, ti = tv.tolist(), ti.tolist()
        new_seqs, new_scores, new_src = [], [], []
        hamming = groups is not None and ses.forced_at(cur_len) < 0      # a forced position overwrites the Hamming term (HF's order)
        for b, g in ((b, g) for b in range(B) for g in range(G)):
            # the groups of an item in order (one group = ordinary beam search); new_tok: the tokens its earlier groups chose here
            r0 = b * nb + g * gs
            if g == 0:
                new_tok = []
            if done[b]:                                                 # on entry, or by an earlier group of this position
                new_seqs += [seqs[r0] + [pad]] * gs; new_scores += [0.0] * gs; new_src += [r0] * gs
                continue
            # merge the per-beam top-2k lists into the group's top-2k (HF: topk over the [gs*V] scores of the group)
            cand = []
            for j in range(gs):
                row_v, row_i = tv[r0 + j], ti[r0 + j]
                for c in range(len(row_v)):
                    if row_i[c] >= 0:
                        sc = row_v[c]
                        f = new_tok.count(row_i[c]) if (hamming and g > 0) else 0
                        if f > 0:
                            # vacnic_group_beam_step's Hamming term, rounded as the kernel rounds it: lambda f [P inside the history]
                            h = _f32(lam * f)
                            if pen_scores != 1.0 and row_i[c] in seqs[r0 + j]:
                                h = _f32(h * pen_scores)
                            sc = _f32(sc - h)
                        cand.append((sc, j, row_i[c]))
            cand.sort(key=lambda x: (-x[0], x[1] * model.V + x[2]))
            cand = cand[:Kc]
            chosen = []
            for rank, (sc, j, tok) in enumerate(cand):
                src = r0 + j
                if tok == eos:
                    if rank >= gs:
                        continue
                    hyps[b].add(seqs[src], sc)
                else:
                    chosen.append((sc, tok, src))
                if len(chosen) == gs:
                    break
            done[b] = done[b] or hyps[b].is_done(cand[0][0], cur_len)
            while len(chosen) < gs:                                     # cannot happen with 2*gs candidates; keep shapes sane
                chosen.append((-1e9, pad, r0))
            for sc, tok, src in chosen:
                new_seqs.append(seqs[src] + [tok]); new_scores.append(sc); new_src.append(src); new_tok.append(tok)
        seqs = new_seqs
        beam_scores = new_scores
        cur_len += 1
        if all(done) or cur_len >= max_length:
            break
    ses.captions += 1
    out, nbest = [], []
    for b in range(B):
        if not done[b]:
            for j in range(nb):
                hyps[b].add(seqs[b * nb + j], float(beam_scores[b * nb + j]))
        ranked = sorted(hyps[b].beams, key=lambda x: x[0])
        out.append(ranked[-1][1])
        nbest.append([(float(sc), list(sq)) for sc, sq in reversed(ranked)])
    L = min(max(len(o) for o in out) + 1, max_length)
    res = torch.full((B, L), pad, dtype=torch.long)
    for b, o in enumerate(out):
        res[b, :len(o)] = torch.tensor(o)
        if len(o) < L:
            res[b, len(o)] = eos
    if was_training:
        model.train()
    return (res.to(dev), nbest) if return_nbest else res.to(dev)
