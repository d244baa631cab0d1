"""BASELINE config 5: captions/sec on 1x MI355X — BART-large + ViT-L/14 full model, batch 1 (test_batch_size 1,
run_full_train.sh:10), beam 5, max_length 50, length_penalty 2.0, seed 42; synthetic GoodNews-shaped inputs.

    bench_generate.py [n] [batch] [--num_beams N] [--do_sample [--top_k K] [--top_p P] [--temperature T] [--num_return_sequences N]]
                      [--repetition_penalty P] [--bad_words 3,4;50264] [--num_beam_groups G --diversity_penalty L]

--do_sample times sampling decode at the same shape (one beam; rows = batch x num_return_sequences); --num_beams 1 is the greedy
decode it goes beside.  --repetition_penalty / --bad_words (comma-separated ids, `;` between words) switch the two logits
processors on; without them the calls are the ones of before.  --num_beam_groups / --diversity_penalty: group (diverse) beam search
(G has to divide --num_beams); one group is the beam search of before.

    bench_generate.py --kernel [--rows 1,8] [--vocab 50265]

times vacnic_sample_step alone (no model): 50 launches on fp32 logits ~ normal(0, 2) captured in one hipGraph, per setting and row
count, and beside them the LM-head GEMM that writes those logits (d_model 1024); one JSON line with microseconds per launch."""
import argparse
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vacnic_amd import kernels as K, synthetic
from vacnic_amd.config import bart_large_vit_l14
from vacnic_amd.models.clip_vit import extract_clip_img_feat, graphed_clip_img_feat
from vacnic_amd.training import build_models, to_device


def graph_us_per_launch(launch, launches=50, replays=20):
    """median over `replays` of (time of one hipGraph holding launch(0) .. launch(launches - 1)) / launches, in microseconds"""
    launch(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with K.capture_scope(("bench-generate", id(g))), torch.cuda.graph(g):
        for i in range(launches):
            launch(i)
    for _ in range(3):
        g.replay()
    times = []
    for _ in range(replays):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); g.replay(); b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / launches)
    return round(sorted(times)[len(times) // 2], 1)


def kernel_mode(rows, V, d=1024, launches=50):
    """vacnic_sample_step by itself.  eos is suppressed so that no row finishes (a finished row only writes pad); every launch is
    a position of its own (cur_len 1 .. launches) on the same logits."""
    V_pad = (V + 15) // 16 * 16 + (16 if V % 16 == 0 else 0)         # ldl > V, as CachedDecoder.step hands the logits over
    settings = {"temperature only": (1.0, 0, 1.0), "top_k 50": (1.0, 50, 1.0), "top_p 0.9": (1.0, 0, 0.9),
                "T 0.8 + top_k 50 + top_p 0.9": (0.8, 50, 0.9)}
    gen = torch.Generator(device="cuda").manual_seed(42)
    w = (torch.randn((V_pad, d), device="cuda", generator=gen) * 0.02).to(torch.bfloat16)
    bias = torch.zeros(V_pad, device="cuda")
    res = {}
    for R in rows:
        logits = torch.randn((R, V_pad), device="cuda", generator=gen) * 2.0
        seq = torch.ones((R, launches + 1), device="cuda", dtype=torch.int32)
        logp = torch.zeros((R, launches + 1), device="cuda")
        done = torch.zeros(R, device="cuda", dtype=torch.int32)
        nxt = torch.zeros(R, device="cuda", dtype=torch.long)
        out = {}
        for name, (T, k, p) in settings.items():
            params = K.sample_params(T, k, p, seed=42).cuda()
            out[name] = graph_us_per_launch(lambda i: K.sample_step(logits, V, params, seq, done, nxt, i + 1, logp=logp, suppress_eos=True),
                                            launches)
        assert int(done.sum()) == 0
        h = torch.randn((R, d), device="cuda", generator=gen).to(torch.bfloat16)
        out["LM-head GEMM -> fp32 logits"] = graph_us_per_launch(
            lambda i: K.gemm(h, w, R, V, d, bias=bias, out=logits, ldo=V_pad, out_mode=1), launches)
        res[f"R={R}"] = out
    print(json.dumps({"metric": f"vacnic_sample_step alone, V {V}, ldl {V_pad}, {launches} launches per hipGraph", "unit": "us per launch",
                      "value": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--vocab", type=int, default=50265)
    ap.add_argument("n", nargs="?", type=int, default=8)
    ap.add_argument("batch", nargs="?", type=int, default=1)    # 1 = BASELINE configs[4]; >1 = batched decode service (the reference never batches)
    ap.add_argument("--num_beams", type=int, default=5)
    ap.add_argument("--do_sample", action="store_true")
    ap.add_argument("--top_k", type=int, default=0)
    ap.add_argument("--top_p", type=float, default=1.0)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--num_return_sequences", type=int, default=1)
    ap.add_argument("--repetition_penalty", type=float, default=1.0)
    ap.add_argument("--bad_words", default="")
    ap.add_argument("--num_beam_groups", type=int, default=1)
    ap.add_argument("--diversity_penalty", type=float, default=0.0)
    a = ap.parse_args()
    if a.kernel:
        return kernel_mode([int(r) for r in a.rows.split(",")], a.vocab)
    n, bsz = a.n, a.batch
    if a.do_sample:
        mode = dict(do_sample=True, num_beams=1, top_k=a.top_k, top_p=a.top_p, temperature=a.temperature,
                    num_return_sequences=a.num_return_sequences, seed=42)
        what = f"sampling (T {a.temperature}, top_k {a.top_k}, top_p {a.top_p}, {a.num_return_sequences} per caption)"
    else:
        mode = dict(num_beams=a.num_beams, length_penalty=2.0)
        what = f"beam {a.num_beams}"
    if a.num_beam_groups != 1 or a.diversity_penalty != 0.0:
        mode.update(num_beam_groups=a.num_beam_groups, diversity_penalty=a.diversity_penalty)
        what += f", {a.num_beam_groups} groups, diversity_penalty {a.diversity_penalty}"
    if a.repetition_penalty != 1.0:
        mode["repetition_penalty"] = a.repetition_penalty
        what += f", repetition_penalty {a.repetition_penalty}"
    if a.bad_words:
        mode["bad_words_ids"] = [[int(t) for t in w.split(",")] for w in a.bad_words.split(";")]
        what += f", {len(mode['bad_words_ids'])} bad words"
    cfg, vcfg = bart_large_vit_l14()
    model, _, clip_model = build_models(cfg, vcfg, device="cuda", seed=42, init="device")
    model.eval()
    times = []
    for i in range(n + 2):
        b = to_device(synthetic.make_batch(cfg, bsz, S=512, T=64, seed=42, step=i, full_length=True), "cuda")
        torch.cuda.synchronize(); t0 = time.perf_counter()
        mask, _ = K.prep_ids(b["article_ids"], 1)
        nmask, _ = K.prep_ids(b["names_art_ids"], 1)
        _, cls = graphed_clip_img_feat(clip_model)(b["img_tensor"])
        out = model.generate(input_ids=b["article_ids"], attention_mask=mask, max_length=50, **mode,
                             min_length=49,      # random-init weights emit EOS at once; force full-length captions (worst case)
                             image_features=cls, face_features=b["face_emb"], face_mask=K.face_mask(b["face_emb"]),
                             name_ids=b["names_art_ids"], name_mask=nmask, add_ner_ffn=True)
        torch.cuda.synchronize()
        if i >= 2:
            times.append(time.perf_counter() - t0)
    t = sum(times) / len(times)
    rows = int(out.shape[0])
    print(json.dumps({"metric": f"captions/sec, {what}, max_length 50" + (", length_penalty 2.0" if not a.do_sample else "")
                      + (", batch 1 (BASELINE configs[4])" if bsz == 1 else f", batch {bsz} (batched decode service)"),
                      "value": round(bsz / t, 3), "unit": "captions/s", "batch": bsz, "ms_per_batch": round(t * 1e3, 1), "tokens": int(out.shape[1]),
                      "ms_per_token": round(t * 1e3 / out.shape[1], 2), "us_per_position": round(t * 1e6 / (out.shape[1] - 1), 1),
                      "rows": rows, "tokens_per_sec": round(rows * (out.shape[1] - 1) / t, 1), "n": len(times), "data": "synthetic",
                      "dtype": "bf16"}))


if __name__ == "__main__":
    main()
