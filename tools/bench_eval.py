"""Validation pass with and without the fused validation head on 1x MI355X: BART-large + ViT-L/14, B = 32, S = 512, T = 64,
synthetic GoodNews-shaped batches.  Two comparisons on the same device batches, the two paths alternating inside every round so
that drift hits both (median [min .. max] over the rounds; the spread of a path is its max - min):
  forward   model(labels, output_logits=True) + argmax_rows (what eval_epoch runs per batch) against
            model(labels, output_token_stats=True) (what eval_epoch_fused runs per batch); device events, frozen-tower features
            computed once outside the window.
  pass      eval_epoch(model, batches) against eval_epoch_fused(model, batches): host clock around the whole pass, which ends in
            its own device-to-host copies (3 waits per batch against 2 per pass).
Per-kernel times: `rocprofv3 --kernel-trace --stats -- python tools/bench_eval.py --rounds 1 --iters 2 --batches 1`."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vacnic_amd import kernels as K, synthetic
from vacnic_amd.config import bart_large_vit_l14
from vacnic_amd.training import _model_inputs, build_models, eval_epoch, eval_epoch_fused, to_device


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="forwards per round and path")
    ap.add_argument("--batches", type=int, default=4, help="batches per validation pass")
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    cfg, vcfg = bart_large_vit_l14()
    model, _, _ = build_models(cfg, vcfg, device="cuda", seed=42, init="device", with_guide=False)
    model.eval()
    batches = [to_device(synthetic.make_batch(cfg, a.batch, S=512, T=64, seed=42, step=i, image_size=vcfg.image_size), "cuda")
               for i in range(a.batches)]
    b = batches[0]
    tgt = b["caption_ids"]
    with torch.no_grad():
        src, src_mask, feats, kw = _model_inputs(model, b)
        _, tgt_in = K.prep_ids(tgt, cfg.pad_token_id, start_id=cfg.eos_token_id)
    inputs = dict(input_ids=src, attention_mask=src_mask, decoder_input_ids=tgt_in, image_features=feats, labels=tgt, add_ner_ffn=True, **kw)

    def old():
        out = model(output_logits=True, label_smoothing=0.0, **inputs)
        lg = out["logits"]
        return out["loss"], K.argmax_rows(lg.view(-1, lg.shape[-1]), model.V).view(tgt.shape)

    def new():
        out = model(output_token_stats=True, **inputs)
        return out["loss"], out["token_stats"]["pred_ids"]

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.iters

    def walled(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(model, batches)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.batches

    with torch.no_grad():
        (l0, p0), (l1, p1) = old(), new()
        torch.cuda.synchronize()
        agree = (p0 == p1).float().mean().item()
        for fn in (old, new):
            timed(fn)                                  # warm
        walled(eval_epoch); walled(eval_epoch_fused)
        t = {"forward": {"eval_epoch": [], "eval_epoch_fused": []}, "pass": {"eval_epoch": [], "eval_epoch_fused": []}}
        for _ in range(a.rounds):
            t["forward"]["eval_epoch"].append(timed(old))
            t["forward"]["eval_epoch_fused"].append(timed(new))
            t["pass"]["eval_epoch"].append(walled(eval_epoch))
            t["pass"]["eval_epoch_fused"].append(walled(eval_epoch_fused))
    print(f"B={a.batch} S=512 T=64 bart-large + ViT-L/14; {a.rounds} rounds, alternating; ms per batch, median [min .. max]")
    print(f"loss {l0.item():.6f} (eval_epoch) {l1.item():.6f} (fused); predicted ids agree on {100 * agree:.2f} % of positions")
    rec = {}
    for what, paths in t.items():
        m = {k: statistics.median(v) for k, v in paths.items()}
        spread = max(max(v) - min(v) for v in paths.values())
        for k, v in paths.items():
            print(f"{what:8s} {k:18s} {m[k]:9.3f} [{min(v):.3f} .. {max(v):.3f}]")
        gain = m["eval_epoch"] - m["eval_epoch_fused"]
        print(f"{what:8s} fused is {gain:+.3f} ms per batch ({100 * gain / m['eval_epoch']:+.1f} %) against a spread of {spread:.3f} ms: "
              f"{'faster by more than the spread' if gain > spread else 'NOT faster by more than the spread'}")
        rec[what] = {"eval_epoch_ms": round(m["eval_epoch"], 3), "eval_epoch_fused_ms": round(m["eval_epoch_fused"], 3), "spread_ms": round(spread, 3)}
    rec["host_waits_per_pass"] = {"eval_epoch": 3 * a.batches, "eval_epoch_fused": 2}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
