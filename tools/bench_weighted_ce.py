"""Cost of per-row loss weights on the fused LM head at the benchmark's size (R = B T = 32 x 64 = 2048, V = 50267, d = 1024): the
forward and the whole backward chunk loop of ops.lm_head_ce, unweighted and weighted ALTERNATING in one process, so that both see
the same clocks and the same neighbours on the box.

    python tools/bench_weighted_ce.py [--rounds 12] [--iters 10] [--deterministic]

Per round and variant: `iters` forward + backward passes between two device events, after a warm-up of both variants.  Reported:
median, min and max over the rounds per variant, the median of the per-round differences (weighted - unweighted, same round), and
the unweighted variant's own run-to-run spread — a difference inside that spread is not a measured difference.  What the weighted
path adds by construction: three R-float vectors written, two of them read back by a one-block sum, two small launches in the
forward (vacnic_lmhead_ce_wloss), none in the backward (vacnic_lmhead_ce_rowp_w replaces vacnic_lmhead_ce_rowp).
One JSON line at the end.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vacnic_amd import kernels as K
from vacnic_amd import ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--cap", type=int, default=64, help="rows per caption (per-caption weights)")
    ap.add_argument("--deterministic", action="store_true", help="both variants in ops.set_deterministic mode")
    a = ap.parse_args()
    dev = "cuda"
    R, V, d, T = a.rows, 50267, 1024, a.cap
    Vp = (V + 31) // 32 * 32
    g = torch.Generator(device="cpu").manual_seed(0)
    h = (torch.randn(R, d, generator=g) * 0.5).to(dev).bfloat16()
    E = torch.zeros(Vp, d, device=dev, dtype=torch.bfloat16)
    E[:V] = (torch.randn(V, d, generator=g) * 0.05).to(dev).bfloat16()
    tgt = torch.randint(3, V, (R,), generator=g).to(dev)
    tgt[::7] = 1
    w_cap = torch.randn(R // T, generator=g).to(dev)
    egrad = torch.zeros(Vp, d, device=dev)
    one = ops.const_one(torch.device(dev))
    ops.set_deterministic(a.deterministic)

    def step(weights, rpw):
        hh = h.detach().requires_grad_(True)
        out = ops.lm_head_ce(hh, None, E, egrad, tgt, V, 1, weights=weights, rows_per_weight=rpw)
        out[0].backward(one)
        ops.flush_wgrads()

    variants = {"unweighted": (None, 1), "weighted_per_caption": (w_cap, T),
                "weighted_per_token": (w_cap.repeat_interleave(T).contiguous(), 1)}
    for wts, rpw in variants.values():                       # warm-up: code objects, allocator, the GEMM's workspaces
        for _ in range(3):
            step(wts, rpw)
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for name, (wts, rpw) in variants.items():            # alternate inside the round
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.iters):
                step(wts, rpw)
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / a.iters * 1e3)        # us per forward + backward
    res = {"what": f"ops.lm_head_ce forward + backward, R={R} V={V} d={d}, us per pass, {a.rounds} rounds x {a.iters} passes, alternating",
           "deterministic": bool(a.deterministic)}
    base = times["unweighted"]
    for name, t in times.items():
        print(f"{name:22s} median {statistics.median(t):9.1f} us   min {min(t):9.1f}   max {max(t):9.1f}")
        res[name] = {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
        if name != "unweighted":
            diff = [x - b for x, b in zip(t, base)]
            res[name]["median_diff_us"] = round(statistics.median(diff), 1)
            print(f"{'':22s} weighted - unweighted, same round: median {statistics.median(diff):+8.1f} us   min {min(diff):+8.1f}   max {max(diff):+8.1f}")
    res["unweighted_spread_us"] = round(max(base) - min(base), 1)
    print(f"run-to-run spread of the unweighted variant (max - min over the rounds): {max(base) - min(base):.1f} us")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
