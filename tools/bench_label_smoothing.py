"""Cost of label smoothing in the fused LM head + cross entropy at configs[1] size (R = 2048, V = 50265, d = 1024): the forward call
(GEMM with the statistics epilogue + combine) and one 16384-column dlogits chunk, label_smoothing = 0.1 against 0.0 on the same
device.  Event timing; the two variants alternate inside every round so that drift hits both; the median over the rounds is reported.
Per-kernel times: run this under `rocprofv3 --kernel-trace --stats -- python tools/bench_label_smoothing.py --rounds 1`."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vacnic_amd import kernels as K


def timed(fn, iters):
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--eps", type=float, default=0.1)
    a = ap.parse_args()
    dev = "cuda"
    R, V, d, CH = 2048, 50265, 1024, 16384
    Vp = (V + 31) // 32 * 32
    h = (torch.randn(R, d, device=dev) * 0.5).bfloat16()
    E = torch.zeros(Vp, d, device=dev, dtype=torch.bfloat16); E[:V] = (torch.randn(V, d, device=dev) * 0.05).bfloat16()
    tgt = torch.randint(3, V, (R,), device=dev)
    dl = torch.empty(R, CH, device=dev, dtype=torch.bfloat16)
    cases = {}
    for eps in (0.0, a.eps):
        lse, acc = K.lmhead_ce_fwd(h, E, tgt, V, label_smoothing=eps)
        rowp = K.lmhead_ce_rowp(lse, tgt, acc, label_smoothing=eps, V=V)
        cases[eps] = {"fused forward (GEMM + combine)": lambda eps=eps: K.lmhead_ce_fwd(h, E, tgt, V, label_smoothing=eps),
                      "dlogits chunk of 16384": lambda eps=eps, rowp=rowp: K.lmhead_ce_dlogits(h, E, tgt, V, rowp, dl, 0, CH, label_smoothing=eps),
                      "rowp": lambda eps=eps, lse=lse, acc=acc: K.lmhead_ce_rowp(lse, tgt, acc, label_smoothing=eps, V=V)}
    print(f"R={R} V={V} d={d}; {a.rounds} rounds x {a.iters} launches per variant, alternating; median [min .. max] in us")
    for name in cases[0.0]:
        for eps in cases:
            timed(cases[eps][name], 20)             # warm
        t = {eps: [] for eps in cases}
        for _ in range(a.rounds):
            for eps in cases:
                t[eps].append(timed(cases[eps][name], a.iters))
        m0, m1 = statistics.median(t[0.0]), statistics.median(t[a.eps])
        print(f"{name:32s} eps=0: {m0:8.1f} [{min(t[0.0]):.1f} .. {max(t[0.0]):.1f}]   eps={a.eps}: {m1:8.1f} [{min(t[a.eps]):.1f} .. {max(t[a.eps]):.1f}]"
              f"   {100 * (m1 / m0 - 1):+.1f} %")


if __name__ == "__main__":
    main()
