"""AdamW kernel alone on a BART-large-sized arena (HBM-bound: 16 B read + 14 B written per parameter).

    python tools/bench_adamw.py [--part all|accum] [--parent-lib DIR/libvacnic_hip.so]

accum: only the gradient-accumulation rows (the last section); --parent-lib: the library built from the parent commit, whose
vacnic_adamw is timed beside them in the same run."""
import argparse
import ctypes as C
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vacnic_amd import kernels as K
_ap = argparse.ArgumentParser()
_ap.add_argument("--part", choices=("all", "accum"), default="all")
_ap.add_argument("--parent-lib", default="", help="libvacnic_hip.so built from the parent commit")
ARGS = _ap.parse_args()
n = 420 * 1024 * 1024
p = torch.randn(n, device="cuda"); g = torch.randn(n, device="cuda") * 1e-3
m = torch.zeros(n, device="cuda"); v = torch.zeros(n, device="cuda"); p16 = torch.empty(n, device="cuda", dtype=torch.bfloat16)
hyper = torch.tensor([3e-5, 1.0], device="cuda")


def accum_rows():
    """Gradient accumulation (vacnic_lr_step_accum, FusedAdamW(accum_steps=4)): what one micro-batch's optimizer phase costs.
    A HOLD launch is the wide AdamW grid reading the step word and leaving (up to 65536 workgroups that do nothing else); an APPLY
    launch is the ungrouped kernel behind one more loaded word.  Both are timed as the phase FusedAdamW.step() issues, lr_step_accum +
    adamw(skip=accum), with the counter preset so that every launch of a row is of one kind; beside them the existing row, lr_step +
    adamw(skip=None), and with --parent-lib the same phase through the parent commit's library.  Rows alternate; the yardstick is the
    spread of the existing row's own repeats."""
    K4 = 4
    accum = K.accum_state("cuda")
    hold_word = torch.tensor([2, 0, 0, 0], device="cuda")

    def existing():
        K.lr_step(hyper, 3e-5, 0.0, 1e9)
        K.adamw(p, g, m, v, p16, hyper, n, zero_grad=True)

    def apply_():                               # pending = k - 1 before every call: each one completes a group
        accum[1:2].fill_(K4 - 1)                # (one 8-byte fill kernel inside the timed window)
        K.lr_step_accum(hyper, 3e-5, 0.0, 1e9, accum, K4)
        K.adamw(p, g, m, v, p16, hyper, n, grad_scale=1.0 / K4, zero_grad=True, skip=accum)

    def hold():                                 # pending = 0 before every call: each one is a group's first micro-batch
        accum[1:2].fill_(0)
        K.lr_step_accum(hyper, 3e-5, 0.0, 1e9, accum, K4)
        K.adamw(p, g, m, v, p16, hyper, n, grad_scale=1.0 / K4, zero_grad=True, skip=accum)

    variants = [("existing: lr_step + adamw(skip=None)", existing),
                ("accum_steps=4 apply: fill + lr_step_accum + adamw(skip=accum)", apply_),
                ("accum_steps=4 hold:  fill + lr_step_accum + adamw(skip=accum)", hold),
                ("hold, adamw launch alone (step word preset to 2)", lambda: K.adamw(p, g, m, v, p16, hyper, n, zero_grad=True, skip=hold_word))]
    if ARGS.parent_lib:
        lib = C.CDLL(ARGS.parent_lib)
        vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
        PArgs = type("parent_adamw_args", (C.Structure,), {"_fields_": [
            ("p", vp), ("g", vp), ("m", vp), ("v", vp), ("p_bf16", vp), ("hyper", vp), ("n", i64), ("beta1", f32), ("beta2", f32),
            ("eps", f32), ("weight_decay", f32), ("grad_scale", f32), ("zero_grad", i32), ("clip_coef", vp), ("skip", vp)]})
        lib.vacnic_adamw.argtypes = [C.POINTER(PArgs), vp]
        lib.vacnic_lr_step.argtypes = [vp, f32, f32, f32, vp, vp]

        def parent():
            s = K._stream()
            rc = lib.vacnic_lr_step(hyper.data_ptr(), 3e-5, 0.0, 1e9, None, s)
            a = PArgs(p=p.data_ptr(), g=g.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), p_bf16=p16.data_ptr(), hyper=hyper.data_ptr(), n=n,
                      beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0, zero_grad=1, clip_coef=None, skip=None)
            rc |= lib.vacnic_adamw(C.byref(a), s)
            if rc != 0:
                raise RuntimeError("parent library call failed")
        variants.append(("parent library: lr_step + adamw(skip=None)", parent))
    rows = {name: [] for name, _ in variants}
    for rep in range(5):
        for name, fn in variants:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                fn()
            e1.record(); torch.cuda.synchronize()
            rows[name].append(e0.elapsed_time(e1) / 10)
            print(f"accum row {rep}: {name}: {rows[name][-1]:.4f} ms (10 launches)")
    assert accum[0].item() == 2 and accum[1].item() == 1, "the last timed variant with the counter was a hold"
    b = rows[variants[0][0]]
    base = sum(b) / len(b)
    print(f"arena of {n / 1e6:.0f}M elements; existing row: mean {base:.4f} ms, spread of its own rows {max(b) - min(b):.4f} ms")
    for name, _ in variants[1:]:
        r = rows[name]
        mean = sum(r) / len(r)
        print(f"  {name}: mean {mean:.4f} ms, spread {max(r) - min(r):.4f} ms = {mean - base:+.4f} ms against the existing row "
              f"({mean / base:.4f} x)")


if ARGS.part == "accum":
    accum_rows()
    sys.exit(0)
for clip in (None, torch.ones(2, device="cuda")):
    for _ in range(3):
        K.adamw(p, g, m, v, p16, hyper, n, zero_grad=False, clip_coef=clip)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        K.adamw(p, g, m, v, p16, hyper, n, zero_grad=True, clip_coef=clip)
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 10
    print(f"clip={'on' if clip is not None else 'off'}: {ms:.3f} ms for {n/1e6:.0f}M params = {n*34/ms/1e9:.2f} TB/s (34 B/param incl. grad zeroing)")
out = K.grad_clip_coef(g, n, 0.1)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(10):
    K.grad_clip_coef(g, n, 0.1, out=out)
e1.record(); torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / 10
print(f"grad_clip_coef: {ms:.3f} ms = {n*4/ms/1e9:.2f} TB/s")

# ---- parameter groups (vacnic_adamw_groups): the same arena through the grouped kernel, in the same process, rows alternating.
# Yardstick: the ungrouped rows; margin: the spread between their own repeats.
from vacnic_amd.arena import no_decay_spec, table_from_segments
from vacnic_amd.config import bart_large_vit_l14
from vacnic_amd.models.mmbart import BartForMultiModalGeneration
cfg, _ = bart_large_vit_l14()
with torch.device("meta"):                 # layout only: names, shapes and arena slots of the real model, no weights
    net = BartForMultiModalGeneration(cfg, enc_fusion_layer=cfg.enc_fusion_layer, dim_common=cfg.dim_common, prompt_size=cfg.prompt_size)
net.finalize("meta")
spec = [{"match": "embed_positions", "frozen": True}] + no_decay_spec(net)
full = net.arena.group_table(net.named_parameters(), spec, 0.01).segments()
segs = [(s, lr, wd, fr) for s, _, lr, wd, fr in full if s < n]          # the model's arena is larger than the bench arena: its first n elements
real = table_from_segments(n, segs).to("cuda")
one = table_from_segments(n, [(0, 1.0, 0.01, False)]).to("cuda")
print(f"BART-large VACNIC arena: {net.arena.n / 1e6:.0f}M elements, {len(full)} segments; bench table: {real.nseg} segments over the first "
      f"{n / 1e6:.0f}M elements, {sum(fr for *_, fr in segs)} frozen")
variants = [("ungrouped K.adamw", lambda: K.adamw(p, g, m, v, p16, hyper, n, zero_grad=True)),
            ("grouped, 1 segment", lambda: K.adamw_groups(p, g, m, v, p16, hyper, n, one, zero_grad=True)),
            (f"grouped, {real.nseg} segments", lambda: K.adamw_groups(p, g, m, v, p16, hyper, n, real, zero_grad=True)),
            ("grad_clip_coef", lambda: K.grad_clip_coef(g, n, 0.1, out=out)),
            (f"grad_clip_coef_groups, {real.nseg} segments", lambda: K.grad_clip_coef_groups(g, n, 0.1, real, out=out))]
rows = {name: [] for name, _ in variants}
for rep in range(3):
    for name, fn in variants:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            fn()
        e1.record(); torch.cuda.synchronize()
        rows[name].append(e0.elapsed_time(e1) / 10)
        print(f"row {rep}: {name}: {rows[name][-1]:.3f} ms (10 launches)")
for base, names in (("ungrouped K.adamw", [v[0] for v in variants[1:3]]), ("grad_clip_coef", [variants[4][0]])):
    b = rows[base]
    mean = sum(b) / len(b)
    print(f"{base}: mean {mean:.3f} ms, spread of its own rows {max(b) - min(b):.3f} ms")
    for name in names:
        r = rows[name]
        print(f"  {name}: mean {sum(r) / len(r):.3f} ms = {sum(r) / len(r) - mean:+.3f} ms against it (rows {', '.join(f'{x:.3f}' for x in r)})")

# ---- moving average of the weights (vacnic_adamw_ema): the same arena with the average kept in the AdamW pass, grouped and
# ungrouped, beside the plain kernels and beside "plain kernel + a separate pass over p and the average" (torch's lerp_: one
# elementwise kernel, 8 B read + 4 B written per parameter), rows alternating as above.
# Traffic model, bytes per parameter: plain 16 read (p, g, m, v) + 18 written (p, m, v, zeroed g, bf16 shadow) = 34;
# fused average +4 read +4 written = 42; separate pass 34 + 12 = 46 and one more launch.
ema = p.clone()
D = 0.999
ema_variants = [("ungrouped K.adamw", 34, lambda: K.adamw(p, g, m, v, p16, hyper, n, zero_grad=True)),
                ("ungrouped K.adamw_ema", 42, lambda: K.adamw_ema(p, g, m, v, p16, hyper, n, ema, D, zero_grad=True)),
                ("ungrouped K.adamw + separate lerp_ pass", 46, lambda: (K.adamw(p, g, m, v, p16, hyper, n, zero_grad=True), ema.lerp_(p, 1.0 - D))),
                (f"grouped, {real.nseg} segments", 34, lambda: K.adamw_groups(p, g, m, v, p16, hyper, n, real, zero_grad=True)),
                (f"grouped K.adamw_ema, {real.nseg} segments", 42, lambda: K.adamw_ema(p, g, m, v, p16, hyper, n, ema, D, table=real, zero_grad=True)),
                ("ema_swap", 18, lambda: K.ema_swap(p, ema, p16))]
rows = {name: [] for name, _, _ in ema_variants}
for rep in range(3):
    for name, _, fn in ema_variants:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            fn()
        e1.record(); torch.cuda.synchronize()
        rows[name].append(e0.elapsed_time(e1) / 10)
        print(f"ema row {rep}: {name}: {rows[name][-1]:.3f} ms (10 launches)")
base = sum(rows["ungrouped K.adamw"]) / 3
for name, bpp, _ in ema_variants:
    r = rows[name]
    mean = sum(r) / len(r)
    print(f"{name}: mean {mean:.3f} ms, spread {max(r) - min(r):.3f} ms, {n * bpp / mean / 1e9:.2f} TB/s at {bpp} B/param, "
          f"{mean / base:.3f} x the ungrouped plain kernel (traffic model: {bpp / 34:.3f})")

# ---- gradient accumulation: a hold launch and an apply launch beside the ungrouped row, on the same arena
accum_rows()
