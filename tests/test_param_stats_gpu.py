"""Per-parameter gradient and weight statistics on the MI355X (vacnic_param_stats, FusedAdamW(grad_stats_every=N),
--grad_stats_every): the kernel against numpy int64 / float64 at every slot and unit edge, its determinism, the device-side gate,
the optimizer option next to a twin without it, and a recorded launch plan and a captured graph against the eager run.
NaN and Inf are ordinary values placed in gradients."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAN, INF = float("nan"), float("inf")
PLANTS = (NAN, INF, -INF, 3e19)             # 3e19 is finite, its square is not
BIG = (1 << 20) + 3                         # 257 units: pass 2's threads take more than one partial
# (offset, numel): length 1 at 0, length 3 at 1, a unit less one / a unit / a unit and one at odd offsets, a 5-element gap, a slot of
# more than 256 units, and a last slot that ends exactly at N.  Elements 4, 4100, 8197, 8198, 12296..12300 and three after the
# big slot lie in no slot.
SLOTS = [(0, 1), (1, 3), (5, 4095), (4101, 4096), (8199, 4097), (12301, BIG), (12301 + BIG + 3, 4493)]
N = SLOTS[-1][0] + SLOTS[-1][1]
assert N % 4 == 0 and N == 1065376
SENT_F, SENT_I = 0x7FC12345, -7             # pre-fill of the outputs: a NaN bit pattern no result can equal, and a negative count

# Error bound of the two fp32 sums against float64, in units of 2^-24 relative (all terms are non-negative, so the relative error
# of a sum is at most the number of roundings on the longest chain into it): pass 1 gives a lane the up to 16 vectors lane,
# lane + 64, ... of a 4096-element unit, 64 terms, and lanes 0..2 one head and one tail element more: 66 fused multiply-adds; the
# wave butterfly adds 6 levels.  Pass 2: a thread adds ceil(257 / 256) = 2 partials, then 6 butterfly levels and 2 levels over the
# four waves.  66 + 6 + 2 + 6 + 2 = 82 roundings <= 100 * 2^-24 = 6.0e-6 (the issue's shape, 4096 serial terms per pass, gives 4.9e-4).
SUM_RTOL = 100 * 2.0 ** -24


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def tab():
    from vacnic_amd.arena import stats_table_from_slots
    t = stats_table_from_slots(SLOTS)
    assert t.nunit == 1 + 1 + 1 + 1 + 2 + 257 + 2
    return t.to("cuda")


def in_slots():
    m = np.zeros(N, dtype=bool)
    for o, n in SLOTS:
        m[o:o + n] = True
    return m


_DATA = {}


def int_data():
    """integer-valued g in [-3, 3] with planted zeros and p in [-5, 5]; NaN in both outside the slots.  Made once, never written."""
    if not _DATA:
        rng = np.random.default_rng(11)
        g = rng.integers(-3, 4, N).astype(np.float32)
        p = rng.integers(-5, 6, N).astype(np.float32)
        for o, n in SLOTS:
            g[o + n // 2:o + n // 2 + min(n, 9) // 2] = 0.0          # a run of planted zeros in the middle of every slot
        g[0] = 2.0; g[1:4] = (0.0, -3.0, 1.0)
        out = ~in_slots()
        g[out] = NAN; p[out] = NAN
        assert int((g[~out] ** 2).sum()) < 1 << 24 and int((p[~out] ** 2).sum()) < 1 << 24
        _DATA["g"], _DATA["p"] = g, p
    return _DATA["g"], _DATA["p"]


def reference(g, p, scale):
    """float64 / int64 statistics per slot, with the kernel's own definition of x and of non-finite (both in fp32)"""
    f, c = np.zeros((len(SLOTS), 4)), np.zeros((len(SLOTS), 2), dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for s, (o, n) in enumerate(SLOTS):
            gs = g[o:o + n]
            x = gs * np.float32(scale)
            bad = ~np.isfinite(x * x)
            xf = x[~bad].astype(np.float64)
            f[s, 0], f[s, 1] = (xf * xf).sum(), np.abs(xf).max() if xf.size else 0.0
            if p is not None:
                ps = p[o:o + n].astype(np.float64)
                f[s, 2], f[s, 3] = (ps * ps).sum(), np.abs(ps).max()
            c[s] = bad.sum(), (gs == 0).sum()
    return f, c


def run(K, tab, g, p, scale=1.0, **kw):
    gd = torch.from_numpy(g).cuda()
    pd = None if p is None else torch.from_numpy(p).cuda()
    out_f, out_i, stamp = K.param_stats(gd, pd, N, tab, grad_scale=scale, **kw)
    torch.cuda.synchronize()
    return out_f.cpu().numpy(), out_i.cpu().numpy(), stamp.tolist()


# ----------------------------------------------------------------------------------------------------- 1: exact at every edge
@pytest.mark.parametrize("with_p", [True, False])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_integer_values_are_exact_at_every_slot_and_unit_edge(K, tab, scale, with_p):
    g, p = int_data()
    out_f, out_i, stamp = run(K, tab, g, p if with_p else None, scale)
    want_f, want_c = reference(g, p if with_p else None, scale)
    assert np.array_equal(out_f.astype(np.float64), want_f), (out_f, want_f)
    assert np.array_equal(out_i, want_c), (out_i, want_c)
    assert (want_c[:, 0] == 0).all() and (want_c[1:, 1] > 0).all() and want_f[5, 0] > 1e6
    assert stamp == [1, -1, 0, 0], "hyper = NULL fires, and says so"
    if not with_p:
        assert (out_f[:, 2:] == 0).all()


# ------------------------------------------------------------------------------------------------------ 2: non-finite elements
@pytest.mark.parametrize("slot", [2, 4, 5])
def test_planted_nonfinite_elements_are_counted_and_left_out(K, tab, slot):
    """at the first element of a slot, at its last, and in the middle of a unit; the neighbouring slots do not change"""
    g0, p = int_data()
    base_f, base_i, _ = run(K, tab, g0, p)
    o, n = SLOTS[slot]
    where = [o, o + n - 1, o + 1000]
    for k in range(len(PLANTS)):
        g = g0.copy()
        for j, w in enumerate(where):
            g[w] = PLANTS[(k + j) % 4]
        out_f, out_i, _ = run(K, tab, g, p)
        want_f, want_c = reference(g, p, 1.0)
        assert want_c[slot, 0] == 3
        assert np.array_equal(out_i, want_c), (out_i, want_c)
        assert np.array_equal(out_f.astype(np.float64), want_f)
        others = [s for s in range(len(SLOTS)) if s != slot]
        assert np.array_equal(out_f[others].view(np.int32), base_f[others].view(np.int32)) and np.array_equal(out_i[others], base_i[others])
    g = g0.copy()
    g[o:o + n] = NAN                                             # a slot with nothing finite: 0, 0 and its length
    out_f, out_i, _ = run(K, tab, g, p)
    assert out_f[slot, 0] == 0 and out_f[slot, 1] == 0 and out_i[slot].tolist() == [n, 0]
    assert out_f[slot, 2] == base_f[slot, 2] and out_f[slot, 3] == base_f[slot, 3]


# ------------------------------------------------------------------------------------------------------------------ 3: floats
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_random_floats_against_float64_and_the_clip_norm(K, tab, scale):
    """sums within SUM_RTOL (derived above) of float64; the largest magnitudes and the counts exactly; the total norm against
    grad_clip_coef's on the same buffer with the gaps zeroed.  That kernel's own sum: a thread of its 1024 x 256 grid adds the 4 or
    8 squares of at most two vectors at this size, 8 tree levels, then 4 partials per thread and 8 more levels in its second pass:
    28 roundings.  Both norms are square roots (half the relative error of the sums, plus one rounding each):
    (100 + 28) / 2 + 2 = 66 units of 2^-24."""
    rng = np.random.default_rng(5)
    g = (rng.standard_normal(N) * 3.0).astype(np.float32)
    p = rng.standard_normal(N).astype(np.float32)
    g[SLOTS[5][0] + 77:SLOTS[5][0] + 99] = 0.0
    out = ~in_slots()
    g[out] = NAN; p[out] = NAN
    out_f, out_i, _ = run(K, tab, g, p, scale)
    want_f, want_c = reference(g, p, scale)
    for col in (0, 2):
        rel = np.abs(out_f[:, col] - want_f[:, col]) / want_f[:, col]
        print(f"column {col}: largest relative error {rel.max():.3g} (bound {SUM_RTOL:.3g})")
        assert (rel <= SUM_RTOL).all(), (col, rel)
    assert np.array_equal(out_f[:, 1].astype(np.float64), want_f[:, 1]) and np.array_equal(out_f[:, 3].astype(np.float64), want_f[:, 3])
    assert np.array_equal(out_i, want_c) and want_c[5, 1] == 22
    total = float(np.sqrt(out_f[:, 0].astype(np.float64).sum()))
    gz = g.copy(); gz[out] = 0.0
    clip = K.grad_clip_coef(torch.from_numpy(gz).cuda(), N, 0.1, grad_scale=scale)[1].item()
    print(f"total norm {total!r} against the clip pass's {clip!r}")
    assert abs(total - clip) <= 66 * 2.0 ** -24 * clip, (total, clip)


# ------------------------------------------------------------------------------------------------------------- 4: determinism
def test_two_launches_are_bitwise_equal_whatever_the_workspace_held(K, tab):
    rng = np.random.default_rng(6)
    g = torch.from_numpy((rng.standard_normal(N) * 3.0).astype(np.float32)).cuda()
    p = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).cuda()
    work = K.param_stats_workspace(tab, "cuda")
    work.zero_()
    a_f, a_i, _ = K.param_stats(g, p, N, tab, workspace=work)
    b_f, b_i, _ = K.param_stats(g, p, N, tab, workspace=work)
    work.fill_(0xFF)
    c_f, c_i, _ = K.param_stats(g, p, N, tab, workspace=work)
    torch.cuda.synchronize()
    for x_f, x_i in ((b_f, b_i), (c_f, c_i)):
        assert torch.equal(a_f.view(torch.int32), x_f.view(torch.int32)) and torch.equal(a_i, x_i)
    assert torch.isfinite(a_f).all() and (a_f[:, 0] > 0).all()


# -------------------------------------------------------------------------------------------------------------------- 5: gate
def _sentinels(tab):
    out_f = torch.full((tab.nslot, 4), SENT_F, device="cuda", dtype=torch.int32).view(torch.float32)
    out_i = torch.full((tab.nslot, 2), SENT_I, device="cuda", dtype=torch.int64)
    stamp = torch.tensor([5, -9, -9, -9], device="cuda", dtype=torch.int64)
    return out_f, out_i, stamp


def _untouched(out_f, out_i, stamp):
    return bool((out_f.view(torch.int32) == SENT_F).all()) and bool((out_i == SENT_I).all()) and stamp.tolist() == [5, -9, -9, -9]


def test_gate_fires_on_multiples_of_every_on_a_skip_and_without_hyper(K, tab):
    g_np, p_np = int_data()
    g, p = torch.from_numpy(g_np).cuda(), torch.from_numpy(p_np).cuda()
    want_f, want_c = reference(g_np, p_np, 1.0)
    work = K.param_stats_workspace(tab, "cuda")
    skip = torch.zeros(4, device="cuda", dtype=torch.int64)
    for with_skip in (False, True):
        for t in range(1, 8):
            out_f, out_i, stamp = _sentinels(tab)
            hyper = torch.tensor([1e-4, float(t)], device="cuda")
            K.param_stats(g, p, N, tab, hyper, 3, skip if with_skip else None, workspace=work, out_f=out_f, out_i=out_i, stamp=stamp)
            torch.cuda.synchronize()
            if t in (3, 6):
                assert stamp.tolist() == [6, t, 0, 0]
                assert np.array_equal(out_f.cpu().numpy().astype(np.float64), want_f) and np.array_equal(out_i.cpu().numpy(), want_c)
            else:
                assert _untouched(out_f, out_i, stamp), f"count {t}: a call that does not fire writes nothing"
    skip[0] = 1
    for t in (1, 3, 5):
        out_f, out_i, stamp = _sentinels(tab)
        K.param_stats(g, p, N, tab, torch.tensor([1e-4, float(t)], device="cuda"), 3, skip, workspace=work, out_f=out_f, out_i=out_i,
                      stamp=stamp)
        torch.cuda.synchronize()
        assert stamp.tolist() == [6, t, 1, 0] and np.array_equal(out_i.cpu().numpy(), want_c)
    out_f, out_i, stamp = _sentinels(tab)
    K.param_stats(g, p, N, tab, None, 3, None, workspace=work, out_f=out_f, out_i=out_i, stamp=stamp)
    torch.cuda.synchronize()
    assert stamp.tolist() == [6, -1, 0, 0] and np.array_equal(out_i.cpu().numpy(), want_c)


def test_bad_arguments_raise_and_launch_nothing(K, tab):
    from vacnic_amd import _lib
    g_np, _ = int_data()
    g = torch.from_numpy(g_np).cuda()
    work = K.param_stats_workspace(tab, "cuda")
    out_f, out_i, stamp = _sentinels(tab)
    good = dict(g=g.data_ptr(), p=None, n=N, grad_scale=1.0, unit_off=tab.unit_off.data_ptr(), unit_len=tab.unit_len.data_ptr(),
                nunit=tab.nunit, slot_unit=tab.slot_unit.data_ptr(), nslot=tab.nslot, hyper=None, every=1, skip=None,
                workspace=work.data_ptr(), workspace_bytes=work.numel(), out_f=out_f.data_ptr(), out_i=out_i.data_ptr(),
                stamp=stamp.data_ptr())
    assert work.numel() == _lib.lib.vacnic_param_stats_workspace_bytes(tab.nunit, tab.nslot) > 0
    for bad, msg in ((dict(g=None), "null operand"), (dict(nslot=0), "nslot"), (dict(every=0), "every"), (dict(n=-4), "n=-4"),
                     (dict(workspace_bytes=work.numel() - 1), "workspace"), (dict(out_f=None), "null operand"),
                     (dict(g=g.data_ptr() + 4), "aligned")):
        with pytest.raises(ValueError, match=msg):
            _lib.call_struct("vacnic_param_stats", stream=K._stream(), **dict(good, **bad))
    torch.cuda.synchronize()
    assert _untouched(out_f, out_i, stamp)
    _lib.call_struct("vacnic_param_stats", stream=K._stream(), **good)      # control: the same arguments, unbroken, fire
    torch.cuda.synchronize()
    assert stamp.tolist() == [6, -1, 0, 0]


# --------------------------------------------------------------------------------------------------------------- 6: optimizer
class _Small(torch.nn.Module):
    """a tied parameter (emb under two names), a fused group whose members are adjacent and start unaligned, a slot with padded
    rows, and a parameter of more than two units"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(9)
        self.emb = torch.nn.Parameter(torch.randn(10, 6, generator=g))
        self.a = torch.nn.Parameter(torch.randn(7, generator=g))
        self.b = torch.nn.Parameter(torch.randn(5003, generator=g))
        self.c = torch.nn.Parameter(torch.randn(3, 3, generator=g))
        self.big = torch.nn.Parameter(torch.randn(4096 * 2 + 1, generator=g))
        self.head = self.emb

    def arena_groups(self):
        return [[self.a, self.b, self.c]]


NAMES = ["emb", "a", "b", "c", "big"]


def _opt(world=1, groups=None, **kw):
    from vacnic_amd.arena import ParamArena
    from vacnic_amd.training import FusedAdamW
    m = _Small()
    arena = ParamArena(m, "cuda", pad_rows={id(m.emb): 32})
    if groups is not None:
        kw.update(param_groups=groups, named_parameters=m.named_parameters())
    return m, arena, FusedAdamW(arena, lr=1e-3, num_warmup_steps=0, num_training_steps=100, world_size=world, **kw)


def _planted(arena, m, step, integers=True):
    """this step's gradient: integer values (exact sums) or normal floats inside the parameters, zero elsewhere, as backward leaves it"""
    gen = torch.Generator().manual_seed(100 + step)
    g = torch.zeros(arena.n)
    for nm in NAMES:
        o, n, _ = arena.slots[id(getattr(m, nm))]
        g[o:o + n] = torch.randint(-3, 4, (n,), generator=gen).float() if integers else torch.randn(n, generator=gen)
    return g.cuda()


def _want(arena, m, g, scale):
    g = g.cpu().numpy()
    p = arena.flat32.cpu().numpy()
    out = {}
    with np.errstate(over="ignore", invalid="ignore"):
        for nm in NAMES:
            o, n, _ = arena.slots[id(getattr(m, nm))]
            x = g[o:o + n] * np.float32(scale)
            bad = ~np.isfinite(x * x)
            xf, pf = x[~bad].astype(np.float64), p[o:o + n].astype(np.float64)
            out[nm] = {"gsq": float((xf * xf).sum()), "grad_absmax": float(np.abs(xf).max()), "wsq": float((pf * pf).sum()),
                       "weight_absmax": float(np.abs(pf).max()), "nonfinite": int(bad.sum()), "zeros": int((g[o:o + n] == 0).sum()),
                       "numel": n}
    return out


def _state(arena, opt):
    return [arena.flat32, arena.exp_avg, arena.exp_avg_sq, arena.flat16, arena.grad, opt.hyper] + ([arena.ema] if arena.ema is not None else [])


@pytest.mark.parametrize("world", [1, 2])
def test_optimizer_records_every_second_step_and_writes_what_its_twin_writes(world):
    m, arena, opt = _opt(world, grad_stats_every=2)
    m2, arena2, twin = _opt(world)
    assert twin._stats is None and opt._stats is not None
    assert opt.grad_stats(m.named_parameters())["fires"] == 0
    for step in range(1, 5):
        g = _planted(arena, m, step)
        arena.grad.copy_(g); arena2.grad.copy_(g)
        want = _want(arena, m, g, 1.0 / world)                     # (the weights as this step finds them)
        opt.step(); twin.step()
        torch.cuda.synchronize()
        for x, y, nm in zip(_state(arena, opt), _state(arena2, twin), ("p", "m", "v", "shadow", "g", "hyper")):
            assert torch.equal(x, y), f"step {step}: {nm} differs from the optimizer without the option"
        assert (arena.grad == 0).all()
        rep = opt.grad_stats(m.named_parameters())
        assert rep["fires"] == step // 2
        if step % 2 == 0:
            assert rep["step"] == step and rep["dropped"] is False
            assert list(rep["params"]) == NAMES, "first names in named_parameters order; the tied parameter once"
            for nm in NAMES:
                got, w = rep["params"][nm], want[nm]
                # integer gradients: the fp32 sums are exact; the weights are floats: SUM_RTOL on the sum, half of it (and the
                # float64 square root's own rounding, far below) on the norm
                assert got["grad_norm"] == np.sqrt(w["gsq"]) and got["grad_absmax"] == w["grad_absmax"], (nm, got, w)
                assert abs(got["weight_norm"] - np.sqrt(w["wsq"])) <= SUM_RTOL * np.sqrt(w["wsq"]) and got["weight_absmax"] == w["weight_absmax"]
                assert (got["nonfinite"], got["zeros"], got["numel"]) == (0, w["zeros"], w["numel"])
            assert sum(w["zeros"] for w in want.values()) > 1000, "integers in [-3, 3]: a seventh of them are zero"
            assert rep["total_grad_norm"] == np.sqrt(sum(w["gsq"] for w in want.values()))
    assert opt.hyper[1].item() == 4.0


def test_dropped_step_is_recorded_off_the_interval_with_everything_on():
    """groups (a frozen parameter among them), clipping, the guard and the moving average on; every = 3"""
    spec = [{"match": "^big$", "frozen": True}, {"match": "^b$", "lr_scale": 10.0}, {"match": "^c$", "weight_decay": 0.0}]
    kw = dict(groups=spec, skip_nonfinite=True, ema_decay=0.99)
    m, arena, opt = _opt(grad_stats_every=3, **kw)
    m2, arena2, twin = _opt(**kw)
    ob = arena.slots[id(m.b)][0]
    for step in (1, 2, 3):
        g = _planted(arena, m, step)
        if step == 2:
            g[ob + 4999] = NAN                                       # in `b`, a trained parameter
        arena.grad.copy_(g); arena2.grad.copy_(g)
        want = _want(arena, m, g, 1.0)
        opt.step(clip_norm=0.1); twin.step(clip_norm=0.1)
        torch.cuda.synchronize()
        for x, y, nm in zip(_state(arena, opt) + [opt.guard, opt.clip], _state(arena2, twin) + [twin.guard, twin.clip],
                            ("p", "m", "v", "shadow", "g", "hyper", "ema", "guard", "clip")):
            assert torch.equal(x, y) or (nm == "clip" and step == 2), f"step {step}: {nm} differs from the optimizer without the option"
        rep = opt.grad_stats(m.named_parameters())
        if step == 1:
            assert rep["fires"] == 0
        if step == 2:
            assert rep["fires"] == 1 and rep["dropped"] is True and rep["step"] == 1, rep
            assert [nm for nm, v in rep["params"].items() if v["nonfinite"]] == ["b"] and rep["params"]["b"]["nonfinite"] == 1
            assert opt.guard_report(m.named_parameters())["first_nonfinite"] == "b"
            assert rep["params"]["b"]["grad_norm"] == np.sqrt(want["b"]["gsq"]) and rep["params"]["big"]["grad_norm"] > 0, \
                "the finite rest of b, and the frozen parameter like any other"
        if step == 3:
            assert rep["fires"] == 1 and opt.hyper[1].item() == 2.0, "count 2 after a dropped and two applied steps: off the interval"


# ---------------------------------------------------------------------------------------------------------- 7: plan and graph
def _eager_reference(steps):
    """the eager run both replays are compared with: (out_f, out_i, stamp, p) after every step, every = 2, float gradients"""
    m, arena, opt = _opt(grad_stats_every=2)
    out = []
    for step in range(1, steps + 1):
        arena.grad.copy_(_planted(arena, m, step, integers=False))
        opt.step()
        torch.cuda.synchronize()
        _, _, out_f, out_i, stamp = opt._stats
        out.append([t.clone() for t in (out_f, out_i, stamp, arena.flat32)])
    return out


def _same(opt, arena, want, step):
    _, _, out_f, out_i, stamp = opt._stats
    for x, y, nm in zip((out_f.view(torch.int32), out_i, stamp, arena.flat32), (want[0].view(torch.int32), *want[1:]),
                        ("out_f", "out_i", "stamp", "p")):
        assert torch.equal(x, y), f"step {step}: {nm} differs from the eager run"


def test_recorded_launch_plan_carries_the_gated_kernel():
    from vacnic_amd import _lib, ops
    want = _eager_reference(4)
    assert [w[2].tolist() for w in want] == [[0, 0, 0, 0], [1, 2, 0, 0], [1, 2, 0, 0], [2, 4, 0, 0]]
    m, arena, opt = _opt(grad_stats_every=2)
    ops.Rng.device_counter()
    torch.cuda.synchronize()
    arena.grad.copy_(_planted(arena, m, 1, integers=False))
    h = int(_lib.lib.vacnic_plan_begin())
    assert h >= 0
    try:
        opt.step()                                                  # step 1: recorded while it runs
        _lib.check(_lib.lib.vacnic_plan_end(h))
        size = int(_lib.lib.vacnic_plan_size(h))
        assert size == 3, "lr_step, param_stats, adamw"
        torch.cuda.synchronize()
        _same(opt, arena, want[0], 1)
        for step in (2, 3, 4):
            arena.grad.copy_(_planted(arena, m, step, integers=False))
            _lib.call("vacnic_plan_replay", h, 0, size)
            torch.cuda.synchronize()
            _same(opt, arena, want[step - 1], step)
    finally:
        _lib.check(_lib.lib.vacnic_plan_destroy(h))


def test_captured_graph_carries_the_gated_kernel():
    from vacnic_amd import ops
    want = _eager_reference(5)
    m, arena, opt = _opt(grad_stats_every=2)
    ops.Rng.device_counter()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # step 1: eager warm-up on a side stream
        arena.grad.copy_(_planted(arena, m, 1, integers=False))
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _same(opt, arena, want[0], 1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for step in (2, 3, 4, 5):
        arena.grad.copy_(_planted(arena, m, step, integers=False))
        graph.replay()
        torch.cuda.synchronize()
        _same(opt, arena, want[step - 1], step)
    assert opt._stats[4].tolist() == [2, 4, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ trainer
def test_trainer_logs_the_statistics_from_a_replayed_plan(tmp_path):
    """--grad_stats_every 2 under --launch_plan True (step 1 eager, step 2 recorded, 3 and 4 replayed): the log record and the
    jsonl file carry steps 2 and 4."""
    import importlib.util
    from vacnic_amd import streams, synthetic
    spec = importlib.util.spec_from_file_location(
        "trainer_stats_test", os.path.join(ROOT, "train_mmbart_enc_self_face_name_ids_retrieve_crossattn_bart_guide_match.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parser.parse_args(["--plm_type", "facebook/bart-base", "--clip_type", "ViT-B/32", "--enc_fusion_layer", "0", "1",
                                  "--dim_common", "768", "--train_batch_size", "2", "--article_max_length", "64", "--steps_per_epoch", "4",
                                  "--log_every", "1", "--out_dir", str(tmp_path), "--experiment_name", "t", "--grad_stats_every", "2"])
    cfg, _ = mod.build_config(args)
    batches = [synthetic.make_batch(cfg, 2, S=64, T=12, seed=90, step=i) for i in range(4)]
    try:
        hist = mod.run(args, batches)
    finally:
        streams.enable(False)
        torch.cuda.synchronize()
    assert [r.get("grad_stats_step") for r in hist] == [None, 2, None, 4], hist
    assert all(np.isfinite(r["grad_norm"]) and r["grad_norm"] > 0 for r in hist if "grad_stats_step" in r)
    lines = [json.loads(l) for l in open(os.path.join(tmp_path, "t_gradstats.jsonl"))]
    assert [l["step"] for l in lines] == [2, 4] and not any(l["dropped"] for l in lines)
    for l, r in zip(lines, (hist[1], hist[3])):
        assert l["total_grad_norm"] == r["grad_norm"]
        assert "model.shared.weight" in l["params"] and "lm_head.weight" not in l["params"], "first names: the tied head once"
        rows = np.array(list(l["params"].values()), dtype=np.float64)
        assert rows.shape[1] == 6 and (rows[:, 4] == 0).all() and np.isfinite(rows).all()
        assert abs(np.sqrt((rows[:, 0] ** 2).sum()) - l["total_grad_norm"]) <= 1e-9 * l["total_grad_norm"]
