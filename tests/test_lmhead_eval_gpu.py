"""The fused validation head on the MI355X (vacnic_lmhead_eval: the argmax epilogue of gemm_t256ceam.hip, eval_combine_kernel,
eval_seq_kernel, eval_totals_kernel) against the float64 host model of tests/test_lmhead_eval.py, whose docstring derives every
margin used here; at the smallest shapes that reach both sides of the 256-column tile, the 8-column group and the 256-row tile.
row_lse is held bit for bit to vacnic_lmhead_ce_fwd's.  Every check prints `LOSSCHK ...` / `EVALCHK ...` lines with its figures."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_loss_gpu import F64, check, check_equal, cpu_randn, host          # noqa: E402
from test_lmhead_eval import (EVAL_RS, EVAL_V, EXACT_PAIRS, eval_case, eval_model, exact_case, row_margin)   # noqa: E402

GUARD = 16
FILLS = {torch.float32: -7.0, torch.int32: -7, torch.int64: -7, torch.float64: -7.0}


@pytest.fixture(scope="module")
def K():
    from vacnic_amd import kernels
    return kernels


class Buffers:
    """scratch and outputs of one call, each inside a buffer of its own with GUARD sentinel elements on either side."""

    def __init__(self, K, R, V, rps):
        tiles, S = (V + 255) // 256, max(R // rps, 1)
        self.full = {}

        def make(name, n, dtype):
            full = torch.full((n + 2 * GUARD,), FILLS[dtype], device="cuda", dtype=dtype)
            self.full[name] = (full, n)
            return full[GUARD:GUARD + n]
        self.part = make("part", R * tiles * 2, torch.float32).view(R, tiles, 2)
        self.part_arg = make("part_arg", R * tiles, torch.int32).view(R, tiles)
        self.tl = make("tl", R, torch.float32)
        self.out = K.LmheadEval(row_lse=make("row_lse", R, torch.float32), row_nll=make("row_nll", R, torch.float32),
                                pred=make("pred", R, torch.int64), seq_nll=make("seq_nll", S, torch.float32),
                                seq_tokens=make("seq_tokens", S, torch.int32), seq_correct=make("seq_correct", S, torch.int32))
        self.totals = make("totals", 4, torch.float64)

    def sentinels_untouched(self, what):
        for name, (full, n) in self.full.items():
            fill = FILLS[full.dtype]
            assert (full[:GUARD] == fill).all() and (full[GUARD + n:] == fill).all(), f"{what}: wrote outside {name}"

    def untouched(self):
        return all(bool((full == FILLS[full.dtype]).all()) for full, _ in self.full.values())


def run(K, c, totals=True, buf=None, zero=True):
    dev = {k: (None if c[k] is None else c[k].cuda()) for k in ("h", "E", "bias", "tgt")}
    buf = buf or Buffers(K, c["R"], c["V"], c["rps"])
    if totals and zero:
        K.zero_(buf.totals)
    K.lmhead_eval_into(dev["h"], dev["E"], dev["tgt"], c["V"], c["rps"], buf.part, buf.part_arg, buf.tl, buf.out,
                       ignore_index=c["ignore"], bias=dev["bias"], totals=buf.totals if totals else None)
    torch.cuda.synchronize()
    return dev, buf


def compare_integers(what, c, buf, calls=1):
    m, o = c["m64"], buf.out
    check_equal(f"{what} seq_tokens", o.seq_tokens, m["seq_tokens"])
    check_equal(f"{what} seq_correct", o.seq_correct, m["seq_correct"])
    tot = host(buf.totals)
    print(f"EVALCHK {what} totals={tot.tolist()} want={(m['totals'] * calls).tolist()}")
    assert torch.equal(tot[1:], m["totals"][1:] * calls), "token / correct / caption counts are exact"
    empty = host(o.seq_tokens) == 0
    assert (host(o.seq_nll)[empty] == 0).all(), "a caption without tokens has seq_nll == 0"


def compare(what, c, K, dev, buf):
    m64, m32, o, R, rps = c["m64"], c["m32"], buf.out, c["R"], c["rps"]
    lse, _ = K.lmhead_ce_fwd(dev["h"], dev["E"], dev["tgt"], c["V"], ignore_index=c["ignore"], bias=dev["bias"])
    torch.cuda.synchronize()
    assert torch.equal(o.row_lse, lse), f"{what}: row_lse differs from vacnic_lmhead_ce_fwd's by up to {(o.row_lse - lse).abs().max().item():.3e}"
    check(f"{what} row_nll", o.row_nll, m64["nll"], m32["nll"], extra=c["a_lse"])
    ign = c["tgt"] == c["ignore"]
    assert (host(o.row_nll)[ign] == 0).all(), "row_nll of an ignored row is an exact 0"
    # pred: inside a_r of the float64 maximum everywhere; the float64 argmax wherever the top-2 gap exceeds a_r
    pred = host(o.pred)
    assert ((pred >= 0) & (pred < c["V"])).all(), "a prediction outside the real columns"
    z = c["z64"]
    short = z.max(1).values - z.gather(1, pred[:, None])[:, 0]
    decided = c["gap"] > c["a_r"]
    print(f"EVALCHK {what} pred: max shortfall={short.max().item():.3e} max a_r={c['a_r'].max().item():.3e} "
          f"undecided rows={int((~decided).sum())}/{R} wrong={int((pred != m64['pred']).sum())}")
    assert (short <= c["a_r"]).all()
    assert torch.equal(pred[decided], m64["pred"][decided])
    assert int((~decided).sum()) <= 0.01 * R
    compare_integers(what, c, buf)
    margin = rps * row_margin(c)
    err = (host(o.seq_nll).to(F64) - m64["seq_nll"]).abs().max().item()
    print(f"EVALCHK {what} seq_nll bound={margin:.3e} err={err:.3e}")
    assert err <= margin
    terr = abs(host(buf.totals)[0].item() - m64["totals"][0].item())
    assert terr <= R * row_margin(c), f"totals[0] off by {terr}"
    buf.sentinels_untouched(what)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("R,rps", EVAL_RS)
@pytest.mark.parametrize("V", EVAL_V)
def test_eval_tile_edges(K, V, R, rps, with_bias):
    c = eval_case(V, R, 64, rps, with_bias)
    dev, buf = run(K, c)
    compare(f"eval V={V} R={R} rps={rps} bias={with_bias}", c, K, dev, buf)


def test_eval_d72(K):
    """d = 72: K no multiple of the 32-deep K tile."""
    c = eval_case(257, 36, 72, 4, True)
    dev, buf = run(K, c)
    compare("eval V=257 R=36 d=72", c, K, dev, buf)


def test_eval_full_vocabulary_row_lse(K):
    """V = 50265: 197 tiles per row, so the combine kernel's lanes walk more than one tile each."""
    c = eval_case(50265, 64, 64, 1, False)
    dev, buf = run(K, c)
    compare("eval V=50265 R=64", c, K, dev, buf)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("V", [513, 257])
def test_eval_exact_ties_and_negative_rows(K, V, with_bias):
    """integer logits: ties inside a thread's walk, across lanes ((0, 255)), across tiles ((255, 256), (256, V - 1)), rows whose
    real logits are all negative (a zero pad column must not win), V = 257 with ONE valid column in the last tile."""
    for pair in EXACT_PAIRS:
        c = exact_case(V, pair, with_bias)
        what = f"exact V={V} pair={c['pair']} bias={with_bias}"
        dev, buf = run(K, c)
        check_equal(f"{what} pred", buf.out.pred, torch.argmax(c["z64"][:, :V], 1))
        compare_integers(what, c, buf)
        assert (host(buf.out.row_nll)[c["tgt"] == 1] == 0).all()
        buf.sentinels_untouched(what)


def test_eval_totals_accumulate_over_calls_and_runs_are_bit_reproducible(K):
    c = eval_case(513, 260, 64, 65, True)
    dev, buf = run(K, c)
    first = [host(t).clone() for t in buf.out] + [host(buf.totals).clone()]
    dev, buf = run(K, c, buf=buf, zero=False)                        # the same buffers: totals now hold both calls
    for name, a, b in zip(K.LmheadEval._fields, first, buf.out):
        assert torch.equal(a, host(b)), f"{name} differs between two launches on the same inputs"
    compare_integers("eval totals after two calls", c, buf, calls=2)
    assert host(buf.totals)[0].item() == 2 * first[-1][0].item(), "the second call adds the same f64 sum"
    dev, buf2 = run(K, c, totals=False)
    assert torch.equal(host(buf2.totals), torch.full((4,), FILLS[torch.float64], dtype=F64)), "totals = NULL: nothing is accumulated"
    for name, a, b in zip(K.LmheadEval._fields, first, buf2.out):
        assert torch.equal(a, host(b)), f"{name} differs in a fresh set of buffers"


def test_eval_public_wrapper(K):
    c = eval_case(257, 255, 64, 5, True)
    dev = {k: c[k].cuda() for k in ("h", "E", "bias", "tgt")}
    totals = K.zero_(torch.empty(4, device="cuda", dtype=F64))
    out = K.lmhead_eval(dev["h"], dev["E"], dev["tgt"], 257, 5, ignore_index=1, bias=dev["bias"], totals=totals)
    _, buf = run(K, c)
    for name, a, b in zip(K.LmheadEval._fields, out, buf.out):
        assert torch.equal(a, b), name
    assert torch.equal(totals, buf.totals)
    with pytest.raises(ValueError, match="float64"):
        K.lmhead_eval(dev["h"], dev["E"], dev["tgt"], 257, 5, totals=torch.zeros(4, device="cuda"))


def test_eval_refusals_launch_nothing(K):
    c = eval_case(257, 255, 64, 5, False)
    dev = {k: c[k].cuda() for k in ("h", "E", "tgt")}
    buf = Buffers(K, 255, 257, 5)
    args = (buf.part, buf.part_arg, buf.tl)
    with pytest.raises(ValueError, match="rows_per_seq"):
        K.lmhead_eval_into(dev["h"], dev["E"], dev["tgt"], 257, 4, *args, buf.out)
    with pytest.raises(ValueError, match="rows_per_seq"):
        K.lmhead_eval_into(dev["h"], dev["E"], dev["tgt"], 257, 0, *args, buf.out)
    with pytest.raises(ValueError, match="part_tiles"):
        K.lmhead_eval_into(dev["h"], dev["E"], dev["tgt"], 257, 5, *args, buf.out, part_tiles=3)
    with pytest.raises(ValueError, match="part_tiles"):
        K.lmhead_eval_into(dev["h"], dev["E"], dev["tgt"], 257, 5, *args, buf.out, part_tiles=1)
    for field in K.LmheadEval._fields:
        with pytest.raises(ValueError, match="null operand"):
            K.lmhead_eval_into(dev["h"], dev["E"], dev["tgt"], 257, 5, *args, buf.out._replace(**{field: None}))
    with pytest.raises(ValueError, match="null operand"):
        K.lmhead_eval_into(dev["h"], dev["E"], dev["tgt"], 257, 5, buf.part, None, buf.tl, buf.out)
    torch.cuda.synchronize()
    assert buf.untouched(), "a refused call wrote something"


def test_eval_recorded_in_a_launch_plan(K):
    """the call is ONE command of a launch plan; replayed after h is refreshed in place it gives the eager call's results."""
    from vacnic_amd import _lib
    c0 = eval_case(513, 260, 64, 65, True)
    c1 = dict(c0, h=cpu_randn(260, 64, seed=4242))
    want0, want1 = run(K, c0)[1], run(K, c1)[1]
    dev = {k: c0[k].cuda() for k in ("h", "E", "bias", "tgt")}
    buf = Buffers(K, 260, 513, 65)
    torch.cuda.synchronize()
    h = int(_lib.lib.vacnic_plan_begin())
    assert h >= 0
    try:
        K.lmhead_eval_into(dev["h"], dev["E"], dev["tgt"], 513, 65, buf.part, buf.part_arg, buf.tl, buf.out, bias=dev["bias"])
        _lib.check(_lib.lib.vacnic_plan_end(h))
        assert int(_lib.lib.vacnic_plan_size(h)) == 1
        torch.cuda.synchronize()
        for a, b in zip(buf.out, want0.out):
            assert torch.equal(a, b)
        dev["h"].copy_(c1["h"].cuda())
        _lib.call("vacnic_plan_replay", h, 0, 1)
        torch.cuda.synchronize()
        assert not torch.equal(buf.out.row_lse, want0.out.row_lse)
        for name, a, b in zip(K.LmheadEval._fields, buf.out, want1.out):
            assert torch.equal(a, b), f"{name}: the replay differs from the eager call"
    finally:
        _lib.check(_lib.lib.vacnic_plan_destroy(h))
