"""CPU: the host side of the per-parameter statistics (FusedAdamW(grad_stats_every=N), --grad_stats_every): the slot / unit table
cut from an arena's layout, the option's validation and what it allocates, the trainer flags, and the data-parallel step's choice of
the reduce-first path.  The kernel is in tests/test_param_stats_gpu.py."""
import importlib.util
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRAINERS = {"full": "train_mmbart_enc_self_face_name_ids_retrieve_crossattn_bart_guide_match.py",
            "onlyvis": "run_train_mmbart_enc_self_onlyvis_retrieve_crossattn.py"}


class _Small(torch.nn.Module):
    """a tied parameter (emb under two names), a fused group whose members are adjacent and start unaligned (7 and 5003 elements),
    a slot with padded rows (emb: 10 rows padded to 32), and a parameter longer than two units"""

    def __init__(self):
        super().__init__()
        self.emb = torch.nn.Parameter(torch.randn(10, 6))
        self.a = torch.nn.Parameter(torch.randn(7))
        self.b = torch.nn.Parameter(torch.randn(5003))
        self.c = torch.nn.Parameter(torch.randn(3, 3))
        self.big = torch.nn.Parameter(torch.randn(4096 * 2 + 1))
        self.head = self.emb

    def arena_groups(self):
        return [[self.a, self.b, self.c]]


def _arena():
    from vacnic_amd.arena import ParamArena
    m = _Small()
    return m, ParamArena(m, "cpu", pad_rows={id(m.emb): 32})


def test_stats_table_covers_every_parameter_once_and_nothing_else(built_lib):
    from vacnic_amd.arena import stats_table
    m, arena = _arena()
    t = stats_table(arena)
    want = sorted((arena.slots[id(p)][0], p.numel()) for p in (m.emb, m.a, m.b, m.c, m.big))
    assert t.slots == want and t.nslot == 5, "one slot per parameter, the tied one once"
    oa, ob, oc = (arena.slots[id(p)][0] for p in (m.a, m.b, m.c))
    assert ob == oa + 7 and oc == ob + 5003 and ob % 4 and oc % 4, "the fused group's members are adjacent and unaligned"
    assert arena.slots[id(m.emb)][2] == 32 * 6 > m.emb.numel(), "the padded slot has padding"
    uo, ul, su = t.unit_off.tolist(), t.unit_len.tolist(), t.slot_unit.tolist()
    assert t.unit_off.dtype == torch.int64 and t.unit_len.dtype == torch.int32 and t.slot_unit.dtype == torch.int64
    assert su[0] == 0 and su[-1] == t.nunit == len(uo) and len(su) == t.nslot + 1
    covered = torch.zeros(arena.n, dtype=torch.int32)
    for s, (o, n) in enumerate(t.slots):
        pos = o
        assert su[s + 1] > su[s]
        for u in range(su[s], su[s + 1]):
            assert uo[u] == pos and 1 <= ul[u] <= 4096, "units tile the slot in order"
            pos += ul[u]
            covered[uo[u]:uo[u] + ul[u]] += 1
        assert pos == o + n, "and end where the slot ends: none crosses into the next"
    inside = torch.zeros(arena.n, dtype=torch.int32)
    for o, n in want:
        inside[o:o + n] = 1
    assert torch.equal(covered, inside), "gaps, padded rows and the tail are in no unit; every element of a parameter in exactly one"
    assert int(inside.sum()) < arena.n
    assert t.slot_unit[-1] - t.slot_unit[-2] == 3, "4096 * 2 + 1 elements: three units"
    small = stats_table(arena, unit=100)
    assert max(small.unit_len.tolist()) == 100 and small.slots == t.slots
    dev = t.to("cpu")
    assert dev.nslot == t.nslot and dev.nunit == t.nunit and torch.equal(dev.unit_off, t.unit_off)
    with pytest.raises(ValueError):
        stats_table(arena, unit=4097)


def test_stats_table_rejects_overlapping_slots(built_lib):
    from vacnic_amd.arena import stats_table_from_slots
    with pytest.raises(ValueError, match="overlaps"):
        stats_table_from_slots([(0, 10), (9, 4)])
    t = stats_table_from_slots([(20, 5), (0, 1), (1, 3)])
    assert t.slots == [(0, 1), (1, 3), (20, 5)] and t.unit_off.tolist() == [0, 1, 20] and t.unit_len.tolist() == [1, 3, 5]


class _A:
    device, n = torch.device("cpu"), 8

    def init_optimizer_state(self):
        pass


def test_option_validation_and_off_means_no_buffers(built_lib):
    from vacnic_amd.training import FusedAdamW
    with pytest.raises(ValueError, match="grad_stats_every"):
        FusedAdamW(_A(), lr=1e-4, grad_stats_every=-1)
    for off in (None, 0):
        opt = FusedAdamW(_A(), lr=1e-4, grad_stats_every=off)
        assert opt.grad_stats_every == 0 and opt._stats is None
        with pytest.raises(RuntimeError, match="grad_stats_every=0"):
            opt.grad_stats([])
    opt = FusedAdamW(_A(), lr=1e-4)
    assert opt.grad_stats_every == 0 and opt._stats is None
    assert not [k for k, v in vars(opt).items() if "stats" in k and k != "grad_stats_every" and v is not None]


def test_option_allocates_in_the_constructor_and_refuses_the_range_wise_step(built_lib):
    from vacnic_amd.training import FusedAdamW
    m, arena = _arena()
    opt = FusedAdamW(arena, lr=1e-4, grad_stats_every=3)
    tab, work, out_f, out_i, stamp = opt._stats
    assert opt.grad_stats_every == 3 and tab.nslot == 5
    assert work.numel() == 24 * tab.nunit and tuple(out_f.shape) == (5, 4) and tuple(out_i.shape) == (5, 2)
    assert out_i.dtype == torch.int64 and stamp.tolist() == [0, 0, 0, 0]
    with pytest.raises(RuntimeError, match="grad_stats_every"):
        opt.begin_step()
    rep = opt.grad_stats(m.named_parameters())
    assert rep["fires"] == 0 and rep["params"] == {}
    assert "grad_stats" not in "".join(opt.state_dict()), "checkpoints carry nothing new"


def _load(fname):
    spec = importlib.util.spec_from_file_location("trainer_stats_" + fname[:3], os.path.join(ROOT, fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("which", sorted(TRAINERS))
def test_trainer_flag_and_default(built_lib, which):
    from vacnic_amd.training import TrainArgs
    assert TrainArgs().grad_stats_every == 0
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_trainer_flags.json")))
    ref = {v["script"]: v for v in ref.values()}[TRAINERS[which]]
    mod = _load(TRAINERS[which])
    args = mod.parser.parse_args(ref["argv"])                      # the reference's flag lines parse unchanged, the option off
    assert args.grad_stats_every == 0 and mod.train_args(args, 100).grad_stats_every == 0
    args = mod.parser.parse_args(ref["argv"] + ["--grad_stats_every", "50"])
    assert args.grad_stats_every == 50 and mod.train_args(args, 100).grad_stats_every == 50
    args = mod.parser.parse_args(ref["argv"] + ["--grad_stats_every", "-2"])
    with pytest.raises(ValueError, match="grad_stats_every"):
        mod.train_args(args, 100)


class _StubOpt:
    def __init__(self, **kw):
        self.calls = []
        vars(self).update(kw)

    def step(self, clip_norm=None):
        self.calls.append(("step", clip_norm))

    def begin_step(self):
        self.calls.append(("begin_step",))

    def step_range(self, start, end):
        self.calls.append(("step_range", start, end))


class _StubDDP:
    """the fields DistributedDataParallel.reduce_and_step reads, with a reducer that only keeps count"""

    def __init__(self):
        from vacnic_amd.ddp import DistributedDataParallel
        self.active, self.native, self.reduced = True, object(), 0
        self.order, self.bucket_end = [0, 8], {0: 8, 8: 16}
        self.tracker = type("T", (), {"buckets": [(0, 8), (8, 16)]})()
        self.reduce_and_step = DistributedDataParallel.reduce_and_step.__get__(self)

    def reduce_gradients(self):
        self.reduced += 1

    def _launch_bucket(self, start):
        pass

    def _wait_bucket(self, start):
        pass

    def _finish(self):
        pass


def test_reduce_and_step_reduces_first_and_steps_once_with_the_option(built_lib):
    w, opt = _StubDDP(), _StubOpt(grad_stats_every=5)
    w.reduce_and_step(opt, None)
    assert opt.calls == [("step", None)] and w.reduced == 1, "one whole step after the whole reduce, never begin_step()"
    w, opt = _StubDDP(), _StubOpt(grad_stats_every=0)              # control: without the option the bucket-wise path is taken
    w.reduce_and_step(opt, None)
    assert opt.calls == [("begin_step",), ("step_range", 0, 8), ("step_range", 8, 16)] and w.reduced == 0

