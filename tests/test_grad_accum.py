"""CPU: the host side of gradient accumulation — the trainers' --grad_accum_steps flag, the schedule it sizes, the truncation of
an epoch to whole optimizer steps, TrainArgs, and every refusal that needs no device.  The kernels, the optimizer and the trainer
run in tests/test_grad_accum_gpu.py."""
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


def _load(fname):
    spec = importlib.util.spec_from_file_location("trainer_accum_" + fname[:3], os.path.join(ROOT, fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference_flags():
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_trainer_flags.json")))
    by_script = {v["script"]: v for v in ref.values()}
    return {which: by_script[script] for which, script in TRAINERS.items()}


class _Arena:
    """what FusedAdamW's constructor touches of a ParamArena"""
    device, n = torch.device("cpu"), 8

    def init_optimizer_state(self):
        pass


@pytest.mark.parametrize("which", sorted(TRAINERS))
def test_trainer_flag_and_the_schedule_it_sizes(built_lib, which):
    from vacnic_amd.training import TrainArgs
    assert TrainArgs().grad_accum_steps == 1
    mod = _load(TRAINERS[which])
    ref = _reference_flags()[which]
    args = mod.parser.parse_args(ref["argv"])                      # the reference's flag lines parse unchanged, one batch per step
    assert args.grad_accum_steps == 1
    targs = mod.train_args(args, 100)
    assert targs.grad_accum_steps == 1 and targs.num_training_steps == 100
    args = mod.parser.parse_args(ref["argv"] + ["--grad_accum_steps", "3"])
    assert args.grad_accum_steps == 3
    targs = mod.train_args(args, 100)
    assert targs.grad_accum_steps == 3 and targs.num_training_steps == 33
    for bad in ("0", "-2"):
        with pytest.raises(ValueError, match="grad_accum_steps"):
            mod.train_args(mod.parser.parse_args(ref["argv"] + ["--grad_accum_steps", bad]), 100)


@pytest.mark.parametrize("which", sorted(TRAINERS))
def test_an_epoch_uses_whole_optimizer_steps(built_lib, which):
    mod = _load(TRAINERS[which])
    assert mod.accum_epoch_steps(5, 2) == 4
    assert mod.accum_epoch_steps(4, 2) == 4
    assert mod.accum_epoch_steps(7, 1) == 7
    with pytest.raises(ValueError, match="no whole optimizer step"):
        mod.accum_epoch_steps(1, 2)


def test_optimizer_refusals(built_lib):
    from vacnic_amd.training import FusedAdamW
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="accum_steps"):
            FusedAdamW(_Arena(), lr=1e-4, accum_steps=bad)
    with pytest.raises(ValueError, match="all-reduces the gradient arena in place"):
        FusedAdamW(_Arena(), lr=1e-4, accum_steps=2, world_size=2)
    opt = FusedAdamW(_Arena(), lr=1e-4, accum_steps=2)
    assert opt.accum_steps == 2 and opt.accum.tolist() == [0, 0, 0, 0] and opt.accum.dtype == torch.int64
    with pytest.raises(RuntimeError, match="accum_steps > 1"):
        opt.begin_step()
    assert opt.accum_report() == {"accum_steps": 2, "pending": 0, "groups": 0}
    off = FusedAdamW(_Arena(), lr=1e-4)
    assert off.accum_steps == 1 and off.accum is None, "off: no buffer, the launches of before"
    with pytest.raises(RuntimeError, match="accum_steps=1"):
        off.accum_report()
    assert FusedAdamW(_Arena(), lr=1e-4, world_size=2).accum is None     # accum_steps == 1 with more ranks stays allowed


def test_checkpoint_refusals(built_lib):
    """a save in the middle of a group and a load with another k raise before anything is written; the counters come back."""
    from vacnic_amd import checkpoint
    from vacnic_amd.training import FusedAdamW

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.arange(8.0))

    class Arena(_Arena):
        def __init__(self, net):
            self.flat32 = net.w.data
            self.grad = torch.ones(8)
            self.exp_avg, self.exp_avg_sq = torch.zeros(8), torch.zeros(8)
            self.slots = {id(net.w): (0, 8, 8)}

        def refresh_shadow(self):
            pass

    net = Net()
    net.arena = Arena(net)
    opt = FusedAdamW(net.arena, lr=1e-4, accum_steps=3)
    opt.accum.copy_(torch.tensor([2, 1, 4, 0]))
    with pytest.raises(RuntimeError, match="middle of an accumulation group: 1 of 3"):
        checkpoint.optimizer_state(net, opt)
    opt.accum.copy_(torch.tensor([0, 0, 5, 0]))
    opt.hyper.copy_(torch.tensor([1e-5, 5.0]))
    ck = {"model": checkpoint.model_state(net), "optimizer": checkpoint.optimizer_state(net, opt),
          "schedule": {"accum_steps": 3}, "meta": {"format": checkpoint.FORMAT, "step": 15}}
    assert ck["optimizer"]["groups"] == 5 and ck["optimizer"]["step"] == 5
    other = FusedAdamW(net.arena, lr=1e-4, accum_steps=2)
    with pytest.raises(ValueError, match=r"accum_steps=3.*accum_steps=2"):
        checkpoint.load_checkpoint(ck, net, other)
    plain = FusedAdamW(net.arena, lr=1e-4)
    with pytest.raises(ValueError, match=r"accum_steps=3.*accum_steps=1"):
        checkpoint.load_checkpoint(ck, net, plain)
    with pytest.raises(ValueError, match=r"accum_steps=1.*accum_steps=2"):    # absent in the file means 1
        checkpoint.load_checkpoint(dict(ck, schedule={}), net, other)
    assert other.accum.tolist() == [0, 0, 0, 0] and (net.arena.grad == 1).all(), "a refused load writes nothing"
    same = FusedAdamW(net.arena, lr=1e-4, accum_steps=3)
    same.accum.copy_(torch.tensor([2, 2, 0, 0]))
    assert checkpoint.load_checkpoint(ck, net, same)["step"] == 15
    assert same.accum.tolist() == [0, 0, 5, 0] and same.hyper[1].item() == 5.0
    assert (net.arena.grad == 0).all(), "a restored run begins a group: nothing is pending"


def test_train_step_refuses_a_flag_the_optimizer_does_not_share(built_lib, monkeypatch):
    """both refusals sit in train_step's own checks, after backward: forward and backward are stubbed out (no device here)."""
    from vacnic_amd import ops, streams, training
    from vacnic_amd.training import FusedAdamW, TrainArgs

    class Net:
        training = True

    class Loss:
        device = torch.device("cpu")

        def backward(self, _):
            pass
    monkeypatch.setattr(training, "forward_losses", lambda *a, **k: (Loss(), None, None))
    monkeypatch.setattr(ops, "begin_step", lambda: None)
    monkeypatch.setattr(ops, "const_one", lambda d: None)
    monkeypatch.setattr(ops, "flush_wgrads", lambda: None)
    monkeypatch.setattr(streams, "join_all", lambda **k: None)
    with pytest.raises(ValueError, match=r"grad_accum_steps=2 .* accum_steps=1"):
        training.train_step(Net(), None, FusedAdamW(_Arena(), lr=1e-4), {}, TrainArgs(grad_accum_steps=2))
    with pytest.raises(ValueError, match=r"grad_accum_steps=1 .* accum_steps=2"):
        training.train_step(Net(), None, FusedAdamW(_Arena(), lr=1e-4, accum_steps=2), {}, TrainArgs())

    class Wrapped(training.DistributedDataParallel):
        def __init__(self):                       # (no process group: only what train_step reads before its checks)
            self.module, self.active, self.native = Net(), True, None
    with pytest.raises(ValueError, match="active DistributedDataParallel"):
        training.train_step(Wrapped(), None, FusedAdamW(_Arena(), lr=1e-4, accum_steps=2), {}, TrainArgs(grad_accum_steps=2))
