"""CPU: the host side of the moving average of the weights (FusedAdamW(ema_decay=...), --ema_decay / --ema_eval) — trainer
flags and their defaults, TrainArgs, argument validation on the host and in the C entry points (status, never an abort), and the
checkpoint rules on hand-made dicts with a small host arena.  The kernels are in tests/test_ema_gpu.py."""
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


def _load(fname, tag="trainer_ema_"):
    spec = importlib.util.spec_from_file_location(tag + os.path.basename(fname)[:3], os.path.join(ROOT, fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference_flags():
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_trainer_flags.json")))
    by_script = {v["script"]: v for v in ref.values()}
    return {which: by_script[script] for which, script in TRAINERS.items()}


# ------------------------------------------------------------------------------------------------------------------ flags
@pytest.mark.parametrize("which", sorted(TRAINERS))
def test_trainer_flags_and_defaults(built_lib, which):
    from vacnic_amd.training import TrainArgs
    assert TrainArgs().ema_decay == 0.0
    mod = _load(TRAINERS[which])
    ref = _reference_flags()[which]
    args = mod.parser.parse_args(ref["argv"])                      # the reference's flag lines parse unchanged, no average
    assert args.ema_decay == 0.0 and args.ema_eval is None
    assert mod.train_args(args, 100).ema_decay == 0.0
    full = _load(TRAINERS["full"])
    assert full.ema_eval(args) is False                            # nothing to evaluate with
    args = mod.parser.parse_args(ref["argv"] + ["--ema_decay", "0.999"])
    assert args.ema_decay == 0.999 and full.ema_eval(args) is True            # evaluation follows the average by default
    targs = mod.train_args(args, 100)
    assert targs.ema_decay == 0.999 and targs.num_training_steps == 100
    args = mod.parser.parse_args(ref["argv"] + ["--ema_decay", "0.999", "--ema_eval", "False"])
    assert args.ema_eval is False and full.ema_eval(args) is False and mod.train_args(args, 100).ema_decay == 0.999
    args = mod.parser.parse_args(ref["argv"] + ["--ema_eval", "True"])
    assert full.ema_eval(args) is False, "--ema_eval without --ema_decay has no average to use"
    for bad in ("1.0", "-0.1", "1.5", "nan"):
        with pytest.raises(ValueError, match="ema_decay"):
            mod.train_args(mod.parser.parse_args(ref["argv"] + ["--ema_decay", bad]), 100)


# ------------------------------------------------------------------------------------------------------------- validation
class _StubArena:
    device, n = torch.device("cpu"), 8
    exp_avg = exp_avg_sq = None

    def __init__(self):
        self.flat32 = torch.arange(8, dtype=torch.float32)
        self.ema = None

    def init_optimizer_state(self):
        pass

    def init_ema(self):
        self.ema = self.flat32.clone()


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")])
def test_decay_outside_the_open_unit_interval_is_rejected(built_lib, bad):
    from vacnic_amd.training import FusedAdamW
    a = _StubArena()
    with pytest.raises(ValueError, match="ema_decay"):
        FusedAdamW(a, lr=1e-4, ema_decay=bad)
    assert a.ema is None, "nothing is allocated for a rejected decay"


def test_average_is_off_by_default_and_allocated_at_construction(built_lib):
    from vacnic_amd.training import FusedAdamW
    a = _StubArena()
    opt = FusedAdamW(a, lr=1e-4)
    assert opt.ema_decay is None and a.ema is None and "ema" not in opt.state_dict()
    with pytest.raises(RuntimeError, match="without ema_decay"):
        opt.swap_ema()
    with pytest.raises(RuntimeError, match="without ema_decay"):
        with opt.ema_weights():
            pass
    a = _StubArena()
    opt = FusedAdamW(a, lr=1e-4, ema_decay=0.999)
    assert opt.ema_decay == 0.999 and opt.ema_warmup is True and opt.ema_swapped is False
    assert a.ema is not a.flat32 and torch.equal(a.ema, a.flat32), "the average starts as a copy of the weights, before any step"
    assert FusedAdamW(_StubArena(), lr=1e-4, ema_decay=0.5, ema_warmup=False).ema_warmup is False


def _ema_call(**over):
    """vacnic_adamw_ema with plausible (never dereferenced: validation comes before any launch) arguments"""
    from vacnic_amd import _lib
    kw = dict(stream=None, p=1024, g=2048, m=3072, v=4096, p_bf16=None, hyper=512, n=8, beta1=0.9, beta2=0.999, eps=1e-8,
              grad_scale=1.0, zero_grad=1, clip_coef=None, seg_start=None, seg=None, first_seg=None, nseg=0, nblocks=0, elem_base=0,
              skip=None, weight_decay=0.01, ema=5120, ema_decay=0.999, ema_warmup=1)
    kw.update(over)
    _lib.call_struct("vacnic_adamw_ema", **kw)


def test_bad_arguments_return_status_not_abort(built_lib):
    from vacnic_amd import _lib
    with pytest.raises(ValueError, match="null ema"):
        _ema_call(ema=None)
    with pytest.raises(ValueError, match="multiple of 4"):
        _ema_call(n=6)
    for bad in (0.0, 1.0, -0.1, 2.0, float("nan")):
        with pytest.raises(ValueError, match=r"ema_decay.*\(0, 1\)"):
            _ema_call(ema_decay=bad)
    with pytest.raises(ValueError, match="null operand"):
        _ema_call(p=None)
    with pytest.raises(ValueError, match="16-byte aligned"):
        _ema_call(ema=5124)
    with pytest.raises(ValueError, match="null group table"):
        _ema_call(seg_start=64)                                    # a table given in part
    with pytest.raises(ValueError, match="null operand"):
        _lib.call("vacnic_ema_swap", 1024, None, None, 8, None)
    with pytest.raises(ValueError, match="multiple of 4"):
        _lib.call("vacnic_ema_swap", 1024, 2048, None, 6, None)
    with pytest.raises(ValueError, match="same buffer"):
        _lib.call("vacnic_ema_swap", 1024, 1024, None, 8, None)


# ------------------------------------------------------------------------------------------------------------ checkpoints
class _Tiny(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.fc = torch.nn.Linear(6, 4)
        self.ln = torch.nn.LayerNorm(4)


def _tiny(seed, ema_decay=None):
    from vacnic_amd.arena import ParamArena
    from vacnic_amd.training import FusedAdamW
    net = _Tiny(seed)
    net.arena = ParamArena(net, "cpu")
    return net, FusedAdamW(net.arena, lr=1e-3, ema_decay=ema_decay)


def _handmade(with_ema, decay=0.9):
    """a checkpoint dict written by hand: weights w, moments, and (with_ema) an average that differs from the weights"""
    shapes = {"fc.weight": (4, 6), "fc.bias": (4,), "ln.weight": (4,), "ln.bias": (4,)}
    g = torch.Generator().manual_seed(5)
    t = lambda: {k: torch.randn(*s, generator=g) for k, s in shapes.items()}      # noqa: E731
    ck = {"model": t(), "optimizer": {"exp_avg": t(), "exp_avg_sq": {k: v.abs() for k, v in t().items()}, "lr": 1e-3, "step": 3},
          "schedule": {"base_lr": 1e-3}, "meta": {"format": 1, "step": 3}}
    if with_ema:
        ck["optimizer"]["ema"] = t()
        ck["schedule"].update(ema_decay=decay, ema_warmup=True)
    return ck


def _flat(net, named):
    a = net.arena
    out = torch.zeros(a.n)
    for name, p in net.named_parameters():
        o, n, _ = a.slots[id(p)]
        out[o:o + n] = named[name].reshape(-1)
    return out


def test_checkpoint_with_an_average_restores_it(built_lib):
    from vacnic_amd import checkpoint
    ck = _handmade(True, decay=0.9)
    net, opt = _tiny(1, ema_decay=0.9999)                           # another decay than the file's: allowed, the optimizer's holds
    assert checkpoint.load_checkpoint(ck, net, opt)["step"] == 3
    assert torch.equal(net.arena.flat32, _flat(net, ck["model"]))
    assert torch.equal(net.arena.ema, _flat(net, ck["optimizer"]["ema"]))
    assert not torch.equal(net.arena.ema, net.arena.flat32)
    assert torch.equal(net.arena.exp_avg, _flat(net, ck["optimizer"]["exp_avg"]))
    assert opt.ema_decay == 0.9999 and opt.hyper.tolist() == [pytest.approx(1e-3), 3.0]


def test_checkpoint_without_an_average_starts_it_from_the_restored_weights(built_lib):
    from vacnic_amd import checkpoint
    ck = _handmade(False)
    net, opt = _tiny(1, ema_decay=0.9)
    before = net.arena.ema.clone()
    checkpoint.load_checkpoint(ck, net, opt)
    assert torch.equal(net.arena.ema, _flat(net, ck["model"])) and torch.equal(net.arena.ema, net.arena.flat32)
    assert not torch.equal(net.arena.ema, before)
    assert net.arena.ema.data_ptr() != net.arena.flat32.data_ptr()
    # a weights-only file (no optimizer entry at all): the same rule
    net, opt = _tiny(2, ema_decay=0.9)
    checkpoint.load_checkpoint({"model": ck["model"], "meta": ck["meta"]}, net, opt)
    assert torch.equal(net.arena.ema, _flat(net, ck["model"]))


def test_optimizer_without_an_average_ignores_a_stored_one(built_lib):
    from vacnic_amd import checkpoint
    ck = _handmade(True)
    net, opt = _tiny(1)
    checkpoint.load_checkpoint(ck, net, opt)
    assert net.arena.ema is None and opt.ema_decay is None
    assert torch.equal(net.arena.flat32, _flat(net, ck["model"])) and torch.equal(net.arena.exp_avg_sq, _flat(net, ck["optimizer"]["exp_avg_sq"]))


def test_weights_ema_loads_the_average_as_the_weights(built_lib):
    from vacnic_amd import checkpoint
    ck = _handmade(True)
    net, _ = _tiny(1)
    checkpoint.load_checkpoint(ck, net, weights="ema")              # inference: no optimizer
    want = _flat(net, ck["optimizer"]["ema"])
    assert torch.equal(net.arena.flat32, want) and torch.equal(net.fc.weight.data, ck["optimizer"]["ema"]["fc.weight"])
    assert torch.equal(net.arena.flat16, want.to(torch.bfloat16)), "the shadow follows"
    with pytest.raises(KeyError, match="no moving average"):
        checkpoint.load_checkpoint(_handmade(False), net, weights="ema")
    with pytest.raises(KeyError, match="no moving average"):
        checkpoint.load_checkpoint({"model": ck["model"], "meta": ck["meta"]}, net, weights="ema")
    assert torch.equal(net.arena.flat32, want), "a refused load leaves the model alone"
    with pytest.raises(ValueError, match="'model' or 'ema'"):
        checkpoint.load_checkpoint(ck, net, weights="average")


def test_saving_stores_the_average_and_refuses_inside_the_swap(built_lib, tmp_path):
    from vacnic_amd import checkpoint, ops
    net, opt = _tiny(1, ema_decay=0.9)
    net.arena.ema.mul_(0.5)                                         # an average that differs from the weights
    rng = (ops.Rng.base, ops.Rng.counter)
    ck = checkpoint.save_checkpoint(str(tmp_path / "a.pt"), net, opt, step=2)
    assert ck["schedule"]["ema_decay"] == 0.9 and ck["schedule"]["ema_warmup"] is True
    assert sorted(ck["optimizer"]["ema"]) == sorted(ck["optimizer"]["exp_avg"]) == ["fc.bias", "fc.weight", "ln.bias", "ln.weight"]
    assert torch.equal(ck["optimizer"]["ema"]["fc.weight"], 0.5 * net.fc.weight.data)
    net2, opt2 = _tiny(9, ema_decay=0.9)
    checkpoint.load_checkpoint(str(tmp_path / "a.pt"), net2, opt2)
    (ops.Rng.base, ops.Rng.counter) = rng
    assert torch.equal(net2.arena.ema, net.arena.ema) and torch.equal(net2.arena.flat32, net.arena.flat32)
    plain_net, plain = _tiny(1)
    ck = checkpoint.save_checkpoint(str(tmp_path / "b.pt"), plain_net, plain, step=2)
    assert "ema" not in ck["optimizer"] and "ema_decay" not in ck["schedule"], "without the option the file is what it was"
    opt.ema_swapped = True                                          # what swap_ema() / ema_weights() set (they launch a kernel)
    with pytest.raises(RuntimeError, match="inside ema_weights"):
        checkpoint.save_checkpoint(str(tmp_path / "c.pt"), net, opt, step=2)
    assert not (tmp_path / "c.pt").exists()
    with pytest.raises(RuntimeError, match="swapped in"):
        opt.step()
    with pytest.raises(RuntimeError, match="swapped"):
        checkpoint.load_checkpoint(str(tmp_path / "a.pt"), net, opt)


def test_refused_load_leaves_weights_and_average_alone(built_lib):
    """every refusal of load_checkpoint comes before its first write: another parameter-group spec, a wrong shape"""
    from vacnic_amd import checkpoint
    net, opt = _tiny(1, ema_decay=0.9)
    net.arena.ema.mul_(0.5)
    w0, e0, m0 = net.arena.flat32.clone(), net.arena.ema.clone(), net.arena.exp_avg.clone()
    ck = _handmade(True)
    ck["schedule"]["param_groups"] = [{"match": "fc", "lr_scale": None, "weight_decay": 0.0, "frozen": None}]
    with pytest.raises(ValueError, match="param_groups"):
        checkpoint.load_checkpoint(ck, net, opt)
    ck = _handmade(True)
    ck["model"]["ln.bias"] = torch.zeros(5)
    with pytest.raises(ValueError, match="shape mismatch"):
        checkpoint.load_checkpoint(ck, net, opt)
    assert torch.equal(net.arena.flat32, w0) and torch.equal(net.arena.ema, e0) and torch.equal(net.arena.exp_avg, m0)


def test_average_exported_as_an_inference_checkpoint(built_lib, tmp_path):
    """checkpoint.ema_as_model / tools/export_ema.py: a file whose weights ARE the average, read by a loader that knows nothing of
    averages (the stand-alone caption generator loads with load_checkpoint(ck, model))."""
    from vacnic_amd import checkpoint
    ck = _handmade(True)
    ck["meta"]["config"] = {"d_model": 4}
    out = checkpoint.ema_as_model(ck)
    assert sorted(out) == ["meta", "model"] and out["meta"] == {"format": 1, "step": 3, "config": {"d_model": 4}, "weights": "ema"}
    assert all(torch.equal(out["model"][k], ck["optimizer"]["ema"][k]) for k in ck["optimizer"]["ema"])
    assert "weights" not in ck["meta"] and not torch.equal(ck["model"]["fc.weight"], out["model"]["fc.weight"]), "the source dict is not edited"
    with pytest.raises(KeyError, match="no moving average"):
        checkpoint.ema_as_model(_handmade(False))
    spec = importlib.util.spec_from_file_location("export_ema_tool", os.path.join(ROOT, "tools", "export_ema.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src, dst = str(tmp_path / "run.pt"), str(tmp_path / "run_ema.pt")
    torch.save(ck, src)
    tool.export(src, dst)
    net, _ = _tiny(1)
    assert checkpoint.load_checkpoint(dst, net)["weights"] == "ema"          # the plain call, as the generator makes it
    assert torch.equal(net.arena.flat32, _flat(net, ck["optimizer"]["ema"]))
    with pytest.raises(ValueError, match="same file"):
        tool.export(src, src)
    torch.save(_handmade(False), src)
    with pytest.raises(KeyError, match="no moving average"):
        tool.export(src, str(tmp_path / "none.pt"))
    assert not (tmp_path / "none.pt").exists()
