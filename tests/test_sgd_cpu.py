"""No-GPU checks of HipSGD's host side: what the constructor refuses, that the warm-up values stay out of param_groups and
checkpoints, that checkpoints pass between HipSGD and torch.optim.SGD, get_optimizer's dispatch on `training.optimizer`,
the script's reading of the config, and the header.  Nothing is launched here; the kernel is covered by
tests/test_gpu_sgd.py."""
import importlib.util
import os

import pytest
import torch
from torch import nn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KW = dict(lr=1e-3, weight_decay=1e-2, patience=3, factor=0.5)


def _params():
    return [nn.Parameter(torch.zeros(4, 3)), nn.Parameter(torch.zeros(5))]


@pytest.mark.parametrize("bad", [dict(dampening=0.1), dict(maximize=True), dict(momentum=0.0), dict(momentum=0.0, nesterov=True),
                                 dict(lr=-1e-3), dict(lr=float("nan")), dict(momentum=-0.1), dict(momentum=float("inf")),
                                 dict(weight_decay=-1.0), dict(weight_decay=float("nan")),
                                 dict(warmup_steps=-1), dict(warmup_steps=2.5), dict(warmup_steps=float("nan")),
                                 dict(warmup_momentum=1.0), dict(warmup_momentum=-0.1), dict(warmup_momentum=float("nan")),
                                 dict(warmup_lr_scale=1.5), dict(warmup_lr_scale=-0.1), dict(warmup_lr_scale=float("nan")),
                                 dict(max_grad_norm=0.0), dict(ema_decay=1.0), dict(ema_tau=-1.0)])
def test_constructor_refusals(bad):
    from src.training.fused_sgd import HipSGD
    with pytest.raises(ValueError):
        HipSGD(_params(), **{"lr": 1e-3, **bad})


def test_momentum_zero_is_allowed_without_nesterov_and_group_keys_are_checked_too():
    from src.training.fused_sgd import HipSGD
    opt = HipSGD(_params(), lr=1e-3, momentum=0.0, nesterov=False)
    assert opt.param_groups[0]["momentum"] == 0.0
    with pytest.raises(ValueError, match="nesterov"):
        HipSGD([dict(params=_params(), momentum=0.0)], lr=1e-3)
    with pytest.raises(ValueError, match="dampening"):
        HipSGD([dict(params=_params(), dampening=0.5)], lr=1e-3)


def test_param_groups_carry_torch_sgd_keys_and_warmup_lives_outside_them():
    from src.training.fused_sgd import HipSGD
    opt = HipSGD(_params(), lr=1e-3, weight_decay=5e-4, warmup_steps=100, warmup_momentum=0.7, warmup_lr_scale=0.2,
                 max_grad_norm=2.0, ema_decay=0.99)
    twin = torch.optim.SGD(_params(), lr=1e-3)
    assert set(opt.param_groups[0]) >= set(twin.param_groups[0]) and opt.param_groups[0]["capturable"] is True
    g = opt.param_groups[0]
    assert (g["momentum"], g["dampening"], g["nesterov"], g["maximize"], g["weight_decay"]) == (0.937, 0, True, False, 5e-4)
    assert (opt.warmup_steps, opt.warmup_momentum, opt.warmup_lr_scale) == (100, 0.7, 0.2)
    for key in ("warmup_steps", "warmup_momentum", "warmup_lr_scale", "max_grad_norm", "ema_decay"):
        assert key not in g and key not in opt.defaults
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and "warmup" not in repr(sd)
    for name, bad in (("warmup_steps", -3), ("warmup_momentum", 1.0), ("warmup_lr_scale", 2.0)):
        with pytest.raises(ValueError, match=name):
            setattr(opt, name, bad)                 # a schedule's new value is validated like the constructor's
    assert (opt.warmup_steps, opt.warmup_momentum, opt.warmup_lr_scale) == (100, 0.7, 0.2)
    opt.warmup_steps = 0
    assert opt.warmup_steps == 0
    assert opt._hyper_values(g) == (1e-3, 0.937, 5e-4, 1.0, 0.0, 0.7, 0.2) and len(opt._hyper_values(g)) == opt._HYPER


def test_state_dicts_pass_between_hipsgd_and_torch_sgd():
    from src.training.fused_sgd import HipSGD
    opt = HipSGD(_params(), lr=1e-3, momentum=0.9, weight_decay=5e-4, warmup_steps=10)
    twin = torch.optim.SGD(_params(), lr=0.5)
    twin.load_state_dict(opt.state_dict())
    assert twin.param_groups[0]["lr"] == 1e-3 and twin.param_groups[0]["nesterov"] is True
    ps = _params()
    theirs = torch.optim.SGD(ps, lr=0.25, momentum=0.8, nesterov=True, weight_decay=1e-4)
    for p in ps:
        p.grad = torch.ones_like(p)
    theirs.step()
    back = HipSGD(_params(), lr=1e-3)
    back.load_state_dict(theirs.state_dict())
    g = back.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g["capturable"]) == (0.25, 0.8, 1e-4, True)
    st = back.state[back.param_groups[0]["params"][0]]
    assert "step" not in st and torch.equal(st["momentum_buffer"], torch.ones(4, 3))
    bad = theirs.state_dict()
    bad["param_groups"][0]["dampening"] = 0.5
    with pytest.raises(ValueError, match="dampening"):
        HipSGD(_params(), lr=1e-3).load_state_dict(bad)


def test_both_optimizers_share_one_base_and_the_old_import_path_works():
    from src.training.fused_adamw import DeviceGradScaler, HipAdamW, HipFusedOptimizer      # noqa: F401
    from src.training.fused_sgd import HipSGD
    assert issubclass(HipAdamW, HipFusedOptimizer) and issubclass(HipSGD, HipFusedOptimizer)
    for name in ("sync_hyper", "finish_capture", "restore_capture", "ema_prepare", "attach_ema_buffers", "_build", "_plan",
                 "_clipped_step", "_launch", "_init_state"):
        assert getattr(HipSGD, name) is getattr(HipAdamW, name) is getattr(HipFusedOptimizer, name), name
    assert "step" in vars(HipFusedOptimizer)        # (torch wraps `step` per class on construction: not comparable by identity)
    assert HipSGD._STATE == ("momentum_buffer",) and HipAdamW._STATE == ("exp_avg", "exp_avg_sq")


def test_dtensor_parameters_refuse_clip_and_ema(monkeypatch):
    from src.training import fused_adamw
    from src.training.fused_sgd import HipSGD

    class FakeDTensor(nn.Parameter):
        pass
    monkeypatch.setattr(fused_adamw, "DTensor", FakeDTensor)
    ps = [FakeDTensor(torch.zeros(3))]
    with pytest.raises(ValueError, match="DTensor"):
        HipSGD(ps, lr=1e-3, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="DTensor"):
        HipSGD(ps, lr=1e-3, ema_decay=0.9)
    opt = HipSGD(ps, lr=1e-3)
    assert not opt._step_supports_amp_scaling          # sharded: the scaler unscales and agrees on found_inf across ranks
    assert HipSGD(_params(), lr=1e-3)._step_supports_amp_scaling


# ------------------------------------------------------------------------------------------------ get_optimizer
@pytest.fixture
def spies(monkeypatch):
    """HipAdamW / HipSGD replaced by recorders, GPU parameters pretended (as tests/test_grad_clip_cpu.py does)"""
    from src.training import fused_adamw, fused_sgd
    calls = []

    def spy(name, base):
        class Spy(base):
            def __init__(self, params, **kw):
                calls.append((name, kw))
                super().__init__(params, **kw)
        return Spy
    monkeypatch.setattr(fused_adamw, "HipAdamW", spy("adamw", fused_adamw.HipAdamW))
    monkeypatch.setattr(fused_sgd, "HipSGD", spy("sgd", fused_sgd.HipSGD))
    monkeypatch.setattr(nn.Parameter, "is_cuda", property(lambda self: True), raising=False)
    return calls


def test_adamw_builds_what_it_built_before(spies):
    from src.training.utils_train import get_optimizer
    model = nn.Linear(3, 2)
    for extra in (dict(), dict(optimizer="adamw"), dict(optimizer="AdamW", max_grad_norm=0.75)):
        del spies[:]
        opt, sched = get_optimizer(model, **KW, **extra)
        assert spies == [("adamw", dict(lr=1e-3, weight_decay=1e-2, max_grad_norm=extra.get("max_grad_norm")))]
        assert isinstance(sched, torch.optim.lr_scheduler.ReduceLROnPlateau) and sched.optimizer is opt
        assert "betas" in opt.param_groups[0]


def test_sgd_in_any_letter_case_builds_hipsgd_and_forwards_the_section(spies):
    from src.training.fused_sgd import HipSGD
    from src.training.utils_train import get_optimizer
    model = nn.Linear(3, 2)
    section = dict(momentum=0.9, nesterov=False, warmup_steps=300, warmup_momentum=0.5, warmup_lr_scale=0.1)
    opt, sched = get_optimizer(model, **KW, optimizer="SGD", sgd=section, max_grad_norm=2.0)
    assert spies == [("sgd", dict(lr=1e-3, weight_decay=1e-2, max_grad_norm=2.0, **section))]
    assert isinstance(opt, HipSGD) and sched.optimizer is opt and opt.warmup_steps == 300 and opt.max_grad_norm == 2.0
    opt, _ = get_optimizer(model, **KW, optimizer="sgd")
    g = opt.param_groups[0]
    assert isinstance(opt, HipSGD) and (g["momentum"], g["nesterov"], opt.warmup_steps) == (0.937, True, 0)


def test_native_master_shard_gets_hipsgd(spies, monkeypatch):
    from src.training import sharded_step
    from src.training.utils_train import get_optimizer

    class FakeShard:
        def __init__(self, model, precision):
            self.master = nn.Parameter(torch.zeros(7))
    monkeypatch.setattr(sharded_step, "ShardState", FakeShard)
    model = nn.Linear(3, 2)
    model._native_shard = {"state": None, "precision": "bfloat16"}
    opt, _ = get_optimizer(model, **KW, optimizer="sgd", sgd=dict(warmup_steps=5))
    assert spies == [("sgd", dict(lr=1e-3, weight_decay=1e-2, warmup_steps=5))]
    assert model._native_shard["optimizer"] is opt and opt.param_groups[0]["params"][0] is model._native_shard["state"].master


def test_unknown_names_and_misplaced_sections_raise():
    from src.training.utils_train import get_optimizer
    model = nn.Linear(3, 2)
    for name in ("lion", "", None, "adam"):
        with pytest.raises(ValueError, match="training.optimizer"):
            get_optimizer(model, **KW, optimizer=name)
    # a config switched back to "adamw" may keep its training.sgd section: it is not read (but still spell-checked)
    assert type(get_optimizer(model, **KW, optimizer="adamw", sgd=dict(momentum=0.9))[0]) is torch.optim.AdamW
    with pytest.raises(ValueError, match="training.sgd"):
        get_optimizer(model, **KW, optimizer="adamw", sgd=dict(momentun=0.9))
    with pytest.raises(ValueError, match="training.sgd"):
        get_optimizer(model, **KW, optimizer="sgd", sgd=dict(momentun=0.9))


def test_torch_fallback_is_torch_sgd_and_refuses_warmup_clip_and_ema():
    from src.training.ema import ModelEMA
    from src.training.utils_train import get_optimizer
    model = nn.Linear(3, 2)                         # CPU parameters: torch's optimizers
    opt, sched = get_optimizer(model, **KW, optimizer="sgd", sgd=dict(momentum=0.9, nesterov=False, warmup_steps=0))
    g = opt.param_groups[0]
    assert type(opt) is torch.optim.SGD and sched.optimizer is opt
    assert (g["lr"], g["weight_decay"], g["momentum"], g["nesterov"]) == (1e-3, 1e-2, 0.9, False)
    g = get_optimizer(model, **KW, optimizer="sgd")[0].param_groups[0]
    assert (g["momentum"], g["nesterov"]) == (0.937, True)
    assert type(get_optimizer(model, **KW)[0]) is torch.optim.AdamW
    with pytest.raises(ValueError, match="warmup_steps"):
        get_optimizer(model, **KW, optimizer="sgd", sgd=dict(warmup_steps=10))
    with pytest.raises(ValueError, match="max_grad_norm"):
        get_optimizer(model, **KW, optimizer="sgd", max_grad_norm=1.0)
    with pytest.raises(ValueError, match="HipSGD"):
        ModelEMA(model, opt)


def test_train_and_the_captured_route_accept_the_shared_base():
    from src.training.fused_sgd import HipSGD
    from src.training.train_model import CapturedTraining, train
    model = nn.Linear(3, 2)
    opt = HipSGD(model.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="HipSGD"):                 # a HipSGD, but without ema_decay: the text names both
        train(model=model, train_loader=None, val_loader=None, optimizer=opt, scheduler=None, criterion=None, initial_epoch=0,
              num_epochs=1, device="cpu", distributed_mode="ddp", ema=object())
    # CPU parameters are never capturable; what the fp16 rule looks at is the optimizer's class and its one group
    assert not CapturedTraining(model, None, opt, "float16").usable
    assert all(g["capturable"] for g in opt.param_groups)


# ------------------------------------------------------------------------------------------------ script and header
def test_script_passes_training_optimizer_and_training_sgd_through():
    path = os.path.join(ROOT, "custom-yolo-implmentation_amd", "scripts", "distributed_training.py")
    spec = importlib.util.spec_from_file_location("distributed_training_under_test", path)
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    assert script.optimizer_choice({"learning_rate": 1e-4}) == dict(optimizer="adamw", sgd=None)
    section = dict(momentum=0.9, nesterov=True, warmup_steps=1000, warmup_momentum=0.8, warmup_lr_scale=0.0)
    assert script.optimizer_choice({"optimizer": "sgd", "sgd": section}) == dict(optimizer="sgd", sgd=section)
    import inspect
    assert "**optimizer_choice(tr_cfg)" in inspect.getsource(script.main)
    # the shipped config names no optimizer (or "adamw", as the reference's does): reference numerics
    from src.utils.config_loader import load_config
    cfg = load_config(os.path.join(ROOT, "custom-yolo-implmentation_amd", "config.yaml"))
    assert script.optimizer_choice(cfg["training"])["optimizer"].lower() == "adamw"


def test_header_block_cites_the_reference_and_keeps_the_existing_prototypes():
    import re
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    block = next(b for b in text.split("/* ---- ") if b.startswith("SGD optimizer"))
    comment = block.split("*/")[0]
    for cite in ("config.yaml:65", "src/training/utils_train.py:34", "src/training/train_model.py:247-253"):
        assert cite in comment, cite
    assert re.search(r"\w+\.py:\d+", comment)
    assert "int yolo_sgd_step(const void* jobs_dev, int njobs, long nchunks, const double* hyper, float* step, " \
           "const float* grad_scale, const float* found_inf, const float* clip_state, hipStream_t st);" in block
    assert "int yolo_sgd_amp_step(" in block
    adamw = next(b for b in text.split("/* ---- ") if b.startswith("optimizer"))
    assert "int yolo_adamw_step(const void* jobs_dev, int njobs, long nchunks, const double* hyper, float* step, " \
           "const float* grad_scale, const float* found_inf, hipStream_t st);" in adamw
    from src.hipops import lib
    protos = lib.parse_header(os.path.join(ROOT, "include", "yolo_hip.h"))
    assert len(protos["yolo_sgd_step"][1]) == 9 and len(protos["yolo_sgd_amp_step"][1]) == 11


def test_native_shard_checkpoints_carry_the_momentum_buffer(tmp_path):
    """ShardState.full_optimizer_state_dict and load_checkpoint's native-shard branch name the state tensors through the
    optimizer (`momentum_buffer` for HipSGD, the two moments for HipAdamW): a fake one-rank shard over nn.Linear(3, 2),
    the state set by hand, out to a torch.optim.SGD-shaped state dict, through a file, and back into a fresh shard."""
    import types
    from src.training.fused_adamw import HipAdamW
    from src.training.fused_sgd import HipSGD
    from src.training.sharded_step import ShardState
    from src.training.utils_train import load_checkpoint

    def shard(model):
        ps = list(model.parameters())
        return types.SimpleNamespace(master=nn.Parameter(torch.zeros(8)), trainable=ps, slices=[(0, 6), (6, 2)], total=8,
                                     rank=0, shard_elems=8, flat_p=torch.zeros(8), gather_flat=lambda t: t.detach().clone())

    for make, names in ((lambda ps: HipSGD(ps, lr=1e-3, momentum=0.9), ("momentum_buffer",)),
                        (lambda ps: HipAdamW(ps, lr=1e-3), ("exp_avg", "exp_avg_sq"))):
        model = nn.Linear(3, 2)
        st = shard(model)
        opt = make([st.master])
        values = {k: torch.arange(8.0) + 10 * i + 1 for i, k in enumerate(names)}
        opt.state[st.master] = dict(step=torch.tensor(5.0), **values)
        sd = ShardState.full_optimizer_state_dict(st, opt)
        assert sorted(sd["state"]) == [0, 1] and sd["param_groups"][0]["params"] == [0, 1]
        for k in names:
            assert torch.equal(sd["state"][0][k], values[k][:6].view(2, 3)) and torch.equal(sd["state"][1][k], values[k][6:])
        assert float(sd["state"][1]["step"]) == 5 and set(sd["state"][0]) == {"step", *names}
        if names == ("momentum_buffer",):       # the shape torch.optim.SGD loads
            torch.optim.SGD(nn.Linear(3, 2).parameters(), lr=1.0).load_state_dict(sd)
        path = str(tmp_path / f"{names[0]}.pth")
        torch.save({"epoch": 3, "model_state": model.state_dict(), "optimizer_state": sd}, path)
        fresh = nn.Linear(3, 2)
        fresh._native_shard = {"state": shard(fresh), "precision": "float32"}
        opt2 = make([fresh._native_shard["state"].master])
        assert load_checkpoint(fresh, opt2, path) == 3
        got = opt2.state[fresh._native_shard["state"].master]
        for k in names:
            assert torch.equal(got[k], values[k]), k
        assert float(got["step"]) == 5
        assert torch.equal(fresh._native_shard["state"].master.detach(),
                           torch.cat([p.detach().reshape(-1) for p in model.parameters()]))
    # a torch.optim.SGD checkpoint of the bare model (no `step`, an unset buffer): zeros and 0
    bare = nn.Linear(3, 2)
    theirs = torch.optim.SGD(bare.parameters(), lr=0.1, momentum=0.9)
    bare.weight.grad = torch.ones(2, 3)
    theirs.step()
    path = str(tmp_path / "torch_sgd.pth")
    torch.save({"epoch": 1, "model_state": bare.state_dict(), "optimizer_state": theirs.state_dict()}, path)
    fresh = nn.Linear(3, 2)
    fresh._native_shard = {"state": shard(fresh), "precision": "float32"}
    opt3 = HipSGD([fresh._native_shard["state"].master], lr=1e-3)
    load_checkpoint(fresh, opt3, path)
    got = opt3.state[fresh._native_shard["state"].master]
    assert torch.equal(got["momentum_buffer"], torch.tensor([1.0] * 6 + [0.0] * 2)) and float(got["step"]) == 0
