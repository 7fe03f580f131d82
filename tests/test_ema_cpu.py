"""No-GPU checks of the weight EMA's host side: validation of `ema_decay` / `ema_tau`, that both stay out of checkpoints,
that every route that cannot average (torch.optim.AdamW, FSDP modes, the native shard, DTensor parameters) refuses
instead of training without the average, and what the header promises.  Nothing is launched here; the kernels are covered
by tests/test_gpu_ema.py."""
import os

import pytest
import torch
from torch import nn


def _params():
    return [nn.Parameter(torch.zeros(4, 3)), nn.Parameter(torch.zeros(5))]


@pytest.mark.parametrize("bad", [0, 1, -0.1, float("nan"), float("inf")])
def test_constructor_and_setter_reject_decays_outside_the_open_unit_interval(bad):
    from src.training.fused_adamw import HipAdamW
    with pytest.raises(ValueError, match="ema_decay"):
        HipAdamW(_params(), lr=1e-3, ema_decay=bad)
    opt = HipAdamW(_params(), lr=1e-3, ema_decay=0.9)
    with pytest.raises(ValueError, match="ema_decay"):
        opt.ema_decay = bad                         # a schedule's new value is validated like the constructor's
    assert opt.ema_decay == 0.9


@pytest.mark.parametrize("bad", [-1, float("nan"), float("inf")])
def test_constructor_and_setter_reject_a_negative_or_non_finite_tau(bad):
    from src.training.fused_adamw import HipAdamW
    with pytest.raises(ValueError, match="ema_tau"):
        HipAdamW(_params(), lr=1e-3, ema_decay=0.9, ema_tau=bad)
    opt = HipAdamW(_params(), lr=1e-3, ema_decay=0.9, ema_tau=3)
    with pytest.raises(ValueError, match="ema_tau"):
        opt.ema_tau = bad
    assert opt.ema_tau == 3.0
    opt.ema_tau = 0                                 # constant decay
    assert opt.ema_tau == 0.0


def test_decay_and_tau_are_attributes_outside_param_groups_and_state_dict():
    from src.training.fused_adamw import HipAdamW
    off = HipAdamW(_params(), lr=1e-3)
    assert off.ema_decay is None and off.ema_tau == 2000.0
    opt = HipAdamW(_params(), lr=1e-3, ema_decay=0.9, ema_tau=3)
    assert opt.ema_decay == 0.9 and opt.ema_tau == 3.0
    for key in ("ema_decay", "ema_tau", "ema"):
        assert all(key not in g for g in opt.param_groups) and key not in opt.defaults
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and "ema" not in repr(sd)
    twin = torch.optim.AdamW(_params(), lr=1e-3)    # the checkpoint stays loadable by torch's AdamW
    twin.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="no step has run"):
        opt.ema_updates


class _Untouchable:
    """Stands in for a data loader: any use is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"train() touched the loader (.{name}) before refusing ema")

    def __iter__(self):
        raise AssertionError("train() iterated the loader before refusing ema")

    def __len__(self):
        raise AssertionError("train() measured the loader before refusing ema")


def _train(model, opt, mode, ema):
    from src.training.train_model import train
    train(model=model, train_loader=_Untouchable(), val_loader=_Untouchable(), optimizer=opt, scheduler=None,
          criterion=None, initial_epoch=0, num_epochs=1, device="cpu", distributed_mode=mode, ema=ema)


@pytest.mark.parametrize("mode", ["fsdp", "fsdp2"])
def test_train_refuses_an_ema_in_fsdp_modes_before_touching_the_loader(mode):
    from src.training.fused_adamw import HipAdamW
    model = nn.Linear(3, 2)
    opt = HipAdamW(model.parameters(), lr=1e-3, ema_decay=0.9)
    with pytest.raises(ValueError, match="training.ema"):
        _train(model, opt, mode, ema=object())


def test_train_refuses_an_ema_on_a_native_shard_model_before_touching_the_loader():
    from src.training.fused_adamw import HipAdamW
    model = nn.Linear(3, 2)
    model._native_shard = {"state": None, "precision": "bfloat16"}
    opt = HipAdamW(model.parameters(), lr=1e-3, ema_decay=0.9)
    with pytest.raises(ValueError, match="training.ema"):
        _train(model, opt, "ddp", ema=object())


def test_train_refuses_an_optimizer_that_keeps_no_average_before_touching_the_loader():
    from src.training.fused_adamw import HipAdamW
    model = nn.Linear(3, 2)
    with pytest.raises(ValueError, match="training.ema"):
        _train(model, torch.optim.AdamW(model.parameters(), lr=1e-3), "ddp", ema=object())
    with pytest.raises(ValueError, match="training.ema"):           # a HipAdamW, but without ema_decay
        _train(model, HipAdamW(model.parameters(), lr=1e-3), "ddp", ema=object())


def test_model_ema_refuses_an_optimizer_that_is_not_hipadamw():
    from src.training.ema import ModelEMA
    model = nn.Linear(3, 2)
    with pytest.raises(ValueError, match="HipAdamW"):
        ModelEMA(model, torch.optim.AdamW(model.parameters(), lr=1e-3))


def test_sharded_step_runner_refuses_an_averaging_optimizer():
    from src.training.fused_adamw import HipAdamW
    from src.training.sharded_step import ShardedStepRunner
    model = nn.Linear(3, 2)
    model._native_shard = {"state": None, "precision": "bfloat16"}
    averaging = HipAdamW(_params(), lr=1e-3, ema_decay=0.9)
    with pytest.raises(ValueError, match="ema_decay"):
        ShardedStepRunner(model, None, shard=object(), optimizer=averaging)


def test_dtensor_parameters_with_a_decay_raise(monkeypatch):
    from src.training import fused_adamw

    class FakeDTensor(nn.Parameter):
        pass
    monkeypatch.setattr(fused_adamw, "DTensor", FakeDTensor)
    ps = [FakeDTensor(torch.zeros(3))]
    with pytest.raises(ValueError, match="DTensor"):
        fused_adamw.HipAdamW(ps, lr=1e-3, ema_decay=0.9)
    opt = fused_adamw.HipAdamW(ps, lr=1e-3)
    assert opt.ema_decay is None
    with pytest.raises(ValueError, match="DTensor"):
        opt.ema_decay = 0.9


def test_header_documents_the_ema_entry_points_and_keeps_the_existing_prototypes():
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    text = open(os.path.join(root, "include", "yolo_hip.h")).read()
    block = next(b for b in text.split("/* ---- ") if b.startswith("optimizer"))
    assert "int yolo_adamw_job_set_ema(void* jobs_host, int index, float* ema, double* ema_ctl);" in block
    assert "int yolo_ema_lerp(const void* jobs_dev, int njobs, long nchunks, const double* ema_ctl, const float* skip_flag, " \
           "hipStream_t st);" in block
    assert "reference has NO EMA" in block and "train_model.py:247-253" in block
    # the prototypes that existed keep their signatures: every step entry point gets the EMA through the job record
    for proto in (
            "int yolo_adamw_job_fill(void* jobs_host, int index, void* p, int p_dtype, const void* g, int g_dtype, float* m, "
            "float* v, long n);",
            "int yolo_adamw_step(const void* jobs_dev, int njobs, long nchunks, const double* hyper, float* step, "
            "const float* grad_scale, const float* found_inf, hipStream_t st);",
            "int yolo_adamw_amp_step(const void* jobs_dev, int njobs, long nchunks, const double* hyper, float* step, "
            "float* amp_state, int* growth_tracker, float growth_factor, float backoff_factor, int growth_interval, "
            "hipStream_t st);",
            "int yolo_adamw_clip_step(const void* jobs_dev, int njobs, long nchunks, const double* hyper, float* step, "
            "const float* grad_scale, const float* found_inf, const float* clip_state, hipStream_t st);"):
        assert proto in block, proto
