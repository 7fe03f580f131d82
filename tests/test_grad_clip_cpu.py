"""No-GPU checks of gradient clipping's host side: validation of `max_grad_norm`, that it stays out of checkpoints, that
get_optimizer forwards it, and that every route that cannot clip (torch.optim.AdamW, FSDP modes, the native shard)
refuses the key instead of training unclipped.  The kernels are covered by tests/test_gpu_grad_clip.py."""
import pytest
import torch
from torch import nn


def _params():
    return [nn.Parameter(torch.zeros(4, 3)), nn.Parameter(torch.zeros(5))]


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf"), -float("inf")])
def test_constructor_rejects_thresholds_that_are_not_finite_and_positive(bad):
    from src.training.fused_adamw import HipAdamW
    with pytest.raises(ValueError, match="max_grad_norm"):
        HipAdamW(_params(), lr=1e-3, max_grad_norm=bad)
    opt = HipAdamW(_params(), lr=1e-3, max_grad_norm=2.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.max_grad_norm = bad                     # a schedule's new value is validated like the constructor's
    assert opt.max_grad_norm == 2.0


def test_threshold_is_an_attribute_outside_param_groups_and_state_dict():
    from src.training.fused_adamw import HipAdamW
    assert HipAdamW(_params(), lr=1e-3).max_grad_norm is None
    opt = HipAdamW(_params(), lr=1e-3, max_grad_norm=0.5)
    assert opt.max_grad_norm == 0.5
    assert all("max_grad_norm" not in g for g in opt.param_groups) and "max_grad_norm" not in opt.defaults
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and "max_grad_norm" not in repr(sd)
    twin = torch.optim.AdamW(_params(), lr=1e-3)    # the checkpoint stays loadable by torch's AdamW
    twin.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="no clipped step"):
        opt.last_grad_norm


def test_get_optimizer_forwards_the_threshold_to_hipadamw(monkeypatch):
    from src.training.fused_adamw import HipAdamW
    from src.training.utils_train import get_optimizer
    model = nn.Linear(3, 2)
    # get_optimizer picks HipAdamW for GPU parameters only; nothing is launched before the first step()
    monkeypatch.setattr(nn.Parameter, "is_cuda", property(lambda self: True), raising=False)
    opt, _ = get_optimizer(model, lr=1e-3, weight_decay=1e-2, patience=3, factor=0.5, max_grad_norm=0.75)
    assert type(opt) is HipAdamW and opt.max_grad_norm == 0.75
    opt, _ = get_optimizer(model, lr=1e-3, weight_decay=1e-2, patience=3, factor=0.5)
    assert type(opt) is HipAdamW and opt.max_grad_norm is None


def test_get_optimizer_refuses_the_key_where_torch_adamw_would_step():
    from src.training.utils_train import get_optimizer
    model = nn.Linear(3, 2)                         # CPU parameters: torch.optim.AdamW
    with pytest.raises(ValueError, match="max_grad_norm"):
        get_optimizer(model, lr=1e-3, weight_decay=1e-2, patience=3, factor=0.5, max_grad_norm=1.0)
    opt, _ = get_optimizer(model, lr=1e-3, weight_decay=1e-2, patience=3, factor=0.5)
    assert type(opt) is torch.optim.AdamW


class _Untouchable:
    """Stands in for a data loader: any use is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"train() touched the loader (.{name}) before refusing max_grad_norm")

    def __iter__(self):
        raise AssertionError("train() iterated the loader before refusing max_grad_norm")

    def __len__(self):
        raise AssertionError("train() measured the loader before refusing max_grad_norm")


@pytest.mark.parametrize("mode", ["fsdp", "fsdp2"])
def test_train_refuses_the_key_in_fsdp_modes_before_touching_the_loader(mode):
    from src.training.train_model import train
    model = nn.Linear(3, 2)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="max_grad_norm"):
        train(model=model, train_loader=_Untouchable(), val_loader=_Untouchable(), optimizer=opt, scheduler=None,
              criterion=None, initial_epoch=0, num_epochs=1, device="cpu", distributed_mode=mode, max_grad_norm=1.0)


def test_native_shard_model_refuses_the_key():
    from src.training.fused_adamw import HipAdamW
    from src.training.sharded_step import ShardedStepRunner
    from src.training.train_model import train
    from src.training.utils_train import get_optimizer
    model = nn.Linear(3, 2)
    model._native_shard = {"state": None, "precision": "bfloat16"}
    with pytest.raises(ValueError, match="max_grad_norm"):
        get_optimizer(model, lr=1e-3, weight_decay=1e-2, patience=3, factor=0.5, max_grad_norm=1.0)
    assert model._native_shard["state"] is None                     # refused before anything was sharded
    clipped = HipAdamW(_params(), lr=1e-3, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        ShardedStepRunner(model, None, shard=object(), optimizer=clipped)
    with pytest.raises(ValueError, match="max_grad_norm"):
        train(model=model, train_loader=_Untouchable(), val_loader=_Untouchable(), optimizer=clipped, scheduler=None,
              criterion=None, initial_epoch=0, num_epochs=1, device="cpu", distributed_mode="fsdp2")


def test_dtensor_parameters_with_the_key_raise_at_construction(monkeypatch):
    from src.training import fused_adamw

    class FakeDTensor(nn.Parameter):
        pass
    monkeypatch.setattr(fused_adamw, "DTensor", FakeDTensor)
    ps = [FakeDTensor(torch.zeros(3))]
    with pytest.raises(ValueError, match="DTensor"):
        fused_adamw.HipAdamW(ps, lr=1e-3, max_grad_norm=1.0)
    assert fused_adamw.HipAdamW(ps, lr=1e-3).max_grad_norm is None


def test_header_documents_that_the_reference_never_reads_grad_clip():
    import os
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    text = open(os.path.join(root, "include", "yolo_hip.h")).read()
    block = next(b for b in text.split("/* ---- ") if b.startswith("optimizer"))
    for name in ("yolo_grad_sqnorm", "yolo_grad_clip_finalize", "yolo_adamw_clip_step", "yolo_amp_update_scale"):
        assert name in block, name
    assert "grad_clip" in block and "never reads" in block
    # the prototypes that existed keep their signatures
    assert "int yolo_adamw_step(const void* jobs_dev, int njobs, long nchunks, const double* hyper, float* step, " \
           "const float* grad_scale, const float* found_inf, hipStream_t st);" in block
