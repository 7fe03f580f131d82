"""SGD with Nesterov momentum over every parameter in ONE kernel launch: `HipSGD`, the optimizer of the YOLO training
recipes, chosen by the config key `training.optimizer: "sgd"` (the reference's config.yaml:65 carries the key, but its
get_optimizer, src/training/utils_train.py:34, never reads it and always builds AdamW; step at
src/training/train_model.py:247-253).

* the update rule of `torch.optim.SGD(momentum=mu, dampening=0, weight_decay=wd, nesterov=..., maximize=False)`:
  `d = wd*p + g;  buf = mu*buf + d;  p -= lr * (mu*buf + d if nesterov else buf)` (csrc/optim.hip: k_sgd), its
  `param_groups` keys (plus `capturable=True`) and its state name `momentum_buffer`, so `ReduceLROnPlateau`,
  `GradScaler.step` and checkpoints work unchanged: a `state_dict()` loads into torch.optim.SGD and the other way round
  (a torch state has no `step`: 0; a buffer torch left unset: zeros);
* everything `HipAdamW` has through the shared `HipFusedOptimizer`: device hyper-parameters that a captured step follows
  without recapture, `max_grad_norm`, `ema_decay` / `ema_tau`, `device_amp`, DTensor local shards;
* a per-iteration WARM-UP on the device: `warmup_steps` W, `warmup_momentum` mu0 and `warmup_lr_scale` s0.  With t the
  group's step count (1, 2, ...) and f = (t-1)/W, a step with t <= W runs at `lr*(s0 + (1-s0)*f)` and `mu0 + (mu-mu0)*f`;
  later steps, and W = 0, see lr and mu themselves.  lr is the group's current value, so ReduceLROnPlateau composes with
  it; a step skipped on overflow does not advance t; nothing is uploaded per step.  The three are attributes of the
  optimizer, validated like `max_grad_norm`, NOT `param_groups` keys and not in `state_dict()`; the position t is the
  state's `step` and survives a checkpoint.

Deviations from torch.optim.SGD: the momentum buffer is fp32 whatever the parameter's dtype; it is kept (and equals d)
with `momentum == 0` too, where torch keeps none -- the parameters follow torch's; `step` is counted per group, as in
HipAdamW.  `dampening != 0` and `maximize` are refused: the constructor takes the two arguments (torch's call shape, and
what a loaded torch.optim.SGD group carries) only to raise a ValueError for any other value.  There is no CPU path."""
import math

from src.hipops import lib
from src.hipops.ops import _p
from src.training.fused_adamw import HipFusedOptimizer


def _finite_nonneg(who, name, value):
    value = float(value)
    if not (0.0 <= value <= 1.7976931348623157e308):            # also rejects nan
        raise ValueError(f"{who}: {name} must be finite and >= 0 (got {value})")
    return value


class HipSGD(HipFusedOptimizer):
    _STATE = ("momentum_buffer",)
    _HYPER = 7                              # [lr, momentum, weight_decay, nesterov, warmup_steps, warmup_momentum, warmup_lr_scale]

    def __init__(self, params, lr=1e-3, momentum=0.937, weight_decay=0.0, nesterov=True, warmup_steps=0, warmup_momentum=0.8,
                 warmup_lr_scale=0.0, max_grad_norm=None, ema_decay=None, ema_tau=2000.0, dampening=0, maximize=False):
        self.warmup_steps, self.warmup_momentum, self.warmup_lr_scale = warmup_steps, warmup_momentum, warmup_lr_scale
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=None, capturable=True, differentiable=False, fused=True)
        self._check_group(defaults)
        self._hyper_values(defaults)
        super().__init__(params, defaults, max_grad_norm=max_grad_norm, ema_decay=ema_decay, ema_tau=ema_tau)
        for group in self.param_groups:     # a group's own keys are checked like the defaults
            self._check_group(group)
            self._hyper_values(group)

    # ------------------------------------------------------------------------------------------ warm-up
    @property
    def warmup_steps(self):
        """Length W of the warm-up in optimizer steps; 0 = none.  Like the other two warm-up values a new one reaches the
        device with the next `sync_hyper()`, so a captured step follows it without recapture."""
        return self._warmup_steps

    @warmup_steps.setter
    def warmup_steps(self, value):
        value = _finite_nonneg("HipSGD", "warmup_steps", value)
        if value != math.floor(value) or value > 16777216.0:        # the step counter is an fp32 on the device
            raise ValueError(f"HipSGD: warmup_steps must be a whole number of steps up to 2^24 (got {value})")
        self._warmup_steps = int(value)

    @property
    def warmup_momentum(self):
        """Momentum mu0 of the first step; it moves linearly to the group's momentum over the warm-up."""
        return self._warmup_momentum

    @warmup_momentum.setter
    def warmup_momentum(self, value):
        value = float(value)
        if not (0.0 <= value < 1.0):                                # also rejects nan
            raise ValueError(f"HipSGD: warmup_momentum must lie in [0, 1) (got {value})")
        self._warmup_momentum = value

    @property
    def warmup_lr_scale(self):
        """Fraction s0 of the group's lr at the first step; it moves linearly to 1 over the warm-up."""
        return self._warmup_lr_scale

    @warmup_lr_scale.setter
    def warmup_lr_scale(self, value):
        value = float(value)
        if not (0.0 <= value <= 1.0):                               # also rejects nan
            raise ValueError(f"HipSGD: warmup_lr_scale must lie in [0, 1] (got {value})")
        self._warmup_lr_scale = value

    # ------------------------------------------------------------------------------------------ the shared base's hooks
    def _check_group(self, group):
        if group.get("dampening", 0) != 0 or group.get("maximize"):
            raise ValueError("HipSGD implements SGD with dampening=0 and maximize=False")
        if group["nesterov"] and not float(group["momentum"]) > 0.0:
            raise ValueError("HipSGD: nesterov needs momentum > 0 (as torch.optim.SGD)")

    def _hyper_values(self, group):
        return (_finite_nonneg("HipSGD", "lr", group["lr"]), _finite_nonneg("HipSGD", "momentum", group["momentum"]),
                _finite_nonneg("HipSGD", "weight_decay", group["weight_decay"]), 1.0 if group["nesterov"] else 0.0,
                float(self._warmup_steps), self._warmup_momentum, self._warmup_lr_scale)

    def _step_call(self, plan, scale, found, clip, st):
        lib.call("yolo_sgd_step", *self._plan_args(plan), _p(scale), _p(found), _p(clip), st)

    def _amp_step_call(self, plan, amp, st):
        lib.call("yolo_sgd_amp_step", *self._plan_args(plan), _p(amp.state), _p(amp.tracker), float(amp.growth_factor),
                 float(amp.backoff_factor), int(amp.growth_interval), st)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:     # torch.optim.SGD's groups have no such key; the captured routes ask for it
            group["capturable"] = True
            self._check_group(group)
            self._hyper_values(group)
