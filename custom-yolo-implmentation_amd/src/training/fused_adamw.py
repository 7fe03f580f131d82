"""AdamW over every parameter in ONE kernel launch: `HipAdamW`, a drop-in for the
`torch.optim.AdamW` that the reference's get_optimizer builds (src/training/utils_train.py:34; step at
src/training/train_model.py:247-253).

* same update rule, defaults, `param_groups` keys and per-parameter state names (`step`, `exp_avg`, `exp_avg_sq`),
  so `ReduceLROnPlateau`, checkpoints (`state_dict` / `load_state_dict`) and `GradScaler.step` work unchanged;
* hyper-parameters and the step counter live in device memory: a captured step follows a learning-rate schedule
  without recapture (`sync_hyper()` copies changed values; `step()` calls it when not capturing);
* the kernel reads a device job table (parameter / gradient / moment pointers).  Gradient tensors are re-created by
  autograd every eager step, so the table is rebuilt when a pointer changed; inside a graph capture the pointers are
  final but an upload cannot be captured safely, so `step()` only records the launch and `finish_capture()` -- called
  by TrainStepRunner after the capture -- uploads the table once.
* FSDP2 (`fully_shard`) parameters are DTensors: the kernel updates each rank's LOCAL shard (a persistent view of the
  wrapper's sharded storage) from the local shard of the reduce-scattered gradient; the moments are DTensors with the
  parameter's placement, so `torch.distributed.checkpoint` gathers / scatters the optimizer state like torch.optim.AdamW's.
  There GradScaler unscales the gradients itself (`_step_supports_amp_scaling` off: ShardedGradScaler must all-reduce
  found_inf across ranks before anyone steps).
* `max_grad_norm=c`: `torch.nn.utils.clip_grad_norm_(params, c)` (L2, one norm over ALL parameter groups) folded into the
  step: one pass over the job tables leaves a partial sum of squares per chunk, one small kernel turns them into
  `[total_norm, coef]` in device memory, and the AdamW kernel multiplies every gradient by `coef` in flight.  The one
  deviation from clip_grad_norm_: the `.grad` tensors themselves are NOT modified.  (The reference's config.yaml carries
  training.grad_clip, but its loop never reads it.)  Not combined with DTensor parameters: the shard norms would need a
  collective.
* `ema_decay=d` (with `ema_tau`): an exponential moving average of the weights -- the `ModelEMA` of the YOLOv5 / v8 recipes,
  `ema = d_t*ema + (1-d_t)*w` after every step with `d_t = d*(1 - exp(-t/tau))` (tau 0: constant d) -- kept by the AdamW
  kernel itself: one fp32 shadow per stepped parameter, no extra launch, inside a captured step.  `src/training/ema.py`
  (`ModelEMA`) adds the BatchNorm running statistics, the swap for validation and the checkpoint form.  Deviations from the
  host-side recipe: a step skipped on overflow moves neither the shadows nor t; a parameter without a gradient on a step is
  not in the job table, so its shadow does not move on that step; the average is of the parameter AS STORED (a bf16
  parameter's rounded value).  The reference has no EMA.  Not combined with DTensor parameters.
There is no CPU path: parameters must live on the GPU (like every op of this package).

Everything above except the update rule itself lives in `HipFusedOptimizer`, the base that `HipAdamW` shares with `HipSGD`
(src/training/fused_sgd.py; config key training.optimizer).
"""
import torch

from src.hipops import lib
from src.hipops.ops import _p, _stream, dt

try:
    from torch.distributed.tensor import DTensor
except ImportError:  # pragma: no cover
    DTensor = ()


def _loc(t):
    """The tensor the kernel touches: a DTensor's local shard, else the tensor itself."""
    return t._local_tensor if isinstance(t, DTensor) else t


def _grad(p):
    """The gradient the kernel reads: `p.lowp_grad` when set (a bf16 / f16 gradient of an fp32 master parameter -- torch
    refuses such a tensor as `.grad`; ShardedStepRunner's reduce-scattered shard), else `p.grad`."""
    g = getattr(p, "lowp_grad", None)
    return g if g is not None else p.grad


class DeviceGradScaler:
    """torch.amp.GradScaler's state and rules (defaults: init_scale 65536, growth 2, backoff 0.5, interval 2000 -- what the
    reference constructs, src/training/train_model.py:195-208) held in device memory, for a training step that never
    returns to the host: `scale` multiplies the loss gradient inside the loss kernel (functions.LOSS_SCALE), `HipAdamW.step`
    with `optimizer.device_amp = this` checks every gradient for inf / nan, skips or applies the unscaled update and
    updates the scale (csrc/optim.hip: yolo_adamw_amp_step).  One optimizer with ONE parameter group per scaler."""

    def __init__(self, device, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        self.state = torch.tensor([init_scale, 0.0, 0.0], dtype=torch.float32, device=device)   # scale, found_inf, last found_inf
        self.tracker = torch.zeros(1, dtype=torch.int32, device=device)
        self.growth_factor, self.backoff_factor, self.growth_interval = growth_factor, backoff_factor, growth_interval

    @property
    def scale(self):
        """fp32 device scalar (a view: the kernels update it in place)."""
        return self.state[0:1]

    def get_scale(self):
        return float(self.state[0])                 # host sync: for logging / tests only

    def last_step_skipped(self):
        return bool(self.state[2] != 0)             # host sync: for logging / tests only

    def state_dict(self):
        return dict(scale=self.get_scale(), growth_tracker=int(self.tracker), growth_factor=self.growth_factor,
                    backoff_factor=self.backoff_factor, growth_interval=self.growth_interval)

    def load_state_dict(self, sd):
        self.state[0] = float(sd["scale"])
        self.tracker.fill_(int(sd.get("growth_tracker", sd.get("_growth_tracker", 0))))
        self.growth_factor, self.backoff_factor = sd["growth_factor"], sd["backoff_factor"]
        self.growth_interval = sd["growth_interval"]


class HipFusedOptimizer(torch.optim.Optimizer):
    """What `HipAdamW` and `HipSGD` (src/training/fused_sgd.py) share: the device job table (plan / build / pointer refresh),
    the device hyper block and step counter (`sync_hyper`), `finish_capture` / `restore_capture`, global-norm clipping
    (`max_grad_norm`, `last_grad_norm`, `last_clip_coef`), the weight EMA (`ema_decay`, `ema_tau`, shadows, `ema_prepare`,
    `attach_ema_buffers`), both loss-scaling routes and the DTensor rules.  A subclass names its fp32 per-parameter state
    tensors (`_STATE`: the job record's m, then v), lays out its hyper block (`_HYPER` doubles, `_hyper_values`), may refuse a
    group (`_check_group`) and issues its own step launches (`_step_call`, `_amp_step_call`)."""
    _step_supports_amp_scaling = True      # GradScaler hands over grad_scale / found_inf instead of unscaling itself
    _STATE = ()
    _HYPER = 0

    def __init__(self, params, defaults, max_grad_norm=None, ema_decay=None, ema_tau=2000.0):
        # an attribute of the optimizer, NOT a param_groups key and not in state_dict(): checkpoints stay loadable by
        # the torch optimizer of the same rule and the reference
        self.max_grad_norm = max_grad_norm
        self._plans = {}                    # group index -> dict(ptrs, jobs_dev, njobs, nchunks, hyper, hyper_host, step, ema_ctl)
        self._ema = {}                      # parameter -> fp32 shadow; on the optimizer but OUTSIDE self.state (checkpoints)
        self._ema_buffers = None            # ModelEMA's job table over the model's float buffers (attach_ema_buffers)
        self._ema_decay = None
        self.ema_tau = ema_tau              # the same kind of attribute as max_grad_norm: validated, not in state_dict()
        self.ema_decay = ema_decay
        super().__init__(params, defaults)
        if any(isinstance(p, DTensor) for g in self.param_groups for p in g["params"]):
            self._step_supports_amp_scaling = False     # sharded: the scaler unscales and agrees on found_inf across ranks
            if max_grad_norm is not None:
                raise ValueError(f"{self._who}: max_grad_norm is not supported with DTensor (FSDP2) parameters: the global "
                                 "norm of sharded gradients needs a collective over the shard norms")
        self._refuse_sharded_ema()
        self._clip = None                   # dict(state = fp32 [max_norm, total_norm, coef], host = uploaded max_norm, partials)
        self._pending = []                  # (jobs_dev, pinned host table) awaiting upload after a capture
        # grad_scale / found_inf are NOT pre-defined: GradScaler.step multiplies an existing grad_scale attribute in,
        # sets both around step() and deletes them afterwards

    @property
    def _who(self):
        return type(self).__name__

    # ------------------------------------------------------------------------------------------ what a subclass provides
    def _hyper_values(self, group):
        """The group's hyper block as a tuple of `_HYPER` floats (validated: they go to the device as they are)."""
        raise NotImplementedError

    def _check_group(self, group):
        """Raise for a group whose keys ask for a variant the kernel does not implement."""

    def _step_call(self, plan, scale, found, clip, st):
        """Tick + update of one job table; scale / found: GradScaler protocol or None, clip: the clip state or None."""
        raise NotImplementedError

    def _amp_step_call(self, plan, amp, st):
        """found_inf pass, tick, update and scale update of one job table under a DeviceGradScaler."""
        raise NotImplementedError

    def _plan_args(self, plan):
        return _p(plan["jobs_dev"]), plan["njobs"], plan["nchunks"], _p(plan["hyper"]), _p(plan["step"])

    # ------------------------------------------------------------------------------------------ clipping
    @property
    def max_grad_norm(self):
        """Threshold of the global L2 gradient norm, or None = no clipping.  A new value reaches the device with the next
        `sync_hyper()` (so a captured step follows it without recapture); switching between None and a number after a
        capture needs a new capture, because the captured launches differ."""
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        if value is not None:
            value = float(value)
            if not (0.0 < value <= 3.4028234664e38):        # fp32 on the device; also rejects nan
                raise ValueError(f"{self._who}: max_grad_norm must be finite and > 0, or None (got {value})")
        self._max_grad_norm = value

    def _clip_view(self, k):
        if self._clip is None:
            raise RuntimeError(f"{self._who}: no clipped step has run yet (max_grad_norm is None or step() was not called)")
        return self._clip["state"][k]

    @property
    def last_grad_norm(self):
        """Global L2 norm of the (unscaled) gradients of the last step BEFORE clipping: a 0-dim device view that later
        steps and replays update in place.  Reading it syncs the host: for logging and tests only."""
        return self._clip_view(1)

    @property
    def last_clip_coef(self):
        """min(1, max_grad_norm / (norm + 1e-6)) of the last step: a 0-dim device view, like `last_grad_norm`."""
        return self._clip_view(2)

    def _clip_buffers(self, dev, nparts, capturing):
        c = self._clip
        if c is None or c["partials"].numel() < nparts or c["state"].device != dev:
            if capturing:
                raise RuntimeError(f"{self._who}: run one eager step before capturing a graph (the clip buffers are allocated there)")
            keep = c is not None and c["state"].device == dev      # more chunks than before: the state views stay valid
            state = c["state"] if keep else torch.tensor([self._max_grad_norm, 0.0, 1.0], dtype=torch.float32, device=dev)
            c = self._clip = dict(state=state, host=c["host"] if keep else self._max_grad_norm,
                                  partials=torch.zeros(nparts, dtype=torch.float32, device=dev))
        return c

    # ------------------------------------------------------------------------------------------ weight EMA
    @property
    def ema_decay(self):
        """Decay of the weight EMA kept inside the step, or None = no EMA.  A new value (and a new `ema_tau`) reaches the
        device with the next `sync_hyper()`, so a captured step follows a decay schedule without recapture; switching
        between None and a number after a capture raises, because the captured job tables differ."""
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, value):
        if value is not None:
            value = float(value)
            if not (0.0 < value < 1.0):                     # also rejects nan
                raise ValueError(f"{self._who}: ema_decay must lie strictly between 0 and 1, or be None (got {value})")
        if (value is None) != (self._ema_decay is None):
            if any(plan.get("cap_host") is not None for plan in self._plans.values()):
                raise RuntimeError(f"{self._who}: the EMA cannot be turned on or off after a graph capture (the captured job "
                                   "tables carry the shadow pointers); capture again with a new optimizer")
            for plan in self._plans.values():
                plan["ptrs"] = None                         # the next step rebuilds the job table with / without shadows
            if value is None:
                # off: a later average starts afresh, at the weights of that time and with updates = 0, not from shadows
                # that stopped following the weights when the average was switched off
                self._ema.clear()
                for plan in self._plans.values():
                    plan["ema_ctl"][2:3].zero_()
        self._ema_decay = value
        if value is not None and hasattr(self, "param_groups"):
            self._refuse_sharded_ema()

    @property
    def ema_tau(self):
        """Ramp of the decay in updates: d_t = ema_decay * (1 - exp(-t / ema_tau)); 0 = constant decay."""
        return self._ema_tau

    @ema_tau.setter
    def ema_tau(self, value):
        value = float(value)
        if not (0.0 <= value <= 1.7976931348623157e308):    # also rejects nan
            raise ValueError(f"{self._who}: ema_tau must be finite and >= 0 (got {value})")
        self._ema_tau = value

    def _refuse_sharded_ema(self):
        if self._ema_decay is not None and any(isinstance(p, DTensor) for g in self.param_groups for p in g["params"]):
            raise ValueError(f"{self._who}: ema_decay is not supported with DTensor (FSDP2) parameters: every rank would average "
                             "only its shard, and nothing gathers the shadows")

    @property
    def ema_updates(self):
        """EMA updates so far (skipped steps do not count): a 0-dim float64 device view that later steps and replays
        update in place, like `last_grad_norm`.  Reading it syncs the host: for logging and tests only."""
        for gi in sorted(self._plans):
            return self._plans[gi]["ema_ctl"][2]
        raise RuntimeError(f"{self._who}: no step has run yet and ema_prepare() was not called")

    def ema_shadow(self, p):
        """The fp32 shadow of parameter `p`, or None (EMA off, or `p` has never been stepped nor prepared)."""
        return self._ema.get(p)

    def _shadow(self, p):
        e = self._ema.get(p)
        if e is None:                                       # the EMA starts at the weights
            if p.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self._who}: run one eager step before capturing a graph (the EMA shadows are created "
                                   "there; a copy made while capturing would be replayed with every step)")
            e = self._ema[p] = _loc(p).detach().clone().to(torch.float32).contiguous()
        return e

    def ema_prepare(self):
        """Create the control blocks and the shadow of every trainable parameter NOW instead of on its first step, so
        that `ModelEMA.load_state_dict` has something to copy into before the first step.  Needs `ema_decay`."""
        if self._ema_decay is None:
            raise RuntimeError(f"{self._who}.ema_prepare: ema_decay is None")
        for gi, group in enumerate(self.param_groups):
            if group["params"]:
                self._plan(group, gi)
                for p in group["params"]:
                    if p.requires_grad:
                        self._shadow(p)

    def attach_ema_buffers(self, table):
        """`table` (ModelEMA's): dict(jobs_dev, njobs, nchunks) over tensors the optimizer does not step.  `step()` ends
        with one launch over it -- after every group's step launch, so the update count already includes the step."""
        self._ema_buffers = table

    # ------------------------------------------------------------------------------------------ state
    def _plan(self, group, gi):
        plan = self._plans.get(gi)
        if plan is None:
            dev = next(p.device for p in group["params"])
            plan = self._plans[gi] = dict(ptrs=None, jobs_dev=None, host=None, njobs=0, nchunks=0, hyper_host=None,
                                          hyper=torch.zeros(self._HYPER, dtype=torch.float64, device=dev),
                                          step=torch.zeros((), dtype=torch.float32, device=dev),
                                          ema_ctl=torch.zeros(3, dtype=torch.float64, device=dev), ema_host=None)
        return plan

    def _init_state(self, group, gi):
        plan = self._plan(group, gi)
        for p in group["params"]:
            if self._ema_decay is not None and _grad(p) is not None:
                self._shadow(p)
            st = self.state[p]
            if self._STATE[0] not in st:
                st["step"] = plan["step"]                           # one shared device counter per group
                for name in self._STATE:
                    st[name] = self._zeros(p)
            elif st.get("step") is not plan["step"]:
                # after load_state_dict: adopt the loaded count (a torch optimizer that keeps none: 0) and tensors (one
                # that torch left unset: zeros); the job table is rebuilt, because it points at the tensors they replace
                plan["step"].copy_(torch.as_tensor(st.get("step", 0.0), dtype=torch.float32).reshape(()))
                st["step"] = plan["step"]
                for name in self._STATE:
                    st[name] = self._zeros(p) if st.get(name) is None else st[name].to(torch.float32)
                plan["ptrs"] = None
        return plan

    @staticmethod
    def _zeros(p):
        if isinstance(p, DTensor):                                  # same mesh / placement as the parameter
            return torch.zeros_like(p, dtype=torch.float32)
        return torch.zeros(p.shape, dtype=torch.float32, device=p.device)

    def sync_hyper(self):
        """Copy changed hyper-parameters (e.g. a scheduler's new lr) to the device; call between graph replays."""
        for gi, group in enumerate(self.param_groups):
            plan = self._plans.get(gi)
            if plan is None:
                continue
            want = self._hyper_values(group)
            if plan["hyper_host"] != want:
                plan["hyper"].copy_(torch.tensor(want, dtype=torch.float64))
                plan["hyper_host"] = want
            # decay and tau only: `updates` is the device's own count (ModelEMA.load_state_dict is its one other writer)
            if self._ema_decay is not None and plan["ema_host"] != (self._ema_decay, self._ema_tau):
                plan["ema_ctl"][0:2].copy_(torch.tensor([self._ema_decay, self._ema_tau], dtype=torch.float64))
                plan["ema_host"] = (self._ema_decay, self._ema_tau)
        c = self._clip
        if c is not None and self._max_grad_norm is not None and c["host"] != self._max_grad_norm:
            c["state"][0:1].copy_(torch.tensor([self._max_grad_norm], dtype=torch.float32))
            c["host"] = self._max_grad_norm

    def finish_capture(self):
        """Upload the job tables recorded while a graph was being captured (call once after the capture ends)."""
        for dev_t, host_t in self._pending:
            dev_t.copy_(host_t)
        self._pending = []
        for plan in self._plans.values():               # kept for restore_capture()
            if plan["host"] is not None:
                plan["cap_host"], plan["cap_ptrs"] = plan["host"].clone(), plan["ptrs"]
        self.sync_hyper()

    def restore_capture(self):
        """After an EAGER step() between replays (its gradients live elsewhere, so it rebuilt the job table the captured
        launch reads): put the captured table back."""
        for plan in self._plans.values():
            if plan.get("cap_host") is not None and plan["ptrs"] != plan["cap_ptrs"]:
                plan["host"].copy_(plan["cap_host"])
                plan["jobs_dev"].copy_(plan["host"])
                plan["ptrs"] = plan["cap_ptrs"]

    # ------------------------------------------------------------------------------------------ step
    @torch.no_grad()
    def step(self, closure=None):
        """One launch for all parameters of a group.  Deviation from torch.optim.AdamW / SGD: the step counter (AdamW's bias
        correction, SGD's warm-up position) is per GROUP, not per parameter -- a parameter that receives no gradient on some
        steps is corrected as if it had been stepped with the others (the reference's model gives every parameter a
        gradient on every step).  The EMA
        (`ema_decay`) shares that table: the update count is per group too, and a parameter without a gradient on a step
        is not in the table, so its shadow does not move on that step."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ready, ema_ctl = [], None
        for gi, group in enumerate(self.param_groups):
            params = [p for p in group["params"] if _grad(p) is not None]
            if not params:
                continue
            self._check_group(group)
            plan = self._init_state(group, gi)
            capturing = torch.cuda.is_current_stream_capturing()
            ptrs = tuple((_loc(p).data_ptr(), _loc(_grad(p)).data_ptr(), _loc(p).numel()) for p in params)
            if plan["ptrs"] != ptrs:
                old = plan["ptrs"]
                if (not capturing and old is not None and len(old) == len(ptrs) and plan["host"] is not None
                        and all(a[0] == b[0] and a[2] == b[2] for a, b in zip(old, ptrs))
                        and plan.get("gdtypes") == tuple(_grad(p).dtype for p in params)):
                    # same parameters, fresh gradient tensors (an eager loop's zero_grad(set_to_none=True)): one call
                    # rewrites the gradient pointers instead of a job_fill call per parameter
                    # The upload is asynchronous from one of TWO pinned staging tables; a table is rewritten only after
                    # the upload that last read it has completed (its event): no host sync unless the device is two
                    # steps behind.
                    import ctypes
                    stage = plan.setdefault("stage", [plan["host"].clone().pin_memory(), plan["host"].clone().pin_memory()])
                    evs = plan.setdefault("stage_ev", [None, None])
                    k = plan["stage_k"] = 1 - plan.get("stage_k", 1)
                    if evs[k] is not None:
                        evs[k].synchronize()
                    stage[k].copy_(plan["host"])
                    arr = (ctypes.c_void_p * len(ptrs))(*[t[1] for t in ptrs])
                    lib.call("yolo_adamw_jobs_set_grads", stage[k].data_ptr(), len(ptrs), arr)
                    plan["jobs_dev"].copy_(stage[k], non_blocking=True)
                    evs[k] = torch.cuda.Event()
                    evs[k].record()
                else:
                    self._build(plan, params, capturing)
                    plan["gdtypes"] = tuple(_grad(p).dtype for p in params)
                plan["ptrs"] = ptrs
            if not capturing:
                self.sync_hyper()
            elif plan["hyper_host"] is None:
                raise RuntimeError(f"{self._who}: run one eager step (or sync_hyper()) before capturing a graph")
            if ema_ctl is None:
                ema_ctl, ema_on = plan["ema_ctl"], params[0]
            if self._max_grad_norm is not None:
                ready.append((plan, params))        # clipped: the norm spans ALL groups, so the launches follow the loop
                continue
            self._launch(plan, params)
        if ready:
            self._clipped_step(ready)
        table = self._ema_buffers
        if table is not None and self._ema_decay is not None and ema_ctl is not None:
            # the statistics of a step that the scaler skipped stay out of the average too.  DeviceGradScaler's step has
            # already handed found_inf on to last_found_inf (state[2]) and cleared it; GradScaler's attribute is still set.
            # (DeviceGradScaler is for ONE parameter group: with several, unclipped, each group's launch decides and updates
            # the scale on its own, as before the EMA existed, and state[2] is the LAST group's decision.)
            amp = getattr(self, "device_amp", None)
            skip = amp.state[2:3] if amp is not None else getattr(self, "found_inf", None)
            lib.call("yolo_ema_lerp", _p(table["jobs_dev"]), table["njobs"], table["nchunks"], _p(ema_ctl), _p(skip),
                     _stream(_loc(ema_on)))
        return loss

    def _launch(self, plan, params):
        amp = getattr(self, "device_amp", None)
        if amp is not None:     # fp16 loss scaling kept on the device (DeviceGradScaler): found_inf, step, scale update
            self._amp_step_call(plan, amp, _stream(_loc(params[0])))
            return
        # GradScaler sets the two attributes around step() and deletes them after
        self._step_call(plan, getattr(self, "grad_scale", None), getattr(self, "found_inf", None), None,
                        _stream(_loc(params[0])))

    def _clipped_step(self, ready):
        """Norm pass of every group into ONE partials buffer, one finalize, then the step launches with the clip state.
        With `device_amp` the norm pass also raises found_inf (it replaces the separate found_inf pass) and the scale
        update follows the last group; with GradScaler's grad_scale attribute the norm is that of the unscaled gradients."""
        dev = ready[0][1][0].device
        st = _stream(ready[0][1][0])
        capturing = torch.cuda.is_current_stream_capturing()
        nparts = sum(plan["nchunks"] for plan, _ in ready)
        clip = self._clip_buffers(dev, nparts, capturing)
        if not capturing:
            self.sync_hyper()                       # max_norm, after the buffers exist
        amp = getattr(self, "device_amp", None)
        if amp is not None:
            scale, found, raise_found = amp.state, amp.state[1:2], amp.state[1:2]
        else:
            scale, found, raise_found = getattr(self, "grad_scale", None), getattr(self, "found_inf", None), None
        off = 0
        for plan, _ in ready:
            lib.call("yolo_grad_sqnorm", _p(plan["jobs_dev"]), plan["njobs"], plan["nchunks"],
                     clip["partials"].data_ptr() + 4 * off, _p(raise_found), st)
            off += plan["nchunks"]
        lib.call("yolo_grad_clip_finalize", _p(clip["partials"]), nparts, _p(clip["state"]), _p(scale), st)
        for plan, _ in ready:
            self._step_call(plan, scale, found, clip["state"], st)
        if amp is not None:
            lib.call("yolo_amp_update_scale", _p(amp.state), _p(amp.tracker), float(amp.growth_factor),
                     float(amp.backoff_factor), int(amp.growth_interval), st)

    def _build(self, plan, params, capturing):
        jb = lib.query("yolo_adamw_job_bytes")
        n = len(params)
        if plan["host"] is None or plan["host"].numel() != n * jb:
            if capturing:
                raise RuntimeError(f"{self._who}: run one eager step before capturing a graph (host/device tables are "
                                   "allocated there)")
            plan["host"] = torch.zeros(n * jb, dtype=torch.uint8).pin_memory()
            plan["jobs_dev"] = torch.empty(n * jb, dtype=torch.uint8, device=_loc(params[0]).device)
        host = plan["host"]
        for i, p in enumerate(params):
            st = self.state[p]
            w, g = _loc(p), _loc(_grad(p))
            bufs = [_loc(st[name]) for name in self._STATE]
            if not (w.is_contiguous() and g.is_contiguous() and all(b.is_contiguous() for b in bufs)):
                raise RuntimeError(f"{self._who} needs contiguous parameters, gradients and state tensors")
            if g.numel() != w.numel() or any(b.numel() != w.numel() for b in bufs):
                raise RuntimeError(f"{self._who}: gradient / state shards do not match the parameter's local shard")
            lib.call("yolo_adamw_job_fill", host.data_ptr(), i, _p(w), dt(w), _p(g), dt(g), _p(bufs[0]),
                     _p(bufs[1]) if len(bufs) > 1 else 0, w.numel())
            if self._ema_decay is not None:
                e = self._ema[p]
                if e.numel() != w.numel() or e.device != w.device:
                    raise RuntimeError(f"{self._who}: an EMA shadow does not match its parameter's local shard")
                lib.call("yolo_adamw_job_set_ema", host.data_ptr(), i, _p(e), _p(plan["ema_ctl"]))
        plan["nchunks"] = lib.query("yolo_adamw_jobs_finalize", host.data_ptr(), n)
        plan["njobs"] = n
        if capturing:
            # the pointers recorded now are the capture's final ones; the upload itself must not be captured
            # (and is not needed until the first replay): finish_capture() does it
            self._pending.append((plan["jobs_dev"], host))
        else:
            plan["jobs_dev"].copy_(host)


class HipAdamW(HipFusedOptimizer):
    _STATE = ("exp_avg", "exp_avg_sq")
    _HYPER = 5                              # [lr, beta1, beta2, eps, weight_decay]

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, capturable=True, max_grad_norm=None,
                 ema_decay=None, ema_tau=2000.0):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid AdamW hyper-parameter")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=True, differentiable=False, fused=True)
        super().__init__(params, defaults, max_grad_norm=max_grad_norm, ema_decay=ema_decay, ema_tau=ema_tau)

    def _hyper_values(self, group):
        return (float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                float(group["weight_decay"]))

    def _check_group(self, group):
        if group.get("amsgrad") or group.get("maximize"):
            raise RuntimeError("HipAdamW implements plain AdamW (amsgrad=False, maximize=False)")

    def _step_call(self, plan, scale, found, clip, st):
        if clip is None:
            lib.call("yolo_adamw_step", *self._plan_args(plan), _p(scale), _p(found), st)
        else:
            lib.call("yolo_adamw_clip_step", *self._plan_args(plan), _p(scale), _p(found), _p(clip), st)

    def _amp_step_call(self, plan, amp, st):
        lib.call("yolo_adamw_amp_step", *self._plan_args(plan), _p(amp.state), _p(amp.tracker), float(amp.growth_factor),
                 float(amp.backoff_factor), int(amp.growth_interval), st)
