"""`ModelEMA`: the exponential moving average of the weights that the YOLOv5 / v8 training recipes validate and ship
(`ema = d_t*ema + (1-d_t)*w` after every optimizer step, `d_t = decay*(1 - exp(-t/tau))`), kept on the device.  The
reference has no EMA (its loop, src/training/train_model.py:247-253, validates and saves the raw weights).

The average of the PARAMETERS is computed by the optimizer kernel itself (`HipAdamW(ema_decay=...)`, `HipSGD` alike: the kernel holds the
freshly updated parameter in a register, so the average costs one more fp32 read and write per element and no launch).
This class adds what belongs to the model rather than to the optimizer:

* the floating-point BUFFERS (BatchNorm running statistics) are averaged as the recipes do, by one launch per step over a
  job table of their own that `HipAdamW.step` issues after its AdamW launches (csrc/optim.hip: yolo_ema_lerp) -- inside a
  captured step like everything else;
* `state_dict()` / `load_state_dict()`: the averaged model under the bare `Model`'s key names and dtypes, so
  `Model(...).load_state_dict(sd["ema_state"])` needs no further code; loading copies IN PLACE, so job tables and captured
  graphs stay valid;
* `applied(model)`: a context manager that swaps the averaged values into the live model (in place: no pointer changes)
  for validation and restores the raw weights bit for bit afterwards.

Every rank applies the same averaged gradient, so the parameter shadows agree across ranks by construction; the buffer
shadows follow each rank's own statistics and `sync_buffers()` gives every rank rank 0's, as CapturedTraining does for
the live buffers.  Not for the sharded routes (FSDP1, FSDP2, native shard)."""
import contextlib

import torch

from src.hipops import lib
from src.hipops.ops import _p, dt


class ModelEMA:
    def __init__(self, model, optimizer, decay=0.9999, tau=2000.0):
        from torch.nn.parallel import DistributedDataParallel as DDP
        from src.training.fused_adamw import HipFusedOptimizer
        if not isinstance(optimizer, HipFusedOptimizer):
            raise ValueError("ModelEMA (training.ema) needs HipAdamW or HipSGD: the average of the parameters is computed "
                             "inside their step")
        self.model = model.module if isinstance(model, DDP) else model
        self.optimizer = optimizer
        optimizer.ema_tau = tau
        optimizer.ema_decay = decay
        optimizer.ema_prepare()                 # control blocks and parameter shadows exist from here on
        # floating-point buffers only: num_batches_tracked (int64) is taken from the live model by state_dict()
        self._buf_names, self._bufs, self._buf_shadows = [], [], []
        seen = set()
        for name, b in self.model.named_buffers():
            if b.is_floating_point() and id(b) not in seen:
                seen.add(id(b))
                self._buf_names.append(name)
                self._bufs.append(b)
                self._buf_shadows.append(b.detach().clone().to(torch.float32).contiguous())
        self._table = None
        self._stash = None
        if self._bufs:
            if not all(b.is_cuda for b in self._bufs):
                raise RuntimeError("ModelEMA needs the model's buffers on the GPU: the average of the running statistics is a "
                                   "HIP launch, and there is no CPU fallback")
            self._table = self._build_table()
            optimizer.attach_ema_buffers(self._table)

    def _build_table(self):
        """An AdamW job table with p = the buffer (read only), e = its shadow, g / m / v null."""
        jb, n = lib.query("yolo_adamw_job_bytes"), len(self._bufs)
        host = torch.zeros(n * jb, dtype=torch.uint8).pin_memory()
        for i, (b, e) in enumerate(zip(self._bufs, self._buf_shadows)):
            if not b.is_contiguous():
                raise RuntimeError("ModelEMA needs contiguous buffers")
            lib.call("yolo_adamw_job_fill", host.data_ptr(), i, _p(b), dt(b), 0, lib.F32, 0, 0, b.numel())
            lib.call("yolo_adamw_job_set_ema", host.data_ptr(), i, _p(e), 0)
        nchunks = lib.query("yolo_adamw_jobs_finalize", host.data_ptr(), n)
        dev = torch.empty(n * jb, dtype=torch.uint8, device=self._bufs[0].device)
        dev.copy_(host)
        return dict(jobs_dev=dev, host=host, njobs=n, nchunks=nchunks)

    # ------------------------------------------------------------------------------------------ views
    @property
    def updates(self):
        """Number of EMA updates so far (host sync: logging, checkpoints and tests)."""
        return int(float(self.optimizer.ema_updates))

    @property
    def decay(self):
        return self.optimizer.ema_decay

    @property
    def tau(self):
        return self.optimizer.ema_tau

    def _pairs(self):
        """(live tensors, their shadows): the parameters the optimizer keeps a shadow of, then the float buffers."""
        live, ema = [], []
        for p in self.model.parameters():
            e = self.optimizer.ema_shadow(p)
            if e is not None:
                live.append(p.detach())
                ema.append(e.view_as(p))
        return live + [b.detach() for b in self._bufs], ema + [e.view_as(b) for b, e in zip(self._bufs, self._buf_shadows)]

    def _named_shadows(self):
        from src.training.utils_train import canonical_state_dict
        named = {}
        for name, p in self.model.named_parameters(remove_duplicate=False):
            e = self.optimizer.ema_shadow(p)
            if e is not None:
                named[name] = e.view_as(p)
        for name, b, e in zip(self._buf_names, self._bufs, self._buf_shadows):
            named[name] = e.view_as(b)
        return canonical_state_dict(named)

    # ------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """{"ema_state", "updates", "decay", "tau"}.  ema_state: the bare Model's keys and the model's own dtypes; parameters
        and float buffers from the shadows, everything else (integer buffers, parameters that are never stepped) from the
        live model."""
        from src.training.utils_train import canonical_state_dict
        shadows = self._named_shadows()
        state = {}
        for k, v in canonical_state_dict(self.model.state_dict()).items():
            e = shadows.get(k)
            state[k] = (v if e is None else e.to(v.dtype)).detach().clone()
        return dict(ema_state=state, updates=self.updates, decay=self.decay, tau=self.tau)

    def _set_updates(self, n):
        for plan in self.optimizer._plans.values():
            plan["ema_ctl"][2:3].fill_(float(n))

    @torch.no_grad()
    def load_state_dict(self, sd):
        """Copies into the existing shadows and control blocks (in place: also valid after a capture)."""
        from src.training.utils_train import canonical_state_dict
        state = canonical_state_dict(sd["ema_state"])
        for k, e in self._named_shadows().items():
            if k not in state:
                raise KeyError(f"ModelEMA.load_state_dict: ema_state has no entry {k!r}")
            e.copy_(state[k].reshape(e.shape))
        self.optimizer.ema_tau = sd["tau"]
        self.optimizer.ema_decay = sd["decay"]
        self.optimizer.sync_hyper()
        self._set_updates(sd["updates"])

    @torch.no_grad()
    def reset_from_model(self):
        """The EMA restarts at the model's current values with updates = 0 (after loading a checkpoint that has no EMA)."""
        live, ema = self._pairs()
        if live:
            torch._foreach_copy_(ema, live)
        self._set_updates(0)

    # ------------------------------------------------------------------------------------------ validation swap
    @contextlib.contextmanager
    def applied(self, model=None):
        """Inside the block the model holds the averaged parameters and float buffers; on exit the raw values are back bit
        for bit.  Everything is copied in place, so a captured step replays correctly afterwards.  The stash is allocated
        on the first use and reused."""
        live, ema = self._pairs()
        if self._stash is None or len(self._stash) != len(live):
            self._stash = [torch.empty_like(t) for t in live]
        with torch.no_grad():
            if live:
                torch._foreach_copy_(self._stash, live)
                torch._foreach_copy_(live, ema)
        try:
            yield model if model is not None else self.model
        finally:
            with torch.no_grad():
                if live:
                    torch._foreach_copy_(live, self._stash)

    def sync_buffers(self):
        """Rank 0's buffer shadows on every rank (one flat fp32 broadcast)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1 or not self._buf_shadows:
            return
        flat = torch.cat([e.reshape(-1) for e in self._buf_shadows])
        dist.broadcast(flat, 0)
        off = 0
        for e in self._buf_shadows:
            e.copy_(flat[off:off + e.numel()].view_as(e))
            off += e.numel()
