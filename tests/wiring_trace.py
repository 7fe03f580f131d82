"""Launch trace of the host wiring (TEST INFRASTRUCTURE): which leaves of src.hipops.ops the autograd Functions call,
in which order, with which shapes and scalars, and into which earlier result each of them writes or accumulates.
Runs on the CPU over the stand-ins of tests/emulated_ops.py.  tools/record_wiring_trace.py writes the traces of a
checkout to tests/golden/wiring_trace.json; tests/test_backward_plan_cpu.py compares the working tree with that file."""
import hashlib
import inspect
import json
import re

import torch

import emulated_ops
from conftest import load_golden
from oracle.params import det_fill_
from src.hipops import functions as F_
from src.hipops import ops

BLOCK_TAGS = ["conv3x3s2", "conv1x1_id", "convdw", "residual", "c3k", "c3k2_res", "c3k2_csp", "sppf", "attention",
              "psablock", "psa"]
# arguments that say WHERE a leaf writes or what it adds: recorded with the record that produced their memory
LINK_ARGS = ("out", "acc_into", "acc2", "stats_acc", "res", "accumulate")


def traced_leaves():
    """Every leaf (a name of emulated_ops.LEAVES) that functions.py names through the `ops` namespace."""
    used = set(re.findall(r"\bops\.(\w+)", inspect.getsource(F_)))
    return sorted(n for n in emulated_ops.LEAVES if n in used)


def _tensors(v):
    if isinstance(v, torch.Tensor):
        return [v]
    if isinstance(v, (list, tuple)):
        return [t for e in v for t in _tensors(e)]
    return []


def _scalar(v):
    if isinstance(v, (list, tuple)):
        return [_scalar(e) for e in v]
    return v if v is None or isinstance(v, (bool, int, float, str)) else str(v)


class Owners:
    """Which record returned the storage behind a tensor (shared with tests/launch_replay.py)."""

    def __init__(self):
        self._owner = {}        # storage address -> (ordinal of the last record that returned it, the storage: kept
        #                         alive so that no later allocation can take its address)

    def of(self, t):
        return self._owner.get(t.untyped_storage().data_ptr(), (-1, None))[0]

    def returned(self, ordinal, result):
        for t in _tensors(result):
            st = t.untyped_storage()
            self._owner[st.data_ptr()] = (ordinal, st)


class Tracer:
    def __init__(self):
        self.records = []
        self.owners = Owners()

    def _record(self, name, sig, args, kwargs):
        bound = sig.bind(*args, **kwargs)
        bound.apply_defaults()
        rec = {"op": name, "tensors": {}, "scalars": {}, "links": {}}
        for arg, v in bound.arguments.items():
            ts = _tensors(v)
            if ts:
                rec["tensors"][arg] = [[list(t.shape), str(t.dtype)] for t in ts]
            else:
                rec["scalars"][arg] = _scalar(v)
            if arg in LINK_ARGS and v is not None:
                if isinstance(v, torch.Tensor):
                    rec["links"][arg] = [self.owners.of(v), v.storage_offset()]
                else:
                    rec["links"][arg] = _scalar(v)
        return rec

    def wrap(self, name, fn):
        sig = inspect.signature(fn)

        def traced(*args, **kwargs):
            rec = self._record(name, sig, args, kwargs)
            ordinal = len(self.records)
            self.records.append(rec)
            result = fn(*args, **kwargs)
            self.owners.returned(ordinal, result)
            return result
        return traced


def install(monkeypatch):
    """Emulated leaves, each of those functions.py calls wrapped to append to the returned Tracer's records."""
    emulated_ops.install(monkeypatch)
    tr = Tracer()
    for name in traced_leaves():
        monkeypatch.setattr(ops, name, tr.wrap(name, getattr(ops, name)))
    return tr


def block_trace(monkeypatch, tag):
    """Training forward and backward of one block of test_wiring_cpu.test_block_wiring."""
    from test_wiring_cpu import _blocks
    gd = load_golden("block_" + tag)
    m = torch.nn.ModuleDict({"m": _blocks()[tag]()})
    det_fill_(m.state_dict(), int(gd["seed"]))
    x = gd["x"].clone().requires_grad_(True)
    m.train()
    tr = install(monkeypatch)
    m["m"](x).backward(gd["dy"])
    monkeypatch.undo()
    return tr.records


def model_trace(monkeypatch):
    """The n320 training step of test_wiring_cpu.test_model_n320_train_step_wiring: forward, loss, backward."""
    from src.model.losses import YoloDFLQFLoss
    from src.model.model_builder import Model
    gd = load_golden("model_n320_train")
    l3 = load_golden("loss_n320")
    model = Model(csp=[False, True], depth=[1] * 6, width=[3, 16, 32, 64, 128, 256], num_classes=80)
    det_fill_(model.state_dict(), int(gd["seed"]))
    img = torch.randn(2, 3, 320, 320, generator=torch.Generator().manual_seed(50))
    model.train()
    tr = install(monkeypatch)
    preds, a, s = model(img)
    loss, _ = YoloDFLQFLoss(num_classes=80)(preds, [l3["gt0"], l3["gt1"]], a, s)
    loss.backward()
    monkeypatch.undo()
    return tr.records


def canonical(records):
    return json.dumps(records, sort_keys=True, separators=(",", ":"))


def summary(records):
    """What the fixture keeps of a long trace: calls per leaf and the digest of the ordered trace."""
    counts = {}
    for r in records:
        counts[r["op"]] = counts.get(r["op"], 0) + 1
    return {"counts": counts, "sha256": hashlib.sha256(canonical(records).encode()).hexdigest()}
