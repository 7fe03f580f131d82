"""What a training step launches, in which order and into which tensor, and the order in which the deferred
parameter gradients reach the side stream -- the host code of src/hipops/functions.py, checked without a GPU.

The launch traces are compared with tests/golden/wiring_trace.json, which tools/record_wiring_trace.py recorded from
the commit named in the file (the state BEFORE the change under test): one reordered, added or re-targeted launch
fails.  The queue is driven with stub streams that log `wait_stream` and context entry."""
import gc
import inspect
import json
import os
import weakref

import pytest
import torch

import wiring_trace as wt
from conftest import GOLDEN
from src.hipops import functions as F_

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "wiring_trace.json")) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------- launch traces
def test_the_traced_leaves_are_the_recorded_ones(fixture):
    assert wt.traced_leaves() == fixture["leaves"]


@pytest.mark.parametrize("tag", wt.BLOCK_TAGS)
def test_block_launch_trace(tag, fixture, monkeypatch):
    got, want = wt.block_trace(monkeypatch, tag), fixture["blocks"][tag]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{tag}: launch {i} differs"
    assert len(got) == len(want)


def test_model_n320_launch_trace(fixture, monkeypatch):
    got, want = wt.summary(wt.model_trace(monkeypatch)), fixture["model_n320"]
    assert got["counts"] == want["counts"]
    assert got["sha256"] == want["sha256"]


# ---------------------------------------------------------------------------------------------- the side queue
class StubStream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_stream(self, other):
        self.log.append(f"wait {self.name}<-{other.name}")

    def __enter__(self):
        self.log.append(f"enter {self.name}")

    def __exit__(self, *exc):
        self.log.append(f"leave {self.name}")


def make_queue(monkeypatch, group, join_each=True, lazy=True, overlap=True):
    log = []
    main, side = StubStream("main", log), StubStream("side", log)
    for name, v in (("WGRAD_GROUP", group), ("JOIN_EACH_GROUP", join_each), ("LAZY_WGRAD_JOIN", lazy), ("OVERLAP_WGRAD", overlap)):
        monkeypatch.setattr(F_, name, v)
    return F_.SideQueue(side, lambda: main, lambda s: s), main, log


def defer_job(q, log, i):
    """Defer job i with a keep-alive tensor of its own; only a weak reference to that tensor comes back."""
    keep = torch.zeros(1)
    assert q.defer((keep,), lambda: log.append(f"job {i}"))
    return weakref.ref(keep)


def alive(refs):
    gc.collect()
    return [r() is not None for r in refs]


def group_log(jobs, wait_first):
    return (["wait main<-side"] if wait_first else []) + ["wait side<-main", "enter side"] + [f"job {i}" for i in jobs] + ["leave side"]


def test_seven_jobs_in_groups_of_three_join_before_each_fork(monkeypatch):
    q, main, log = make_queue(monkeypatch, 3)
    refs = [defer_job(q, log, i) for i in range(2)]
    assert log == [] and len(q.queued) == 2
    refs.append(defer_job(q, log, 2))                       # sync 1: nothing in flight, so no wait main<-side
    assert log == group_log([0, 1, 2], wait_first=False)
    assert alive(refs) == [True] * 3
    refs += [defer_job(q, log, i) for i in (3, 4)]
    assert alive(refs) == [True] * 5
    refs.append(defer_job(q, log, 5))                       # sync 2 releases group 0, holds group 1
    assert alive(refs) == [False] * 3 + [True] * 3
    refs.append(defer_job(q, log, 6))
    q.join(main)                                            # sync 3 (releases group 1), then the last wait
    assert log == group_log([0, 1, 2], False) + group_log([3, 4, 5], True) + group_log([6], True) + ["wait main<-side"]
    assert alive(refs) == [False] * 7
    assert q.queued == [] and q.inflight == []


def test_the_group_size_is_read_when_a_job_is_deferred(monkeypatch):
    q, main, log = make_queue(monkeypatch, 8)
    defer_job(q, log, 0)
    monkeypatch.setattr(F_, "WGRAD_GROUP", 2)
    defer_job(q, log, 1)
    assert log == group_log([0, 1], wait_first=False)


def test_without_a_join_per_group_everything_is_held_until_the_one_join(monkeypatch):
    q, main, log = make_queue(monkeypatch, 3, join_each=False)
    refs = [defer_job(q, log, i) for i in range(7)]
    assert log == group_log([0, 1, 2], False) + group_log([3, 4, 5], False)
    assert alive(refs) == [True] * 7
    q.join(main)
    assert log == group_log([0, 1, 2], False) + group_log([3, 4, 5], False) + group_log([6], False) + ["wait main<-side"]
    assert alive(refs) == [False] * 7


def test_join_of_an_idle_queue_waits_for_nothing(monkeypatch):
    q, main, log = make_queue(monkeypatch, 3)
    q.join(main)
    assert log == []


@pytest.mark.parametrize("lazy, overlap", [(False, True), (True, False)])
def test_nothing_is_deferred_outside_a_lazy_overlapped_backward(monkeypatch, lazy, overlap):
    q, main, log = make_queue(monkeypatch, 1, lazy=lazy, overlap=overlap)
    assert q.defer((), lambda: log.append("job")) is False
    assert log == [] and q.queued == [] and q.inflight == []


def _closure_tensors(fn):
    out = []
    for cell in fn.__closure__ or ():
        v = cell.cell_contents
        out += [v] if isinstance(v, torch.Tensor) else _closure_tensors(v) if inspect.isfunction(v) else []
    return out


def test_a_deferred_gradient_shares_storage_but_no_tensor_object_with_the_queue(monkeypatch):
    """AccumulateGrad steals a gradient only if nobody else holds the tensor OBJECT; otherwise it clones it at once --
    before the side stream has written it (the regression of test_runner_gradients_equal_plain_autograd)."""
    q, main, log = make_queue(monkeypatch, 3)
    monkeypatch.setitem(F_._QUEUES, CPU, q)
    x, written = torch.ones(4), []

    def run(out):
        written.append(out)
        out.fill_(7.0)
    dw = F_._param_grad(CPU, (2, 3), torch.float32, (x,), run)
    assert written == [] and len(q.queued) == 1             # deferred: not written yet
    keep, fn = q.queued[0]
    held = list(keep) + _closure_tensors(fn)
    assert any(t.data_ptr() == dw.data_ptr() for t in held)
    assert all(t is not dw for t in held)
    assert not dw.requires_grad and dw.shape == (2, 3) and dw.dtype == torch.float32
    q.join(main)
    assert len(written) == 1 and written[0] is not dw and written[0].data_ptr() == dw.data_ptr()
    assert torch.equal(dw, torch.full((2, 3), 7.0))


def test_a_refused_gradient_is_written_inline(monkeypatch):
    q, main, log = make_queue(monkeypatch, 3, lazy=False)
    monkeypatch.setitem(F_._QUEUES, CPU, q)
    dw = F_._param_grad(CPU, (2,), torch.float32, (), lambda out: out.fill_(3.0))
    assert torch.equal(dw, torch.full((2,), 3.0)) and q.queued == [] and log == []
    monkeypatch.delitem(F_._QUEUES, CPU)                    # a device without a queue: inline as well
    assert torch.equal(F_._param_grad(CPU, (2,), torch.float32, (), lambda out: out.fill_(4.0)), torch.full((2,), 4.0))


@pytest.mark.parametrize("raises", [False, True])
def test_the_context_manager_clears_the_flag_and_joins(monkeypatch, raises):
    q, main, log = make_queue(monkeypatch, 3, lazy=False)
    monkeypatch.setitem(F_._QUEUES, CPU, q)
    try:
        with F_.lazy_param_grads(CPU, True):
            assert F_.LAZY_WGRAD_JOIN is True
            assert q.defer((), lambda: log.append("job 0"))
            assert log == []
            if raises:
                raise ZeroDivisionError
    except ZeroDivisionError:
        assert raises
    assert F_.LAZY_WGRAD_JOIN is False
    assert log == group_log([0], wait_first=False) + ["wait main<-side"]
    assert q.queued == [] and q.inflight == []
    del log[:]
    with F_.lazy_param_grads(CPU, False):
        assert q.defer((), lambda: log.append("job 1")) is False
    assert log == [] and F_.LAZY_WGRAD_JOIN is False


def test_the_queue_has_one_way_in():
    """Every deferred parameter gradient goes through _param_grad: the only caller of SideQueue.defer."""
    src = inspect.getsource(F_)
    assert src.count(".defer(") == 1 and ".defer(" in inspect.getsource(F_._param_grad)
