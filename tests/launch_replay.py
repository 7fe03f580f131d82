"""Launch recorder and replayer (TEST INFRASTRUCTURE): every launch of a real forward / backward held to its leaf's own
derived bound, against a float64 reference computed from the inputs the device itself read.

Principle (tests/strict_move.py's chain, applied to whole blocks): a leaf test chooses its own arguments, a whole-model
test carries every layer's error into the next and can only assert a loose band.  Here the real autograd Functions of
src/hipops/functions.py run on the real leaves of src.hipops.ops; a Recorder wrapped around each leaf copies, BEFORE the
launch and on the stream the launch goes to, the whole underlying buffer of every tensor argument (so also the prior contents
of out / acc_into / acc2 / res / stats_acc / acc / running_mean / running_var / idx), and AFTER the launch every result and
every argument again.  The replayer then rebuilds, per record, the float64 reference and the mass or noise budget from the
record's own snapshots and calls the comparator that leaf already has.  No error is carried from launch to launch, so the
leaf's bound applies unchanged however deep the network is.  No constant and no family multiplier is defined here.

Recorder.  named_leaves(): every function of src.hipops.ops that functions.py names through the `ops` namespace, the
device-only ones included; helpers that launch nothing of their own are left out (HELPERS; bn_acc_new's memset is recorded
through zero_).  A deferred weight gradient is recorded where it runs: the wrapper sits on the leaf, the SideQueue job calls
the leaf on the side stream.  Ownership is wiring_trace.Tracer's: a record knows which earlier record returned the storage
of each argument (`owner`), which is how a conv finds the OIHW weights its packed matrix was made from.

Adapters (leaf -> comparator):
    conv_fwd, conv_fwd_act, conv_dgrad (+ acc_into, acc2), conv_wgrad      strict_compare  auto / fp32 (+ _wgrad)
    dw_fwd, dw_fwd_act, dw_dgrad (+ acc_into), dw_wgrad                    strict_compare  depthwise (+ _wgrad)
    stem_conv_fwd, stem_wgrad                                              strict_compare  stem, stem_wgrad
    stem_bn_wgrad                                                          strict_stem_bwd reference / check
    statistics epilogue of conv_fwd / dw_fwd / stem_conv_fwd               strict_compare.assert_stats on the INCREMENT of the
                                                                           slice; the slice before must be exactly zero
    bn_act_fwd_train, bn_act_bwd_train, bn_train_stats,      strict_bn sums_* / coef_* / fwd_apply / bwd_dz /
    bn_act_fwd, bn_act_bwd, bn_act_bwd_eval, bn_eval_coeffs, channel_sum   bwd_apply / assert_within, fed the RECORDED sums
                                                                           (atomics order does not matter); running statistics too
    maxpool5_fwd / _bwd (routed by the recorded idx), upsample2x_fwd /     strict_move assert_exact / assert_sum
    _bwd, copy_channels, add_n, to_nhwc, head_group, zero_, fill_,
    scale_inplace, stem_im2col, stem_pack_weights, stem_unpack_wgrad
    pack_weights                                                           strict_move.bits: the packed matrix holds exactly the
                                                                           rounded weights and zeros (layout-free; the POSITIONS are
                                                                           held by the conv that reads it, whose reference is built
                                                                           from the OIHW weights)
    attn_fwd, attn_fwd_nograd, attn_bwd                                    strict_attention check_forward / check_backward
    loss_fwd_bwd                                                           strict_loss.verify (decode, assignment, scalars, gradients),
                                                                           the boxes and the assignment read from the launch's workspace
    loss_tal_fwd_bwd                                                       strict_tal.verify (decode, top-k lists, owners, targets,
                                                                           out[4], dpreds), the state read from the launch's workspace
replay() fails on a record of a leaf without an adapter.

Guard, on every record: an argument the leaf does not write is bit-equal before and after; of a written argument every byte
of the whole buffer outside the view is bit-equal before and after.

Identities (identities()): every parameter's .grad is bit-equal to the recorded output of the launch that produced it; the
block input's .grad is bit-equal to the last recorded write of that buffer; every tensor INPUT of a launch is bit-equal, at
launch time, to the last recorded write of that memory.  Memory written by anything that is not a recorded leaf is listed
as "<writer> -> <leaf>.<arg>" (the writer's ATen name from a TorchDispatchMode, `external` for memory that existed before the
recording); the tests pin that list per case, so a fall-back from the fan-in rule to an autograd sum shows up.

Recorded maxima: see MAXIMA below (filled from the runs named there)."""
import inspect
import re

import torch
from torch.utils._python_dispatch import TorchDispatchMode

import emulated_ops as emu
import strict_attention as sa
import strict_bn as sb
import strict_compare as sc
import strict_move as sm
import strict_stem_bwd as ssb
import wiring_trace as wt
from src.hipops import functions as F_
from src.hipops import ops

MAXIMA = """Recorded 2026-10-20 on the parent commit f54efa2 plus the kernel fix this module led to (csrc/conv_generic.hip, below).
MI355X, tests/test_gpu_launch_replay.py (181 tests, 18 s; 6140 launches of 38 leaves), largest value per family over every record:
  strict_compare families, (|got - ref| - 1/2 ulp - E_act) / (2^-24 M), c = 16 held:
    auto 0.75   auto_wgrad 4.89   depthwise 2.50   depthwise_wgrad 1.74   fp32 5.87   fp32_wgrad 2.43   stem 0.28   stem_wgrad 0.23
  budget families, share of the noise budget used (limit 1):
    attn_fused o 0.68  lse 0.09  dq 0.79  dk 0.76  dv 0.81     attn_fp32 o 0.05  lse 0.13  dq 0.05  dk 0.08  dv 0.09
    bn_coef 0.97   bn_fwd 0.41   bn_dy 0.56   bn_sum 0.21   bn_bwd_sum 0.06   bn_bwd_sumsq 0.07   bn_dgamma 0.07   bn_dbeta 0.04
    move_pool 0.43   move_up 0.00   move_copy 0.00   loss_decode 0.11 (assignment, scalars and the three gradient families inside 1/2 ulp)
    tal_target 0.37 (strict_tal.verify: top-k lists, owners, dense and box gradients, scalars inside 1/2 ulp)
  every exact-class tensor, every guard and every identity bit-equal.
  Found by the first run: conv_dgrad with acc_into AND acc2 on the VALU path (a Residual of 4 output channels inside C3K2, bf16 and
  f16) was up to 221 ulp off where the three terms cancel, 35 726 x 2^-24 M: valu_conv_launch added acc2 in a second pass, a second
  rounding to the 16-bit type.  k_conv_generic now adds both sources in fp32 before its one rounding; the launch is kept as
  test_regression_second_accumulate_source_on_the_valu_path_rounds_once.
CPU stand-ins (tests/test_launch_replay_cpu.py): STAND_IN_MAXIMA there, every family inside 1 x."""

HELPERS = {"is_nhwc", "new_nhwc", "geom", "bn_acc_new", "stem_conv_eligible"}      # launch nothing of their own
# the arguments a leaf writes or adds into (everything else must come back bit-equal)
WRITES = {"conv_fwd": ("stats_acc", "out"), "conv_fwd_act": ("out",), "conv_dgrad": ("acc_into",), "conv_wgrad": ("out",),
          "dw_fwd": ("stats_acc",), "dw_dgrad": ("acc_into",), "dw_wgrad": ("out",), "stem_conv_fwd": ("stats_acc",),
          "stem_wgrad": ("out",), "stem_bn_wgrad": ("out",), "stem_im2col": ("out",), "stem_unpack_wgrad": ("out",),
          "bn_act_fwd_train": ("running_mean", "running_var", "out"), "bn_act_bwd_train": ("acc",),
          "bn_train_stats": ("running_mean", "running_var"), "bn_act_fwd": ("out",), "channel_sum": ("out",),
          "copy_channels": ("dst",), "add_n": ("out",), "maxpool5_fwd": ("out",), "maxpool5_bwd": ("acc_into",),
          "upsample2x_fwd": ("out",), "upsample2x_bwd": ("acc_into",), "head_group": ("branches", "preds"),
          "zero_": ("t",), "fill_": ("t",), "scale_inplace": ("x",)}
MAY_DECLINE = ("conv_fwd_act", "dw_fwd_act", "attn_fwd_nograd")       # return None when the kernel does not take the problem


def named_leaves():
    """Every leaf of src.hipops.ops that functions.py names (wiring_trace.traced_leaves() without the restriction to the
    stand-ins' list: the device-only leaves are in)."""
    used = set(re.findall(r"\bops\.(\w+)", inspect.getsource(F_)))
    return sorted(n for n in used if n not in HELPERS and callable(getattr(ops, n, None)))


class ReplayMismatch(AssertionError):
    """A record outside its bound (or a broken guard / identity): `ordinal`, `op` and `arg` name the launch and the argument."""

    def __init__(self, msg, ordinal, op, arg, cause=None):
        super().__init__(f"launch {ordinal} {op} [{arg}]: {msg}")
        self.ordinal, self.op, self.arg, self.cause = ordinal, op, arg, cause


# ---------------------------------------------------------------------------------------------- snapshots
class Snap:
    """Copy of the WHOLE storage behind a tensor (1-D, the tensor's dtype, on the CPU) and the tensor's view of it."""
    __slots__ = ("whole", "shape", "stride", "offset", "dtype", "ptr")

    def __init__(self, t):
        t = t.detach()
        st = t.untyped_storage()
        n = st.nbytes() // t.element_size()
        whole = torch.empty(0, dtype=t.dtype, device=t.device).set_(st, 0, (n,), (1,))
        self.whole = whole.clone().cpu()                       # the clone runs on the current stream: the launch's own
        self.shape, self.stride, self.offset, self.dtype, self.ptr = tuple(t.shape), tuple(t.stride()), t.storage_offset(), t.dtype, st.data_ptr()

    def view(self, whole=None):
        return torch.as_strided(self.whole if whole is None else whole, self.shape, self.stride, self.offset)

    def mask(self):
        m = torch.zeros(self.whole.numel(), dtype=torch.bool)
        torch.as_strided(m, self.shape, self.stride, self.offset).fill_(True)
        return m


def _raw(t):
    """the bytes of a CPU tensor, in logical order"""
    return torch.empty(t.numel(), dtype=t.dtype).copy_(t.detach().reshape(-1)).view(torch.uint8)


def _tensors(v):
    if isinstance(v, torch.Tensor):
        return [v]
    if isinstance(v, (list, tuple)):
        return [t for e in v for t in _tensors(e)]
    return []


def _scalar(v):
    if isinstance(v, (list, tuple)):
        return [_scalar(e) for e in v]
    return v if v is None or isinstance(v, (bool, int, float, str, torch.dtype)) else str(v)


class Record:
    __slots__ = ("ordinal", "op", "before", "after", "results", "scalars", "owner", "source", "depth", "returned_none")

    def __init__(self, ordinal, op, depth):
        self.ordinal, self.op, self.depth = ordinal, op, depth
        self.before, self.after, self.results, self.scalars, self.owner, self.source = {}, {}, [], {}, {}, {}
        self.returned_none = False

    def b(self, arg, i=None):
        """the argument as the launch found it (logical view, CPU); None if it was not given"""
        s = self.before.get(arg)
        if isinstance(s, list):
            s = s[i or 0]
        return None if s is None else s.view()

    def a(self, arg):
        s = self.after.get(arg)
        return None if s is None else s.view()

    def r(self, i=0):
        return self.results[i].view()


class _Writers(TorchDispatchMode):
    """Which ATen op last wrote each storage (by address; the storage is kept so that no later allocation takes it)."""

    def __init__(self, rec):
        super().__init__()
        self.rec = rec

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        rec = self.rec
        if rec.quiet:
            return out
        name = str(func)
        outs = list(out) if isinstance(out, (list, tuple)) else [out]
        written = []
        try:
            rets = func._schema.returns
            for i, o in enumerate(outs):                      # a view or an in-place result is no new memory
                if i >= len(rets) or rets[i].alias_info is None:
                    written += _tensors(o)
            if func._schema.is_mutable:
                for a_, v in zip(func._schema.arguments, args):
                    if a_.alias_info is not None and a_.alias_info.is_write:
                        written += _tensors(v)
        except Exception:
            pass
        for t in written:
            try:
                st = t.untyped_storage()
            except Exception:
                continue
            rec.clock += 1
            rec.writer[st.data_ptr()] = (rec.clock, name, st)
        return out


class Recorder:
    def __init__(self):
        self.records = []
        self.owners = wt.Owners()   # which record RETURNED a storage: wiring_trace.Tracer's own bookkeeping
        self.shadow = {}         # storage address -> (clock, ordinal, Snap.whole after the last record that wrote it, storage)
        self.writer = {}         # storage address -> (clock, ATen op, storage)
        self.clock, self.quiet, self.depth = 0, False, 0
        self.mode = _Writers(self)
        self.unexplained = []    # (ordinal, op, arg): an input that differs from the last recorded write with no writer seen

    # -- the wrapper
    def wrap(self, name, fn):
        sig = inspect.signature(fn)

        def recorded(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            rec = Record(len(self.records), name, self.depth)
            self.records.append(rec)
            self.quiet = True
            try:
                for arg, v in bound.arguments.items():
                    ts = _tensors(v)
                    if not ts:
                        rec.scalars[arg] = _scalar(v)
                        continue
                    snaps = [Snap(t) for t in ts]
                    rec.before[arg] = snaps if isinstance(v, (list, tuple)) else snaps[0]
                    rec.owner[arg] = [self.owners.of(t) for t in ts]
                    rec.source[arg] = [self._source(rec, arg, s) for s in snaps]
            finally:
                self.quiet = False
            self.depth += 1
            try:
                result = fn(*args, **kwargs)
            finally:
                self.depth -= 1
            self.quiet = True
            try:
                rec.returned_none = result is None and name in MAY_DECLINE
                for arg, v in bound.arguments.items():
                    ts = _tensors(v)
                    if ts:
                        snaps = [Snap(t) for t in ts]
                        rec.after[arg] = snaps if isinstance(v, (list, tuple)) else snaps[0]
                        if arg in WRITES.get(name, ()):
                            for t, s in zip(ts, snaps):
                                self._wrote(rec, t, s)
                for t in _tensors(result):
                    s = Snap(t)
                    rec.results.append(s)
                    self._wrote(rec, t, s)
                self.owners.returned(rec.ordinal, result)
            finally:
                self.quiet = False
            return result
        return recorded

    def _wrote(self, rec, t, s):
        self.clock += 1
        self.shadow[s.ptr] = (self.clock, rec.ordinal, s.whole, t.untyped_storage())

    def _source(self, rec, arg, s):
        """ordinal of the record whose write this input is, bit for bit; else the name of what wrote the memory"""
        sh = self.shadow.get(s.ptr)
        wr = self.writer.get(s.ptr)
        if sh is not None:
            if sh[2].numel() == s.whole.numel() and torch.equal(_raw(sh[2]), _raw(s.whole)):
                return sh[1]
            if wr is not None and wr[0] > sh[0]:
                return wr[1]
            self.unexplained.append((rec.ordinal, rec.op, arg))
            return "unexplained"
        return wr[1] if wr is not None else "external"

    # -- what a finished recording says
    def counts(self):
        c = {}
        for r in self.records:
            c[r.op] = c.get(r.op, 0) + 1
        return c

    def foreign_writers(self):
        """sorted "<writer> -> <leaf>.<arg>" of every input that no recorded leaf wrote"""
        out = set()
        for r in self.records:
            for arg, srcs in r.source.items():
                out |= {f"{s} -> {r.op}.{arg}" for s in srcs if not isinstance(s, int)}
        return sorted(out)

    def last_write(self, t):
        """(ordinal, tensor) of the last recorded write of t's memory, viewed as t; None if no record wrote it"""
        sh = self.shadow.get(t.untyped_storage().data_ptr())
        if sh is None:
            return None
        return sh[1], torch.as_strided(sh[2], tuple(t.shape), tuple(t.stride()), t.storage_offset())


def pinned_writers(where):
    """tests/golden/launch_replay_writers.json -> {case: list} for `where` in ("cpu", "gpu").  The file keeps every DISTINCT
    list once ("lists", one per line) and, per case, the number of its list: a new writer shows as a new line."""
    import json
    import os
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "launch_replay_writers.json")) as f:
        d = json.load(f)
    return {k: d["lists"][i] for k, i in d["cases"][where].items()}


def install(monkeypatch, leaves=None):
    """Wrap the leaves (default: named_leaves()) as they are -- the real ones, or the stand-ins a caller installed before --
    and return the Recorder.  Use `with rec.mode:` around the pass to learn the ATen writers' names."""
    rec = Recorder()
    for name in (named_leaves() if leaves is None else leaves):
        if hasattr(ops, name):
            monkeypatch.setattr(ops, name, rec.wrap(name, getattr(ops, name)))
    return rec


# ---------------------------------------------------------------------------------------------- adapters
def _fam(dtype, low="auto"):
    return "fp32" if dtype == torch.float32 else low


def _weights(R, r, arg, kind):
    """OIHW weights (rounded to the compute type, float64) behind the packed matrix `arg`: from the pack record that
    returned its storage"""
    mine = r.before[arg]
    src = None
    for o in range(r.ordinal - 1, -1, -1):                     # the last pack launch that returned exactly this memory (a plan
        c = R.records[o]                                       # hands out views of one flat buffer: the storage alone is not enough)
        if c.op in ("pack_weights", "stem_pack_weights") and c.results and c.results[0].ptr == mine.ptr \
                and c.results[0].offset == mine.offset:
            src = c
            break
    if src is None or src.op != kind:
        raise ReplayMismatch(f"packed weights come from {'nowhere recorded' if src is None else src.op}, not from {kind}",
                             r.ordinal, r.op, arg)
    w = src.b("w")
    return w.to(src.scalars["dtype"]).double()


def _stats(r, arg, y, what):
    """the statistics epilogue: the slice was exactly zero, its increment is the sums of the STORED y"""
    before, after = r.b(arg), r.a(arg)
    if before is None:
        return
    if bool((before != 0).any()):
        raise ReplayMismatch(f"statistics slice not zero before the launch ({int((before != 0).sum())} of {before.numel()} "
                             f"entries, first {float(before[before != 0][0]):g})", r.ordinal, r.op, arg)
    c = y.shape[1]
    inc = (after.double() - before.double()).view(-1, 2, c).sum(0)
    try:
        sc.assert_stats(inc, y, what)
    except AssertionError as e:
        raise ReplayMismatch(str(e), r.ordinal, r.op, arg, e) from None


def _bias(ref, mass, bias):
    if bias is None:
        return ref, mass
    b = bias.double().view(1, -1, 1, 1)
    return ref + b, mass + b.abs()


def _act_res(ref, mass, act, res):
    e_act = None
    if act:
        ref, mass, e_act = sc.silu_terms(ref, mass)
    if res is not None:
        ref, mass = ref + res.double(), mass + res.double().abs()
    return ref, mass, e_act


def _base(ref, mass, *bases):
    for b in bases:
        if b is not None:
            ref, mass = ref + b.double(), mass + b.double().abs()
    return ref, mass


def a_conv_fwd(R, r, what):
    x, k, s = r.b("x"), r.scalars["k"], r.scalars["stride"]
    stem_cols = r.owner["wp"][0] >= 0 and R.records[r.owner["wp"][0]].op == "stem_pack_weights"
    if stem_cols:                                              # the unfold route: a 1x1 conv over the 32 columns
        w = _weights(R, r, "wp", "stem_pack_weights")
        w = torch.nn.functional.pad(w.reshape(w.shape[0], 27), (0, 5)).reshape(w.shape[0], 32, 1, 1)
    else:
        w = _weights(R, r, "wp", "pack_weights")
    ref, mass = _bias(*sc.conv_ref(x, w, k, s), r.b("bias"))
    got = r.r(0)
    sc.assert_close(got, ref, mass, got.dtype, what, _fam(got.dtype))
    _stats(r, "stats_acc", got, what)


def a_conv_fwd_act(R, r, what):
    x, k, s = r.b("x"), r.scalars["k"], r.scalars["stride"]
    ref, mass = _bias(*sc.conv_ref(x, _weights(R, r, "wp", "pack_weights"), k, s), r.b("bias"))
    ref, mass, e_act = _act_res(ref, mass, r.scalars["act"], r.b("res"))
    got = r.r(0)
    sc.assert_close(got, ref, mass, got.dtype, what, _fam(got.dtype), e_act=e_act)


def a_conv_dgrad(R, r, what):
    dy, k, s = r.b("dy"), r.scalars["k"], r.scalars["stride"]
    shape = (dy.shape[0], r.scalars["cin"], r.scalars["h"], r.scalars["w"])
    ref, mass = sc.dgrad_ref(dy, _weights(R, r, "wb", "pack_weights"), shape, k, s)
    ref, mass = _base(ref, mass, r.b("acc_into"), r.b("acc2"))
    got = r.r(0)
    sc.assert_close(got, ref, mass, got.dtype, what, _fam(got.dtype))


def a_conv_wgrad(R, r, what):
    x, dy, k, s = r.b("x"), r.b("dy"), r.scalars["k"], r.scalars["stride"]
    got = r.r(0)
    ref, mass = sc.wgrad_ref(x, dy, tuple(got.shape), k, s)
    sc.assert_close(got, ref, mass, got.dtype, what, _fam(x.dtype) + "_wgrad")


def _w9(r):
    w9 = r.b("w9")
    return w9.double().view(w9.shape[0], 1, 3, 3)


def a_dw_fwd(R, r, what):
    x = r.b("x")
    ref, mass = sc.conv_ref(x, _w9(r), 3, 1, groups=x.shape[1])
    got = r.r(0)
    sc.assert_close(got, ref, mass, got.dtype, what, "depthwise")
    _stats(r, "stats_acc", got, what)


def a_dw_fwd_act(R, r, what):
    x = r.b("x")
    ref, mass = _bias(*sc.conv_ref(x, _w9(r), 3, 1, groups=x.shape[1]), r.b("bias"))
    ref, mass, e_act = _act_res(ref, mass, r.scalars["act"], None)
    got = r.r(0)
    sc.assert_close(got, ref, mass, got.dtype, what, "depthwise", e_act=e_act)


def a_dw_dgrad(R, r, what):
    dy = r.b("dy")
    ref, mass = sc.dgrad_ref(dy, _w9(r), tuple(dy.shape), 3, 1, groups=dy.shape[1])
    ref, mass = _base(ref, mass, r.b("acc_into"))
    got = r.r(0)
    sc.assert_close(got, ref, mass, got.dtype, what, "depthwise")


def a_dw_wgrad(R, r, what):
    x, dy = r.b("x"), r.b("dy")
    got = r.r(0)
    ref, mass = sc.wgrad_ref(x, dy, tuple(got.shape), 3, 1, groups=x.shape[1])
    sc.assert_close(got, ref, mass, got.dtype, what, "depthwise_wgrad")


def a_stem_conv_fwd(R, r, what):
    T = r.scalars["dtype"]
    w = _weights(R, r, "wp", "stem_pack_weights")
    ref, mass = _bias(*sc.conv_ref(r.b("img").to(T), w, 3, 2), r.b("bias"))
    ref, mass, e_act = _act_res(ref, mass, r.scalars["act"], None)
    got = r.r(0)
    sc.assert_close(got, ref, mass, got.dtype, what, "stem", e_act=e_act)
    _stats(r, "stats_acc", got, what)


def a_stem_wgrad(R, r, what):
    dy = r.b("dy")
    got = r.r(0)
    ref, mass = sc.wgrad_ref(r.b("img").to(dy.dtype), dy, tuple(got.shape), 3, 2)
    sc.assert_close(got, ref, mass, got.dtype, what, "stem_wgrad")


def a_stem_bn_wgrad(R, r, what):
    act = r.scalars["act"]
    ref = ssb.reference(r.b("img"), r.b("dout"), r.b("y"), r.b("scale"), r.b("shift"), r.b("mean"), r.b("invstd"), r.b("gamma"),
                        act, dz_exact=not act)
    ssb.check(r.r(0), r.r(1), r.r(2), ref, what)


def a_stem_im2col(R, r, what):
    sm.assert_exact(r.r(0), emu.stem_im2col(r.b("img"), r.scalars["dtype"]), what, "exact")


def a_stem_pack_weights(R, r, what):
    got = r.r(0)
    sm.assert_exact(got.reshape(-1), emu.stem_pack_weights(r.b("w"), r.scalars["dtype"]).reshape(-1), what, "pack")


def a_stem_unpack_wgrad(R, r, what):
    sm.assert_exact(r.r(0), emu.stem_unpack_wgrad(r.b("dw32"), r.scalars["w_dtype"]), what, "exact")


def a_pack_weights(R, r, what):
    """layout-free: the packed matrix holds exactly the rounded weights, and zeros (see the module docstring)"""
    w, got = r.b("w").to(r.scalars["dtype"]), r.r(0)
    if got.shape == w.shape:                                   # the stand-ins' handle: the OIHW tensor itself
        return sm.assert_exact(got, w, what, "pack")
    have, want = torch.unique(sm.bits(got)), torch.unique(sm.bits(w))
    zero = sm.bits(torch.zeros(1, dtype=got.dtype))
    extra = have[~torch.isin(have, torch.cat([want, zero]))]
    missing = want[~torch.isin(want, have)]
    assert extra.numel() == 0 and missing.numel() == 0, \
        f"{what}: {extra.numel()} values of the packed matrix are no weight, {missing.numel()} weights are not in it"
    if r.scalars["mode"] == 0:
        nz_got, nz_want = sm.bits(got)[sm.bits(got) != zero], sm.bits(w)[sm.bits(w) != zero]
        assert torch.equal(torch.sort(nz_got.reshape(-1))[0], torch.sort(nz_want.reshape(-1))[0]), \
            f"{what}: the forward matrix is not a permutation of the weights plus zeros"


# -- BatchNorm
def _count(y):
    return y.numel() // y.shape[1]


def _within(got, ref_noise, dtype, what, family):
    sb.assert_within(got, ref_noise, dtype, what, family)


def _coef(r, s, q, n, got, what, ds=0.0, dq=0.0):
    """mean, invstd, scale, shift and the running statistics against coef_fwd of the sums (s, q) the kernel read"""
    rm, rv = r.b("running_mean"), r.b("running_var")
    k = sb.coef_fwd(s, q, n, r.scalars["eps"], r.b("gamma"), r.b("beta"), rm, rv, r.scalars["momentum"], ds, dq)
    for g, nm in zip(got, ("mean", "invstd", "scale", "shift")):
        _within(g, k[nm], torch.float32, f"{what} {nm}", "bn_coef")
    for arg, nm in (("running_mean", "rmean"), ("running_var", "rvar")):
        try:
            _within(r.a(arg), k[nm], rm.dtype, f"{what} {arg}", "bn_coef")
        except AssertionError as e:
            raise ReplayMismatch(str(e), r.ordinal, r.op, arg, e) from None


def a_bn_act_fwd_train(R, r, what):
    y = r.b("y")
    s, q = sb.fold(r.b("acc"), y.shape[1])
    _coef(r, s, q, _count(y), [r.r(i) for i in (1, 2, 3, 4)], what)
    _within(r.r(0), sb.fwd_apply(y, r.r(3), r.r(4), r.scalars["act"], r.b("res")), y.dtype, what + " out", "bn_fwd")


def a_bn_train_stats(R, r, what):
    y = r.b("y")
    t = sb.sums_fwd(y, y.dtype)
    _coef(r, t["s"][0], t["q"][0], _count(y), [r.r(i) for i in range(4)], what, t["s"][1], t["q"][1])


def a_bn_act_fwd(R, r, what):
    y = r.b("y")
    _within(r.r(0), sb.fwd_apply(y, r.b("scale"), r.b("shift"), r.scalars["act"], r.b("res")), y.dtype, what + " out", "bn_fwd")


def _bn_bwd(r, what, acc):
    dout, y, gamma = r.b("dout"), r.b("y"), r.b("gamma")
    dz, ddz, dga = sb.bwd_dz(dout, y, r.b("scale"), r.b("shift"), r.scalars["act"])
    sums = sb.sums_bwd(dz, ddz, dga, y)
    n = _count(y)
    if acc is not None:
        _within(acc[0], sums["s"], torch.float32, what + " sum dz", "bn_bwd_sum")
        _within(acc[1], sums["q"], torch.float32, what + " sum dz y", "bn_bwd_sumsq")
        k = sb.coef_bwd(acc[0], acc[1], n, gamma, r.b("mean"), r.b("invstd"), gamma.dtype)
    else:
        k = sb.coef_bwd(sums["s"][0], sums["q"][0], n, gamma, r.b("mean"), r.b("invstd"), gamma.dtype, sums["s"][1], sums["q"][1])
    dy, dgamma, dbeta = r.r(0), r.r(1), r.r(2)
    _within(dbeta, k["dbeta"], gamma.dtype, what + " dbeta", "bn_dbeta")
    _within(dgamma, k["dgamma"], gamma.dtype, what + " dgamma", "bn_dgamma")
    _within(dy, sb.bwd_apply(dz, ddz, y, k["A"], k["B"], k["D"], k["dB"], k["dD"]), y.dtype, what + " dy", "bn_dy")


def a_bn_act_bwd_train(R, r, what):
    before = r.b("acc")
    if bool((before != 0).any()):
        raise ReplayMismatch(f"backward sums' slice not zero before the launch ({int((before != 0).sum())} entries)", r.ordinal, r.op, "acc")
    c = r.b("y").shape[1]
    _bn_bwd(r, what, sb.fold(r.a("acc"), c))


def a_bn_act_bwd(R, r, what):
    _bn_bwd(r, what, None)


def a_bn_act_bwd_eval(R, r, what):
    y = r.b("y")
    dz, ddz, _ = sb.bwd_dz(r.b("dout"), y, r.b("scale"), r.b("shift"), r.scalars["act"])
    _within(r.r(0), sb.bwd_apply(dz, ddz, y, r.b("scale")), y.dtype, what + " dy", "bn_dy")


def a_bn_eval_coeffs(R, r, what):
    e = sb.coef_eval(r.b("gamma"), r.b("beta"), r.b("running_mean"), r.b("running_var"), r.scalars["eps"])
    _within(r.r(0), e["scale"], torch.float32, what + " scale", "bn_coef")
    _within(r.r(1), e["shift"], torch.float32, what + " shift", "bn_coef")


def a_channel_sum(R, r, what):
    x = r.b("x")
    _within(r.r(0), sb.sums_fwd(x, x.dtype)["s"], torch.float32, what, "bn_sum")


# -- memory-bound
def taps(idx, shape):
    """recorded argmax -> kh * 5 + kw, (N, C, H, W) uint8: the device stores that (NHWC bytes), the stand-in ATen's flat index"""
    n, c, h, w = shape
    if idx.dtype == torch.uint8:
        return idx.reshape(n, h, w, c).permute(0, 3, 1, 2)
    i = idx.reshape(n, c, h, w).to(torch.int64)
    kh = torch.div(i, w, rounding_mode="floor") - torch.arange(h).view(1, 1, h, 1) + 2
    kw = i % w - torch.arange(w).view(1, 1, 1, w) + 2
    return (kh * 5 + kw).to(torch.uint8)


def a_maxpool5_fwd(R, r, what):
    x = r.b("x")
    sm.check_pool_fwd(x, r.r(0), taps(r.r(1), x.shape), what)


def a_maxpool5_bwd(R, r, what):
    dout = r.b("dout")
    sm.check_pool_bwd(dout, taps(r.b("idx"), dout.shape), r.r(0), what, base=r.b("acc_into"))


def a_upsample2x_fwd(R, r, what):
    sm.check_up_fwd(r.b("x"), r.r(0), what)


def a_upsample2x_bwd(R, r, what):
    sm.check_up_bwd(r.b("dout"), r.r(0), what, base=r.b("acc_into"))


def a_copy_channels(R, r, what):
    sm.check_copy(r.b("src"), r.b("dst"), r.a("dst"), what, bool(r.scalars["accumulate"]))


def a_add_n(R, r, what):
    sm.check_add([s.view() for s in r.before["xs"]], r.r(0), what)


def a_to_nhwc(R, r, what):
    sm.check_cast(r.b("x"), r.r(0), what)


def a_head_group(R, r, what):
    pack = r.scalars["pack"]
    pb, pa = r.b("preds"), r.a("preds")
    want = pb.clone()
    for i, (c_off, m_off) in enumerate(zip(r.scalars["c_offs"], r.scalars["m_offs"])):
        bb, ba = r.before["branches"][i].view(), r.after["branches"][i].view()
        n, c, h, w = bb.shape
        if pack:
            want[:, c_off:c_off + c, m_off:m_off + h * w] = bb.reshape(n, c, h * w)
        else:
            sm.assert_exact(ba, pb[:, c_off:c_off + c, m_off:m_off + h * w].reshape(n, c, h, w), f"{what} branch {i}", "exact")
    sm.assert_exact(pa, want, what + " preds", "exact")


def a_zero_(R, r, what):
    sm.assert_exact(r.a("t"), torch.zeros_like(r.a("t")), what, "exact")


def a_fill_(R, r, what):
    sm.assert_exact(r.a("t"), torch.full_like(r.a("t"), r.scalars["v" if "v" in r.scalars else "value"]), what, "exact")


def a_scale_inplace(R, r, what):
    sm.check_cast(r.b("x"), r.a("x"), what, scale=float(r.b("scale_dev").reshape(-1)[0]))


# -- attention
def _route(stash, n, heads, t, dtype):
    if dtype == torch.float32:
        return "fp32"
    return "fused" if stash.numel() * stash.element_size() == n * heads * t * 4 else "gemm"


def _stash_views(route, stash, b, t, dtype):
    if route != "gemm":
        st = stash if stash.dtype == torch.float32 else stash.view(torch.float32)
        return st.reshape(b, t, 1).double(), None
    tp = (t + 31) // 32 * 32
    pm = stash.view(dtype).reshape(b, t, tp)
    assert not bool(pm[..., t:].any()), "stashed P: pad columns not zero"
    return None, pm[..., :t].double()


def _attn_geom(r):
    qkv = r.b("qkv")
    n, _, h, w = qkv.shape
    heads, dk, dh = r.scalars["heads"], r.scalars["dk"], r.scalars["dh"]
    return qkv, n, h * w, heads, dk, dh, r.scalars["scale"]


def a_attn_fwd(R, r, what):
    qkv, n, t, heads, dk, dh, scale = _attn_geom(r)
    o, vp, stash = r.r(0), r.r(1), r.r(2)
    route = _route(stash, n, heads, t, qkv.dtype)
    q, k, v = sa.split_qkv(qkv, heads, dk, dh)
    lse, pm = _stash_views(route, stash.contiguous(), n * heads, t, qkv.dtype)
    sa.check_forward(route, q, k, v, scale, qkv.dtype, sa.split(o, heads), got_lse=lse, got_p=pm, what=f"{what} [{route}]", guard=False)
    sm.assert_exact(vp, sa.merge(v, n, *qkv.shape[2:]).to(qkv.dtype), what + " vp", "exact")


def a_attn_fwd_nograd(R, r, what):
    qkv, n, t, heads, dk, dh, scale = _attn_geom(r)
    route = "fused" if t <= 448 else "long"
    q, k, v = sa.split_qkv(qkv, heads, dk, dh)
    sa.check_forward(route, q, k, v, scale, qkv.dtype, sa.split(r.r(0), heads), what=f"{what} [{route}]", guard=False)
    sm.assert_exact(r.r(1), sa.merge(v, n, *qkv.shape[2:]).to(qkv.dtype), what + " vp", "exact")


def a_attn_bwd(R, r, what):
    qkv, n, t, heads, dk, dh, scale = _attn_geom(r)
    stash = r.b("lse" if "lse" in r.before else "stash")
    route = _route(stash, n, heads, t, qkv.dtype)
    q, k, v = sa.split_qkv(qkv, heads, dk, dh)
    lse, pm = _stash_views(route, stash.contiguous(), n * heads, t, qkv.dtype)
    d_vp = r.b("d_vp")
    sa.check_backward(route, q, k, v, sa.split(r.b("d_o"), heads), None if d_vp is None else sa.split(d_vp, heads), scale, qkv.dtype,
                      *sa.split_qkv(r.r(0), heads, dk, dh), o=sa.split(r.b("o"), heads), lse=lse, p_stash=pm, what=f"{what} [{route}]",
                      guard=False)


# -- loss
def a_loss_fwd_bwd(R, r, what):
    """strict_loss.verify on what the launch left: out, dpreds and, from its workspace, the decoded boxes and the assignment
    (the stand-in returns no workspace: this adapter runs on the device only)"""
    import strict_loss as sl
    preds = r.b("preds")
    n, _, a = preds.shape
    n_gt, nc = r.scalars["n_gt"], r.scalars["nc"]
    ws = r.results[-1].view()
    if ws.dtype != torch.uint8:
        raise ReplayMismatch("no workspace among the results: nothing to take the decoded boxes and the assignment from", r.ordinal, r.op, "result")
    off = r.b("gt_off").tolist()
    gt = r.b("gt").reshape(-1, 5).float()
    gs = r.b("grad_scale")
    case = sl.Case(preds.float(), r.b("anchors").float(), r.b("strides").float(), [gt[off[i]:off[i + 1]] for i in range(n)], nc,
                   preds.dtype, what, lam=(r.scalars["lambda_dfl"], r.scalars["lambda_cls"]),
                   grad_scale=None if gs is None else float(gs.reshape(-1)[0]))
    na = n * a
    pbox = ws[:na * 16].contiguous().view(torch.float32).view(n, a, 4)
    idx = ws[na * 16:na * 16 + 4 * max(n_gt, 1)].contiguous().view(torch.int32)[:n_gt]
    sl.verify(case, r.r(0), r.r(1) if len(r.results) == 3 else None, pbox, idx)


def _loss_case_args(r):
    preds = r.b("preds")
    off = r.b("gt_off").tolist()
    gt = r.b("gt").reshape(-1, 5).float()
    gs = r.b("grad_scale")
    gts = [gt[off[i]:off[i + 1]] for i in range(preds.shape[0])]
    return preds, gts, (None if gs is None else float(gs.reshape(-1)[0]))


def tal_state(r):
    """strict_tal.State of a recorded loss_tal_fwd_bwd launch, from its workspace (the stand-ins return none)"""
    import strict_tal as st
    preds, gts, _ = _loss_case_args(r)
    n, _, a = preds.shape
    ws = r.results[-1].view()
    if ws.dtype != torch.uint8:
        raise ReplayMismatch("no workspace among the results", r.ordinal, r.op, "result")
    views = ops.loss_tal_workspace_views(ws.contiguous(), n, a, r.scalars["n_gt"])
    live = sum(g.shape[0] for g in gts)
    return st.State.from_views(views, live, r.r(0), r.r(1) if len(r.results) == 3 else None)


def a_loss_tal_fwd_bwd(R, r, what):
    """strict_tal.verify on what the launch left: the decoded boxes, the top-k lists, owners and targets from its workspace,
    out[4] and dpreds (device only, as loss_fwd_bwd)"""
    import strict_tal as st
    preds, gts, gs = _loss_case_args(r)
    sc_ = r.scalars
    hyper = dict(topk=sc_["topk"], alpha=sc_["alpha"], beta=sc_["beta"], box=sc_["lambda_box"], cls=sc_["lambda_cls"], dfl=sc_["lambda_dfl"])
    case = st.Case(preds.float(), r.b("anchors").float(), r.b("strides").float(), gts, sc_["nc"], preds.dtype, what, hyper=hyper, grad_scale=gs)
    st.verify(case, tal_state(r))


def dflqfl_assignment(r):
    """(G,) anchor index per ground-truth row, from the workspace of a recorded loss_fwd_bwd launch"""
    preds = r.b("preds")
    na, n_gt = preds.shape[0] * preds.shape[2], r.scalars["n_gt"]
    ws = r.results[-1].view()
    return ws[na * 16:na * 16 + 4 * max(n_gt, 1)].contiguous().view(torch.int32)[:n_gt].long()


# -- the whole pass's ground truth: boxes that put positives on every pyramid level
def level_of(anchor, size):
    """pyramid level (0, 1, 2 = stride 8, 16, 32) of a flat anchor index of a size x size input"""
    n8, n16 = (size // 8) ** 2, (size // 16) ** 2
    anchor = torch.as_tensor(anchor)
    return (anchor >= n8).long() + (anchor >= n8 + n16).long()


def whole_pass_targets(n_img, size, seed):
    """Per image: for each stride s in (8, 16, 32) boxes of 7 pixels centred ON anchor points of that level (two of stride 8,
    six of stride 16, all nine of stride 32).  Every anchor point of another level is at least 4 pixels away along an axis (the centres are
    s / 2 + k s), so such a box holds exactly ONE anchor point: the task-aligned assignment has one candidate for it, on that
    level, whatever the predictions are.  Then one box of 30 .. 60 pixels and six of 7 .. 40 pixels anywhere: the DFL / QFL loss
    assigns each row the anchor whose DECODED centre is nearest, which on an untrained net scatters by a fraction of the stride
    round the anchor point (up to half a cell at stride 32), so no geometry fixes its level; the rows are many enough that
    every level is taken over the batch, which the device test asserts from the launch's workspace.  Rows cx, cy, w, h, class."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n_img):
        rows = []
        for s, count in ((8, 2), (16, 6), (32, 9)):
            cells = size // s
            pick = torch.randperm(cells * cells, generator=g)[:count]
            for c in pick.tolist():
                rows.append([s / 2 + (c % cells) * s, s / 2 + (c // cells) * s, 7.0, 7.0, float(torch.randint(0, 80, (1,), generator=g))])
        wh = torch.rand(2, generator=g) * 30 + 30
        rows.append([size / 2 + float(torch.rand(1, generator=g)) * 10 - 5, size / 2 + float(torch.rand(1, generator=g)) * 10 - 5,
                     float(wh[0]), float(wh[1]), float(torch.randint(0, 80, (1,), generator=g))])
        for _ in range(6):
            wh = torch.rand(2, generator=g) * 33 + 7
            c = torch.rand(2, generator=g) * (size - 40) + 20
            rows.append([float(c[0]), float(c[1]), float(wh[0]), float(wh[1]), float(torch.randint(0, 80, (1,), generator=g))])
        out.append(torch.tensor(rows, dtype=torch.float32))
    return out


ROWS_PER_IMAGE, SMALL_ROWS = 24, 17           # rows per image; the first 17 are the 7-pixel boxes


ADAPTERS = {n[2:]: f for n, f in list(globals().items()) if n.startswith("a_") and callable(f)}


# ---------------------------------------------------------------------------------------------- the replay
def _guard(r):
    """unwritten arguments bit-equal; of written ones every byte outside the view bit-equal"""
    written = WRITES.get(r.op, ())
    masks = {}
    for arg, s in r.before.items():
        for sb_, sa_ in zip(s if isinstance(s, list) else [s], r.after[arg] if isinstance(s, list) else [r.after[arg]]):
            if arg in written:
                m = masks.get(sb_.ptr)
                masks[sb_.ptr] = sb_.mask() if m is None else (m | sb_.mask())
    for arg, s in r.before.items():
        for sb_, sa_ in zip(s if isinstance(s, list) else [s], r.after[arg] if isinstance(s, list) else [r.after[arg]]):
            diff = (_raw(sb_.whole) != _raw(sa_.whole)).view(sb_.whole.numel(), -1).any(1)
            if sb_.ptr in masks:
                diff &= ~masks[sb_.ptr]
            if bool(diff.any()):
                first = diff.nonzero().flatten()[:8].tolist()
                kind = "outside its view" if arg in written else "although the leaf does not write it"
                raise ReplayMismatch(f"{int(diff.sum())} elements of the whole buffer changed {kind}; first at flat offsets {first} "
                                     f"(view offset {sb_.offset}, shape {sb_.shape}, strides {sb_.stride})", r.ordinal, r.op, arg)


def shares():
    """family -> largest share of its bound used so far: excess / c for the 2^-24 M families, the budget share itself elsewhere"""
    return {f: v[0] / (1.0 if f in sc.BUDGET_FAMILIES else sc.C.get(f, sc.C_DEFAULT)) for f, v in sc.OBSERVED.items()}


def replay(R, unchecked=(), only=None):
    """Every record (or those with an ordinal in `only`) through the guard and its adapter.  -> {leaf: largest share of a bound
    used by its records}.  Raises ReplayMismatch naming the launch (ordinal, op) and the argument."""
    per_leaf = {}
    R.family_share = getattr(R, "family_share", {})            # family -> largest share used by THIS recording's records
    for r in R.records:
        if only is not None and r.ordinal not in only:
            continue
        if r.returned_none:                                    # "not taken" (conv_fwd_act / dw_fwd_act / attn_fwd_nograd): nothing ran
            continue
        _guard(r)
        fn = ADAPTERS.get(r.op)
        if fn is None:
            if r.op in unchecked:
                continue
            raise ReplayMismatch("no adapter for this leaf", r.ordinal, r.op, "-")
        before = {f: v[0] for f, v in sc.OBSERVED.items()}
        for v in sc.OBSERVED.values():
            v[0] = float("-inf")
        try:
            fn(R, r, f"launch {r.ordinal} {r.op}")
        except ReplayMismatch:
            raise
        except AssertionError as e:
            raise ReplayMismatch(str(e), r.ordinal, r.op, _blame(R, r, fn), e) from None
        finally:
            now = shares()
            for f, v in sc.OBSERVED.items():
                v[0] = max(v[0], before.get(f, float("-inf")))
        for f, v in now.items():
            if v > float("-inf"):
                R.family_share[f] = max(R.family_share.get(f, float("-inf")), v)
        used = max([v for v in now.values() if v > float("-inf")], default=float("-inf"))
        per_leaf[r.op] = max(per_leaf.get(r.op, float("-inf")), used)
    return per_leaf


def _zeroed(snap):
    z = object.__new__(Snap)
    for f in Snap.__slots__:
        setattr(z, f, getattr(snap, f))
    z.whole = torch.zeros_like(snap.whole)
    return z


def _blame(R, r, fn):
    """The argument a failing record's error comes from.  For each source the launch was to ADD (acc_into, acc2, res) the
    residual is tested against that source's prior contents: the adapter runs again on the record with that one source zeroed,
    and if the result then fits its bound, the launch left exactly that source out -- it alone is named.  Otherwise: the link
    arguments the record was given (the error is not the omission of one source)."""
    for arg in ("acc2", "acc_into", "res"):
        if isinstance(r.before.get(arg), Snap):
            alt = Record(r.ordinal, r.op, r.depth)
            alt.before, alt.after, alt.results, alt.scalars, alt.owner = dict(r.before), r.after, r.results, r.scalars, r.owner
            alt.before[arg] = _zeroed(r.before[arg])
            saved = {f: list(v) for f, v in sc.OBSERVED.items()}
            try:
                fn(R, alt, "hypothesis")
                return arg
            except AssertionError:
                pass
            finally:
                sc.OBSERVED.clear()
                sc.OBSERVED.update(saved)
    if r.op == "maxpool5_bwd":
        # the residual against the prior contents again: got - acc_into holds, per (image, channel), the whole of dout when
        # every window's gradient was routed SOMEWHERE (each element rounded once: one spacing of T per pixel allowed);
        # what is left wrong is then where it went -- the idx
        base, got, d = r.b("acc_into"), r.r(0), r.b("dout").double()
        b = torch.zeros_like(d) if base is None else base.double()
        room = sc.ulp(torch.maximum(got.double().abs(), b.abs()), got.dtype).sum((2, 3)) + 64 * sc.U24 * (d.abs() + b.abs()).sum((2, 3))
        if bool((((got.double() - b).sum((2, 3)) - d.sum((2, 3))).abs() <= room).all()):
            return "idx"
    given = [a for a in ("acc_into", "acc2", "res", "out", "stats_acc", "acc", "idx", "dst") if r.before.get(a) is not None]
    return ", ".join(given) if given else "result"


def _producer(R, g):
    """ordinal of the launch whose last write of a buffer `g` is, bit for bit: by g's own memory where autograd kept the
    tensor, else by value (AccumulateGrad copies a gradient whose strides are not the parameter's)"""
    lw = R.last_write(g)
    g = g.detach().cpu()
    if lw is not None:
        assert torch.equal(_raw(g), _raw(lw[1])), f"a gradient differs from what launch {lw[0]} {R.records[lw[0]].op} wrote to its memory"
        return lw[0]
    want = _raw(g)
    for r in reversed(R.records):
        outs = r.results + [s_ for a, s_ in r.after.items() if a in WRITES.get(r.op, ()) and isinstance(s_, Snap)]
        for s_ in outs:
            if s_.shape == tuple(g.shape) and s_.dtype == g.dtype and R.shadow[s_.ptr][1] == r.ordinal and torch.equal(_raw(s_.view()), want):
                return r.ordinal
    return None


def identities(R, params, x=None, allow_missing=("head.dfl.conv.weight",)):
    """params: {name: parameter}.  Every .grad bit-equal to the recorded output of the launch that produced it; x.grad
    bit-equal to the last recorded write of its buffer; no input of any launch unexplained.  -> {name: ordinal}"""
    made = {}
    for name, p in params.items():
        if not p.requires_grad:
            continue
        hit = None if p.grad is None else _producer(R, p.grad)
        if hit is None:
            assert name in allow_missing, f"{name}: its gradient is the last recorded write of no buffer"
            continue
        made[name] = hit
    if x is not None:
        assert _producer(R, x.grad) is not None, "the input's gradient is the last recorded write of no buffer"
    assert not R.unexplained, f"inputs that differ from the last recorded write of their memory, with no writer seen: {R.unexplained}"
    return made


def family_counts(R):
    """launches per conv family, for the report"""
    fam = {}
    for r in R.records:
        if r.op.startswith(("conv_", "dw_", "stem_")):
            t = next((s for s in (r.before.get("x"), r.before.get("dy"), r.before.get("img")) if s is not None), None)
            low = "depthwise" if r.op.startswith("dw_") else "stem" if r.op.startswith("stem_") else "auto"
            f = _fam(t.dtype if t is not None and not r.op.startswith("stem_") else torch.bfloat16, low) + ("_wgrad" if "wgrad" in r.op else "")
            fam[f] = fam.get(f, 0) + 1
    return fam
