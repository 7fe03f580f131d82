"""-m gpu: every launch of real blocks, of the stem and of one whole training pass held to its leaf's own derived bound.

The real autograd Functions run on the real HIP leaves; tests/launch_replay.py records every launch (every tensor argument's
whole buffer before and after, every result) and replays each record against a float64 reference built from what the
device itself read -- see that module for the principle, the adapters and the guard.  Cases, the smallest that reach every
branch (the module prints the launch counts per leaf and per conv family when it finishes):

  blocks     the eleven tags of wiring_trace.BLOCK_TAGS at their golden x / dy shapes, cast to bf16, f16 and fp32; training
             forward and backward with per-layer accumulators (`default`, as the committed CPU trace), with the arena a
             Model.forward provides (`arena`: bn_act_bwd_train) and in deterministic mode; then fused and in eval mode
             (conv_fwd_act / dw_fwd_act); the two C3K2 tags also at 13 x 11 (partial tiles meet the slice arguments) and
             without their ChunkLink (copy_channels(accumulate=True) from Chunk2.backward)
  stem       Conv(3, 16, k=3, s=2) on an fp32 image, output 19 x 21, bf16 and f16 with STEM_BWD_FUSED on and off, and fp32
             (the unfold route: stem_im2col, stem_unpack_wgrad)
  eval       four tags in eval mode, forward and backward, from an NCHW fp32 input (to_nhwc, bn_eval_coeffs, bn_act_bwd_eval)
  whole pass preset n, 3 images of 96 x 96 (P5 is 3 x 3), bf16 autocast through TrainStepRunner(use_graph=False)._fwd_bwd
             with YoloDFLQFLoss and with YoloTALoss: the deferred weight gradients are recorded on the side stream; replayed
             by backbone, neck and head over one recorded pass.  The loss launches go through strict_loss.verify and
             strict_tal.verify, on the workspace the launch left.  The seeded boxes (launch_replay.whole_pass_targets) put
             positives on every level in every image: proved on the CPU against tests/tal_ref.py, asserted here from the
             recorded workspaces
  trace      the fp32 `default` block runs launch what tests/golden/wiring_trace.json says, but for DEVICE_ONLY below
  coverage   the leaves recorded over the module are the leaves functions.py names, minus UNREACHED (each with its reason)
"""
import json
import os

import pytest
import torch

import launch_replay as lr
import strict_compare as sc
import strict_move as sm
import wiring_trace as wt
from conftest import GOLDEN, load_golden
from oracle.params import det_fill_

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "fp32": torch.float32}
SEEN, PER_LEAF, COUNTS, FAMILIES, WRITERS = set(), {}, {}, {}, {}
# leaves functions.py names that no case here can reach, and why
UNREACHED = {
    "add_n": "only functions.Fanout calls it, and no module of src/model uses fanout()",
}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n" + sc.report())
    print(sm.report())
    print("[launch_replay] launches per leaf, largest share of its bound used:")
    for leaf in sorted(COUNTS):
        print(f"[launch_replay]   {leaf:20s} {COUNTS[leaf]:6d}   {PER_LEAF.get(leaf, float('nan')):8.3f}")
    print(f"[launch_replay] launches per conv family: {dict(sorted(FAMILIES.items()))}")
    dump = os.environ.get("YOLO_REPLAY_DUMP")
    if dump:
        with open(dump, "w") as f:
            json.dump(WRITERS, f, indent=0, sort_keys=True)


def _ops():
    from src.hipops import ops
    return ops


def nhwc(t, dtype):
    out = _ops().new_nhwc(*t.shape, dtype, DEV)
    out.copy_(t)
    return out


def _block(tag, seed):
    from test_wiring_cpu import _blocks
    m = torch.nn.ModuleDict({"m": _blocks()[tag]()})
    det_fill_(m.state_dict(), seed)
    return m.to(DEV)


def _channels(m):
    return [c.conv.out_channels for c in m.modules() if hasattr(c, "norm") and hasattr(c, "conv")]


def _inputs(tag, shape):
    gd = load_golden("block_" + tag)
    x, dy = gd["x"], gd["dy"]
    if shape is not None:
        g = torch.Generator().manual_seed(5)
        x = torch.randn(x.shape[0], x.shape[1], *shape, generator=g)
        dy = torch.randn(dy.shape[0], dy.shape[1], *shape, generator=g)
    return int(gd["seed"]), x, dy


def _tally(R, per_leaf):
    for leaf, n in R.counts().items():
        COUNTS[leaf] = COUNTS.get(leaf, 0) + n
    for leaf, v in per_leaf.items():
        PER_LEAF[leaf] = max(PER_LEAF.get(leaf, float("-inf")), v)
    for f, n in lr.family_counts(R).items():
        FAMILIES[f] = FAMILIES.get(f, 0) + n
    SEEN.update(R.counts())


def _pinned(key, R):
    WRITERS[key] = R.foreign_writers()
    want = lr.pinned_writers("gpu")
    assert key in want, f"{key}: no pinned list of non-leaf writers; this run saw {WRITERS[key]}"
    assert WRITERS[key] == want[key], (key, sorted(set(WRITERS[key]) ^ set(want[key])))


def train_block(monkeypatch, tag, dtype, mode, shape=None, chunk_link=True):
    from src.hipops import functions as F_
    seed, x, dy = _inputs(tag, shape)
    m = _block(tag, seed).train()
    monkeypatch.setattr(F_, "DETERMINISTIC", mode == "deterministic")
    monkeypatch.setattr(F_, "CHUNK_LINK", chunk_link)
    R = lr.install(monkeypatch)
    xin = nhwc(x, dtype).requires_grad_(True)
    g = nhwc(dy, dtype)
    torch.cuda.synchronize()
    with R.mode:
        if mode == "arena":
            F_.BnArena.current = F_.BnArena(xin.device, F_.BnArena.elems_for(_channels(m)))
        try:
            with torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
                y = m["m"](xin)
        finally:
            F_.BnArena.current = None
        y.backward(g)
        torch.cuda.synchronize()
    monkeypatch.undo()
    return R, m, xin


def _check_training(R, m, x, key):
    WRITERS[key] = R.foreign_writers()
    per_leaf = lr.replay(R)
    _tally(R, per_leaf)
    made = lr.identities(R, dict(m.named_parameters()), x)
    assert set(made) == {k for k, _ in m.named_parameters()}
    _pinned(key, R)
    for f, v in R.family_share.items():
        assert v <= 1.0, (f, v)


@pytest.mark.parametrize("mode", ["default", "arena", "deterministic"])
@pytest.mark.parametrize("dn", list(DTYPES))
@pytest.mark.parametrize("tag", wt.BLOCK_TAGS)
def test_block_training_pass(tag, dn, mode, monkeypatch):
    R, m, x = train_block(monkeypatch, tag, DTYPES[dn], mode)
    _check_training(R, m, x, f"{tag}-{dn}-{mode}")
    ops_seen = R.counts()
    if mode == "arena":
        assert "bn_act_bwd_train" in ops_seen and "bn_act_bwd" not in ops_seen
    if mode == "deterministic":
        assert "bn_train_stats" in ops_seen and "bn_act_fwd_train" not in ops_seen


@pytest.mark.parametrize("dn", list(DTYPES))
@pytest.mark.parametrize("tag", ["c3k2_res", "c3k2_csp"])
def test_c3k2_on_a_map_that_is_no_multiple_of_16(tag, dn, monkeypatch):
    R, m, x = train_block(monkeypatch, tag, DTYPES[dn], "arena", shape=(13, 11))
    _check_training(R, m, x, f"{tag}-{dn}-arena-13x11")
    assert any(r.op == "conv_dgrad" and r.before.get("acc_into") is not None and r.before["acc_into"].offset % r.before["acc_into"].stride[3]
               for r in R.records), "no data gradient was added into a slice of the concat gradient"


@pytest.mark.parametrize("dn", list(DTYPES))
@pytest.mark.parametrize("tag", ["c3k2_res", "c3k2_csp"])
def test_c3k2_without_its_chunk_link(tag, dn, monkeypatch):
    R, m, x = train_block(monkeypatch, tag, DTYPES[dn], "default", chunk_link=False)
    assert any(r.op == "copy_channels" and r.scalars["accumulate"] for r in R.records)
    _check_training(R, m, x, f"{tag}-{dn}-nochunklink")


def _fuse(m):
    from src.model.model_blocks import Conv
    from src.utils.model_utils import fuse_conv
    for c in m.modules():
        if type(c) is Conv and hasattr(c, "norm"):
            c.conv = fuse_conv(c.conv, c.norm)
            c.forward = c.fuse_forward
            delattr(c, "norm")
    return m


@pytest.mark.parametrize("dn", list(DTYPES))
@pytest.mark.parametrize("tag", wt.BLOCK_TAGS)
def test_block_fused_inference(tag, dn, monkeypatch):
    dtype = DTYPES[dn]
    seed, x, _ = _inputs(tag, None)
    m = _fuse(_block(tag, seed).eval())
    R = lr.install(monkeypatch)
    xin = nhwc(x, dtype)
    torch.cuda.synchronize()
    with R.mode, torch.no_grad(), torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
        m["m"](xin)
        torch.cuda.synchronize()
    monkeypatch.undo()
    _tally(R, lr.replay(R))
    taken = {r.op for r in R.records if not r.returned_none}
    if dtype != torch.float32:
        if tag not in ("conv1x1_id", "attention"):             # those two hold identity convs only: conv_fwd + bias
            assert taken & {"conv_fwd_act", "dw_fwd_act"}, sorted(taken)
        if tag in ("attention", "psablock", "psa"):
            assert "attn_fwd_nograd" in taken, sorted(taken)
    _pinned(f"{tag}-{dn}-fused", R)
    for f, v in R.family_share.items():
        assert v <= 1.0, (f, v)


@pytest.mark.parametrize("dn", ["bf16", "fp32"])
@pytest.mark.parametrize("tag", ["conv3x3s2", "convdw", "residual", "sppf"])
def test_block_eval_mode_forward_and_backward(tag, dn, monkeypatch):
    """frozen statistics (bn_eval_coeffs, bn_act_fwd, bn_act_bwd_eval) from an NCHW fp32 input (to_nhwc)"""
    dtype = DTYPES[dn]
    seed, x, dy = _inputs(tag, None)
    m = _block(tag, seed).eval()
    R = lr.install(monkeypatch)
    xin = x.to(DEV).requires_grad_(True)
    g = nhwc(dy, dtype)
    torch.cuda.synchronize()
    with R.mode:
        with torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
            y = m["m"](xin)
        y.backward(g)
        torch.cuda.synchronize()
    monkeypatch.undo()
    _tally(R, lr.replay(R))
    seen = R.counts()
    assert {"to_nhwc", "bn_eval_coeffs", "bn_act_fwd", "bn_act_bwd_eval"} <= set(seen), sorted(seen)
    norm = {k for k, _ in m.named_parameters() if ".norm." in k}
    assert norm and all(p.grad is None for k, p in m.named_parameters() if k in norm), "frozen statistics: BatchNorm's parameters take no gradient"
    made = lr.identities(R, {k: p for k, p in m.named_parameters() if k not in norm})
    assert set(made) == {k for k, _ in m.named_parameters()} - norm
    # the input's gradient: autograd itself casts the first conv's data gradient to the fp32 input's type, and in Residual
    # (eval mode: no link) adds the skip gradient, which is the incoming gradient, to it -- both already cast
    dx = [r for r in R.records if r.op in ("conv_dgrad", "dw_dgrad")][-1].r(0)
    want = (g.cpu().float() + dx.float()) if tag == "residual" else dx.float()
    assert torch.equal(xin.grad.cpu(), want.contiguous()), "the input's gradient is not the last data gradient (+ skip), cast"
    _pinned(f"{tag}-{dn}-eval", R)
    for f, v in R.family_share.items():
        assert v <= 1.0, (f, v)


def test_regression_second_accumulate_source_on_the_valu_path_rounds_once(monkeypatch):
    """C3K2(16, 32, 1, False, 4): the Residual's conv1 has 4 output channels, so its data gradient takes the VALU kernel, with
    acc_into (the concat gradient's slice) AND acc2 (the skip gradient).  That path added acc2 in a second pass, a second
    rounding to bf16: up to 221 ulp off where the three terms cancel (this launch, found by this module).  Now one rounding."""
    R, m, x = train_block(monkeypatch, "c3k2_res", torch.bfloat16, "default")
    hit = [r for r in R.records if r.op == "conv_dgrad" and r.before.get("acc2") is not None and r.before["dy"].shape[1] == 4]
    assert hit, "no data gradient with a second accumulate source and 4 output channels was launched"
    lr.replay(R, only=[r.ordinal for r in hit])
    assert R.family_share["auto"] <= 1.0, R.family_share


@pytest.mark.parametrize("fused", [True, False], ids=["one_pass", "three_launches"])
@pytest.mark.parametrize("dn", ["bf16", "f16", "fp32"])
def test_stem_training_pass(dn, fused, monkeypatch):
    from torch import nn
    from src.hipops import functions as F_
    from src.model.model_blocks import Conv
    dtype = DTYPES[dn]
    torch.manual_seed(3)
    m = torch.nn.ModuleDict({"m": Conv(3, 16, nn.SiLU(), k=3, s=2, p=1)}).to(DEV).train()
    g = torch.Generator().manual_seed(31)
    img = (torch.randn(2, 3, 38, 42, generator=g) + 0.5).to(DEV)               # output 19 x 21
    dy = nhwc(torch.randn(2, 16, 19, 21, generator=g), dtype)
    monkeypatch.setattr(F_, "STEM_BWD_FUSED", fused)
    R = lr.install(monkeypatch)
    torch.cuda.synchronize()
    with R.mode:
        with torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
            y = m["m"](img)
        y.backward(dy)
        torch.cuda.synchronize()
    monkeypatch.undo()
    _tally(R, lr.replay(R))
    seen = R.counts()
    if "stem_conv_fwd" in seen:
        assert ("stem_bn_wgrad" in seen) == fused and ("stem_wgrad" in seen) == (not fused)
    else:                                                      # the unfold route, where stem_conv_eligible() declines
        assert {"stem_im2col", "stem_unpack_wgrad"} <= set(seen) and dtype == torch.float32, sorted(seen)
    made = lr.identities(R, dict(m.named_parameters()))
    assert set(made) == {k for k, _ in m.named_parameters()}
    _pinned(f"stem-{dn}-{'one_pass' if fused else 'three_launches'}", R)
    for f, v in R.family_share.items():
        assert v <= 1.0, (f, v)


# ---------------------------------------------------------------------------------------------- one whole training pass
NANO = dict(csp=[False, True], depth=[1] * 6, width=[3, 16, 32, 64, 128, 256])
SIZE = 96
_PASSES = {}


def _whole_pass(loss_name):
    """one recorded pass per loss, shared by the tests below; a pass that raised is not run again: its exception is kept"""
    if loss_name in _PASSES:
        hit = _PASSES[loss_name]
        if isinstance(hit, BaseException):
            raise RuntimeError(f"the recorded pass with {loss_name} failed in an earlier test; it is not run again") from hit
        return hit
    try:
        _PASSES[loss_name] = _record_whole_pass(loss_name)
    except BaseException as e:
        _PASSES[loss_name] = e
        raise
    return _PASSES[loss_name]


def _record_whole_pass(loss_name):
    from src.model import losses
    from src.model.model_builder import Model
    from src.training.graph_step import TrainStepRunner
    mp = pytest.MonkeyPatch()
    img = torch.randn(3, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(12)).to(DEV)
    gts = [g.to(DEV) for g in lr.whole_pass_targets(3, SIZE, 12)]      # positives on every level: see that function
    torch.manual_seed(0)
    model = Model(**NANO, num_classes=80).to(DEV).train()
    crit = getattr(losses, loss_name)(num_classes=80)
    opt = torch.optim.AdamW(model.parameters(), lr=0.0, weight_decay=0.0)
    runner = TrainStepRunner(model, crit, opt, "bfloat16", use_graph=False)
    packed = losses.PackedTargets(gts, img.device)
    R = lr.install(mp)
    torch.cuda.synchronize()
    try:
        with R.mode:
            runner._fwd_bwd(img, packed)
            torch.cuda.synchronize()
    finally:
        mp.undo()
    return R, model


def _parts(R, model):
    """backbone / neck / head of every record: by the parameter or buffer among its arguments, or -- a weight gradient, which
    takes none -- by the parameter whose .grad its result is; a record with neither (copies, pools, attention, the loss)
    belongs where the record before it does"""
    where = {}
    for part in ("net", "fpn", "head"):
        sub = getattr(model, part)
        for t in list(sub.parameters()) + list(sub.buffers()):
            where[t.untyped_storage().data_ptr()] = part
            if getattr(t, "grad", None) is not None:
                where[t.grad.untyped_storage().data_ptr()] = part
    out, cur = [], "net"
    for r in R.records:
        snaps = [s_ for v in r.before.values() for s_ in (v if isinstance(v, list) else [v])] + r.results
        cur = next((where[s_.ptr] for s_ in snaps if s_.ptr in where), cur)
        out.append(cur)
    return out


@pytest.mark.parametrize("part", ["net", "fpn", "head"])
@pytest.mark.parametrize("loss_name", ["YoloDFLQFLoss", "YoloTALoss"])
def test_whole_pass_launches(loss_name, part):
    R, model = _whole_pass(loss_name)
    parts = _parts(R, model)
    only = [i for i, p in enumerate(parts) if p == part]
    assert len(only) > 100, (part, len(only))
    per_leaf = lr.replay(R, only=set(only))
    if part == "net":
        _tally(R, {})
    for leaf, v in per_leaf.items():
        PER_LEAF[leaf] = max(PER_LEAF.get(leaf, float("-inf")), v)
    for f, v in R.family_share.items():
        assert v <= 1.0, (f, v)


@pytest.mark.parametrize("loss_name", ["YoloDFLQFLoss", "YoloTALoss"])
def test_whole_pass_assigns_positives_on_every_level(loss_name):
    """from the loss launch's own workspace: assigned anchors on each of the three pyramid levels -- in every image for the
    task-aligned assignment, over the batch for the nearest-decoded-centre one -- so the positive branches of the loss kernel
    ran on every level (the boxes: launch_replay.whole_pass_targets, proved on the CPU
    against tests/tal_ref.py by tests/test_launch_replay_cpu.py)"""
    R, model = _whole_pass(loss_name)
    (r,) = [r for r in R.records if r.op in ("loss_fwd_bwd", "loss_tal_fwd_bwd")]
    if loss_name == "YoloTALoss":
        label = lr.tal_state(r).label
        per_image = [(label[i] >= 0).nonzero().flatten() for i in range(3)]
    else:
        idx = lr.dflqfl_assignment(r)
        assert idx.numel() == 3 * lr.ROWS_PER_IMAGE
        print(f"\n[launch_replay] DFL / QFL assignment, level per row: {lr.level_of(idx, SIZE).tolist()}")
        per_image = [idx]
    for i, anchors in enumerate(per_image):
        levels = set(lr.level_of(anchors, SIZE).tolist())
        assert levels == {0, 1, 2}, (loss_name, i, sorted(levels), anchors.tolist())


@pytest.mark.parametrize("loss_name", ["YoloDFLQFLoss", "YoloTALoss"])
def test_whole_pass_identities(loss_name):
    from src.hipops import functions as F_
    R, model = _whole_pass(loss_name)
    made = lr.identities(R, dict(model.named_parameters()))
    assert set(made) == {k for k, _ in model.named_parameters()} - {"head.dfl.conv.weight"}
    seen = R.counts()
    loss_leaf = "loss_fwd_bwd" if loss_name == "YoloDFLQFLoss" else "loss_tal_fwd_bwd"
    assert seen.get(loss_leaf) == 1 and seen.get("channel_sum", 0) > 0 and seen.get("upsample2x_bwd", 0) > 0
    assert F_.WGRAD_GROUP < seen["conv_wgrad"], "fewer weight gradients than one sync group: the queue never synced"
    _pinned(f"whole-{loss_name}", R)


# ---------------------------------------------------------------------------------------------- device trace vs CPU trace
# What the device launches differently from the committed CPU trace (tests/golden/wiring_trace.json), each with the condition
# in functions.py / ops.py it comes from.  Anything else fails.
DEVICE_ONLY = {
    "wgrad_first": "_wgrad_overlapped: `OVERLAP_WGRAD and x.is_cuda` issues conv_wgrad on the side stream BEFORE the data gradient "
                   "(pack_weights, conv_dgrad); the CPU path runs dgrad_fn() first",
    "out_none": "ops.conv_wgrad / dw_wgrad / channel_sum / stem_im2col / stem_unpack_wgrad take `out=` (the deferred _param_grad path, "
                "`x.is_cuda and LAZY_WGRAD_JOIN`); None in these runs, absent from the stand-ins' signatures",
    "stash": "ops.attn_bwd's fifth argument is the forward's `stash` (bytes) where the stand-in takes `lse`: its name, shape and type",
    "idx": "ops.maxpool5_fwd returns idx as NHWC bytes (kh * 5 + kw); the stand-in ATen's int64 NCHW index: shape and type of maxpool5_bwd.idx",
    "fill_name": "ops.fill_(t, value) where the stand-in names it v",
    "packed": "ops.pack_weights returns the K-major packed matrix (flat, padded); the stand-in's handle is the OIHW tensor: the "
              "shape of conv_fwd.wp and conv_dgrad.wb",
}


def _normalise(records):
    """the device trace brought to the CPU trace's conventions by exactly the DEVICE_ONLY substitutions"""
    recs = json.loads(json.dumps(records))
    order, i = [], 0
    while i < len(recs):                                       # wgrad_first: move each conv_wgrad behind the data gradient that follows it
        if recs[i]["op"] == "conv_wgrad":
            j = i + 1
            while j < len(recs) and recs[j]["op"] in ("pack_weights",):
                j += 1
            if j < len(recs) and recs[j]["op"] == "conv_dgrad":
                order += list(range(i + 1, j + 1)) + [i]
                i = j + 1
                continue
        order.append(i)
        i += 1
    new_of = {old: new for new, old in enumerate(order)}
    out = []
    for old in order:
        r = recs[old]
        for arg, link in r["links"].items():
            if isinstance(link, list) and len(link) == 2 and isinstance(link[0], int) and link[0] >= 0:
                link[0] = new_of[link[0]]
        if r["scalars"].get("out", 0) is None and r["op"] in ("conv_wgrad", "dw_wgrad", "channel_sum", "stem_im2col", "stem_unpack_wgrad"):
            del r["scalars"]["out"]                            # out_none
            r["links"].pop("out", None)
        if r["op"] == "attn_bwd" and "stash" in r["tensors"]:  # stash
            r["tensors"]["lse"] = "device-only"
            del r["tensors"]["stash"]
        if r["op"] == "maxpool5_bwd":                          # idx
            r["tensors"]["idx"] = "device-only"
        for op_, arg_ in (("conv_fwd", "wp"), ("conv_dgrad", "wb")):                   # packed
            if r["op"] == op_:
                r["tensors"][arg_] = "device-only"
        if r["op"] == "fill_" and "value" in r["scalars"]:     # fill_name
            r["scalars"]["v"] = r["scalars"].pop("value")
        out.append(r)
    return out


def _cpu_view(records):
    recs = json.loads(json.dumps(records))
    for r in recs:
        if r["op"] == "attn_bwd":
            r["tensors"]["lse"] = "device-only"
        if r["op"] == "maxpool5_bwd":
            r["tensors"]["idx"] = "device-only"
        for op_, arg_ in (("conv_fwd", "wp"), ("conv_dgrad", "wb")):
            if r["op"] == op_:
                r["tensors"][arg_] = "device-only"
    return recs


@pytest.mark.parametrize("tag", wt.BLOCK_TAGS)
def test_device_launch_trace_is_the_cpu_trace(tag, monkeypatch):
    from src.hipops import ops
    with open(os.path.join(GOLDEN, "wiring_trace.json")) as f:
        want = _cpu_view(json.load(f)["blocks"][tag])
    gd = load_golden("block_" + tag)
    m = _block(tag, int(gd["seed"])).train()
    x = gd["x"].to(DEV).requires_grad_(True)
    tr = wt.Tracer()
    for name in wt.traced_leaves():
        monkeypatch.setattr(ops, name, tr.wrap(name, getattr(ops, name)))
    m["m"](x).backward(gd["dy"].to(DEV))
    torch.cuda.synchronize()
    monkeypatch.undo()
    got = _normalise(tr.records)
    diffs = [f"launch {i}: device {g['op']} {json.dumps(g, sort_keys=True)[:400]}\n          cpu    {w['op']} {json.dumps(w, sort_keys=True)[:400]}"
             for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not diffs and len(got) == len(want), f"{tag}: {len(got)} device launches, {len(want)} in the CPU trace\n" + "\n".join(diffs[:6])


def test_every_named_leaf_was_recorded():
    named = set(lr.named_leaves())
    missing = named - SEEN
    print(f"\n[launch_replay] leaves recorded: {len(SEEN & named)} of {len(named)}; not reached: {sorted(missing)}")
    assert set(UNREACHED) <= named
    assert len(COUNTS) >= 20, "nothing was recorded: this test closes the module, run it with the cases above"
    assert missing == set(UNREACHED) - SEEN and not (set(UNREACHED) & SEEN), (sorted(missing), sorted(set(UNREACHED) & SEEN))
