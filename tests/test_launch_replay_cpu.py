"""Proof of tests/launch_replay.py without a GPU: the eleven blocks of the wiring tests run through the recorder and the
replayer over the stand-ins of tests/emulated_ops.py.  The stand-ins must pass -- every launch inside 1 x its leaf's bound,
the guard and the identities intact -- and every mutant (ONE stand-in with ONE thing changed, the suite's mutant convention)
must fail, naming the right launch and argument.

The BatchNorm stand-ins are refined here (BN_STAND_INS): emulated_ops forms the coefficients in fp32 and ignores the
backward's accumulator; the kernels fold the sums and form every coefficient in double, round each published value once
and leave (sum dz, sum dz y) in the accumulator, which is what strict_bn.py's limits describe and what the adapters read
(the stand-in of tests/test_strict_bn_cpu.py does the same).  Attention likewise: emulated_ops differentiates the exact
softmax, the kernels recompute P from the stored log-sum-exp and take D from the stored o, which is what
strict_attention.py bounds: the stand-ins here are the fused route of tests/test_strict_attention_cpu.py.

STAND_IN_MAXIMA: largest share of each family's bound used by the stand-ins (limit 1), printed by
test_stand_in_maxima_are_inside_one; recorded 2026-10-20 on the parent commit f54efa2:
    auto 0.02   auto_wgrad 0.15   fp32 0.33   fp32_wgrad 0.25   depthwise 0.16   depthwise_wgrad 0.09
    bn_coef 0.90   bn_fwd 0.55   bn_dy 0.59   bn_bwd_sum 0.01   bn_bwd_sumsq 0.02   bn_dgamma 0.01   bn_dbeta 0.01   move_pool 0.37
    attn_fused o 0.52  lse 0.03  dq 0.66  dk 0.59  dv 0.58     attn_fp32 o 0.03  lse 0.04  dq 0.06  dk 0.07  dv 0.06
(the conv families as excess / c, c = 16; every other family is its share of the noise budget)."""
import pytest
import torch

import emulated_ops as emu
import launch_replay as lr
import strict_attention as sa
import strict_bn as sb
import strict_compare as sc
import test_strict_attention_cpu as tsa
import wiring_trace as wt
from conftest import load_golden
from oracle.params import det_fill_
from src.hipops import functions as F_
from src.hipops import ops

BF, F32 = torch.bfloat16, torch.float32
STAND_IN_MAXIMA = {}        # filled by the tests of this module as they run; asserted at the end


def _bc(t):
    return t.view(1, -1, 1, 1)


def _coef(s, q, cnt, gamma, beta, rm, rv, momentum, eps):
    """bn_fwd_coef of the kernels: from the double sums, in double, each published value rounded once"""
    m = s / cnt
    var = (q / cnt - m * m).clamp_min(0.0)
    invstd, mean = ((var + sb.f32_of(eps)) ** -0.5).float(), m.float()
    scale = gamma.float() * invstd
    shift = beta.float() - mean * scale
    mom = torch.tensor(momentum, dtype=F32)
    unbiased = (var * (cnt / (cnt - 1.0)) if cnt > 1 else var).float()
    rm.copy_(((1.0 - mom) * rm.float() + mom * mean).to(rm.dtype))
    rv.copy_(((1.0 - mom) * rv.float() + mom * unbiased).to(rv.dtype))
    return mean, invstd, scale, shift


def bn_act_fwd_train(y, acc, gamma, beta, running_mean, running_var, momentum, eps, act, res=None, out=None):
    c = y.shape[1]
    s, q = acc.view(ops.BN_REPL, 2, c).double().sum(0)
    mean, invstd, scale, shift = _coef(s, q, y.numel() // c, gamma, beta, running_mean, running_var, momentum, eps)
    return emu.bn_act_fwd(y, scale, shift, act, res, out), mean, invstd, scale, shift


def bn_train_stats(y, gamma, beta, running_mean, running_var, momentum, eps):
    yd = y.double()
    return _coef(yd.sum((0, 2, 3)), (yd * yd).sum((0, 2, 3)), y.numel() // y.shape[1], gamma, beta, running_mean, running_var, momentum, eps)


def _bn_bwd(dout, y, scale, shift, mean, invstd, gamma, act, acc=None):
    yf = y.float()
    cnt = y.numel() // y.shape[1]
    dz = dout.float() * emu._act_grad(yf * _bc(scale) + _bc(shift), act)
    s, q = dz.double().sum((0, 2, 3)), (dz * yf).double().sum((0, 2, 3))
    if acc is not None:                                       # the kernel leaves its two sums in the accumulator and reads them back
        a = acc.view(ops.BN_REPL, 2, -1)
        a[0, 0] += s.float()
        a[0, 1] += q.float()
        s, q = a.double().sum(0)
    inv, mu = invstd.double(), mean.double()
    dg = inv * (q - mu * s)
    k0, c1, c2 = gamma.double() * inv, s / cnt, dg / cnt
    a_, b_, d_ = k0.float(), (-k0 * c2 * inv).float(), (-k0 * c1 + k0 * c2 * mu * inv).float()
    dy = (_bc(a_) * dz + _bc(b_) * yf + _bc(d_)).to(y.dtype)
    return emu._nhwc(dy), dg.float().to(gamma.dtype), s.float().to(gamma.dtype)


def bn_act_bwd(dout, y, scale, shift, mean, invstd, gamma, act):
    return _bn_bwd(dout, y, scale, shift, mean, invstd, gamma, act)


def bn_act_bwd_train(dout, y, scale, shift, mean, invstd, gamma, act, acc):
    return _bn_bwd(dout, y, scale, shift, mean, invstd, gamma, act, acc)


def _heads(t, heads):
    return sa.split(t, heads).float()


def attn_fwd(qkv, heads, dk, dh, scale):
    """the fused route as tests/test_strict_attention_cpu.py models it: probabilities rounded to T, o rounded once, fp32 lse"""
    n, _, h, w = qkv.shape
    q, k, v = (x.float() for x in sa.split_qkv(qkv, heads, dk, dh))
    o, lse = tsa.fwd_fused(q, k, v, scale, qkv.dtype)
    return (emu._nhwc(sa.merge(o, n, h, w).to(qkv.dtype)), emu._nhwc(sa.merge(v, n, h, w).to(qkv.dtype)), lse.reshape(-1).float())


def attn_bwd(qkv, o, d_o, d_vp, lse, heads, dk, dh, scale):
    """from the STORED o and lse, dS rounded to T: the fused route's backward"""
    n, _, h, w = qkv.shape
    q, k, v = (x.float() for x in sa.split_qkv(qkv, heads, dk, dh))
    got = tsa.bwd("fused", q, k, v, _heads(d_o, heads), None if d_vp is None else _heads(d_vp, heads), scale, qkv.dtype,
                  o=_heads(o, heads), lse=lse.reshape(n * heads, h * w, 1))
    return emu._nhwc(sa.merge(torch.cat(got, -1), n, h, w).to(qkv.dtype))


BN_STAND_INS = {"attn_fwd": attn_fwd, "attn_bwd": attn_bwd, "bn_act_fwd_train": bn_act_fwd_train, "bn_train_stats": bn_train_stats, "bn_act_bwd": bn_act_bwd,
                "bn_act_bwd_train": bn_act_bwd_train}


def _outside_autocast(fn):
    import functools

    @functools.wraps(fn)
    def plain(*args, **kwargs):
        with torch.autocast("cpu", enabled=False):
            return fn(*args, **kwargs)
    return plain


def _channels(m):
    return [c.conv.out_channels for c in m.modules() if hasattr(c, "norm") and hasattr(c, "conv")]


def run_block(monkeypatch, tag, dtype, mode="default", mutant=None, shape=None, nchw=False, chunk_link=True):
    """training forward and backward of one block over the stand-ins (one of them replaced by `mutant` = (name, fn)), recorded.
    mode: default (accumulators per layer, as the wiring trace), arena (one zeroed pool, bn_act_bwd_train), deterministic.
    nchw: x and dy come as the goldens are (to_nhwc runs, as in the committed trace).  chunk_link=False: C3K2 without its
    ChunkLink (functions.CHUNK_LINK, the A/B switch): Chunk2.backward then ADDS the block's gradient with copy_channels"""
    from test_wiring_cpu import _blocks
    gd = load_golden("block_" + tag)
    m = torch.nn.ModuleDict({"m": _blocks()[tag]()})
    det_fill_(m.state_dict(), int(gd["seed"]))
    m.train()
    x, dy = gd["x"], gd["dy"]
    if shape is not None:
        g = torch.Generator().manual_seed(5)
        x = torch.randn(x.shape[0], x.shape[1], *shape, generator=g)
        dy = torch.randn(dy.shape[0], dy.shape[1], *shape, generator=g)
    emu.install(monkeypatch)
    for name, fn in BN_STAND_INS.items():
        monkeypatch.setattr(ops, name, fn)
    if mutant is not None:
        monkeypatch.setattr(ops, mutant[0], mutant[1])
    for name in emu.LEAVES:                                   # a kernel does not know about autocast: neither does its stand-in
        monkeypatch.setattr(ops, name, _outside_autocast(getattr(ops, name)))
    monkeypatch.setattr(F_, "DETERMINISTIC", mode == "deterministic")
    monkeypatch.setattr(F_, "CHUNK_LINK", chunk_link)
    R = lr.install(monkeypatch)
    xin = (x.to(dtype).clone() if nchw else emu._nhwc(x.to(dtype))).requires_grad_(True)
    dy = dy.to(dtype).clone() if nchw else emu._nhwc(dy.to(dtype))
    with R.mode:
        if mode == "arena":
            F_.BnArena.current = F_.BnArena(xin.device, F_.BnArena.elems_for(_channels(m)))
        try:
            with torch.autocast("cpu", dtype=dtype, enabled=dtype != F32):
                y = m["m"](xin)
        finally:
            F_.BnArena.current = None
        y.backward(dy)
    monkeypatch.undo()
    return R, m, xin


def _note(per_leaf):
    for f, v in lr.shares().items():
        STAND_IN_MAXIMA[f] = max(STAND_IN_MAXIMA.get(f, float("-inf")), v)


@pytest.mark.parametrize("mode", ["default", "arena", "deterministic"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("tag", wt.BLOCK_TAGS)
def test_stand_ins_stay_inside_one_times_the_bound(tag, dtype, mode, monkeypatch):
    R, m, x = run_block(monkeypatch, tag, dtype, mode)
    per_leaf = lr.replay(R)
    _note(per_leaf)
    made = lr.identities(R, dict(m.named_parameters()), x)
    assert set(made) == {k for k, p in m.named_parameters()}
    dn = "fp32" if dtype == F32 else "bf16"
    assert R.foreign_writers() == lr.pinned_writers("cpu")[f"{tag}-{dn}-{mode}"]
    for f, v in R.family_share.items():
        assert v <= 1.0, (f, v)


@pytest.mark.parametrize("tag", ["c3k2_res", "c3k2_csp"])
def test_stand_ins_on_a_map_that_is_no_multiple_of_16(tag, monkeypatch):
    R, m, x = run_block(monkeypatch, tag, BF, "arena", shape=(13, 11))
    _note(lr.replay(R))
    lr.identities(R, dict(m.named_parameters()), x)


@pytest.mark.parametrize("tag", ["c3k2_res", "c3k2_csp"])
def test_stand_ins_without_the_chunk_link(tag, monkeypatch):
    """the path on which Chunk2.backward accumulates with copy_channels (no block reaches it with the link on)"""
    R, m, x = run_block(monkeypatch, tag, BF, chunk_link=False)
    assert any(r.op == "copy_channels" and r.scalars["accumulate"] for r in R.records)
    _note(lr.replay(R))
    lr.identities(R, dict(m.named_parameters()), x)


def test_the_default_mode_records_the_committed_launch_trace(monkeypatch):
    """the recorder sees what wiring_trace.Tracer sees: op for op the committed trace of the block (fp32, per-layer accumulators)"""
    import json
    import os
    from conftest import GOLDEN
    with open(os.path.join(GOLDEN, "wiring_trace.json")) as f:
        fixture = json.load(f)
    for tag in wt.BLOCK_TAGS:
        R, _, _ = run_block(monkeypatch, tag, F32, nchw=True)
        got = [r.op for r in R.records if r.op in fixture["leaves"] and r.depth == 0]
        assert got == [w["op"] for w in fixture["blocks"][tag]], tag


def test_stand_in_maxima_are_inside_one():
    assert STAND_IN_MAXIMA, "nothing was recorded: this test closes the module, run it with the stand-in tests above"
    print("\n[launch_replay] CPU stand-ins, largest share of the bound used per family:")
    for f, v in sorted(STAND_IN_MAXIMA.items()):
        print(f"[launch_replay]   {f:18s} {v:8.3f}")
    assert all(v <= 1.0 for v in STAND_IN_MAXIMA.values())


# ---------------------------------------------------------------------------------------------- the whole pass's boxes
@pytest.mark.parametrize("seed", [12, 13, 14])
def test_the_whole_pass_boxes_put_positives_on_every_level(seed):
    """launch_replay.whole_pass_targets at 96 x 96, three images, against tests/tal_ref.py and strict_loss.assign_cpu on the
    predictions of an untrained head (small logits: decoded centres near their anchor points): both assignments have a
    positive on each of the three levels -- the task-aligned one in every image and whatever the predictions are (the one
    candidate of each 7-pixel box), the nearest-decoded-centre one over the batch.  The device test asserts the same from the
    recorded workspaces, where the predictions are the model's own."""
    import strict_loss as sl
    import tal_ref as tr
    size, n = 96, 3
    gts = lr.whole_pass_targets(n, size, 12)
    for g in gts:
        assert g.shape == (lr.ROWS_PER_IMAGE, 5) and float(g[:, :2].min()) > 3.5 and float(g[:, :2].max()) < size - 3.5
    anchors, strides = tr.make_anchors(size, size)
    preds = 0.1 * torch.randn(n, 64 + 80, anchors.shape[1], generator=torch.Generator().manual_seed(seed))
    pbox = tr.decode(preds.double(), anchors.double(), strides.double())
    asg = tr.assign(preds.double(), pbox, anchors.double(), strides.double(), gts, tr.DEFAULTS)
    for i in range(n):
        levels = set(lr.level_of((asg["label"][i] >= 0).nonzero().flatten(), size).tolist())
        assert levels == {0, 1, 2}, (seed, i, levels)
    for j, lst in enumerate(asg["lists"]):                    # a 7-pixel box has its one candidate, whatever the predictions
        if j % lr.ROWS_PER_IMAGE < lr.SMALL_ROWS:
            assert len(lst) == 1, (j, lst)
    case = sl.Case(preds, anchors, strides, gts, 80, F32, "whole pass boxes")
    idx = sl.assign_cpu(case, sl.decode64(case)[0])
    assert set(lr.level_of(idx, size).tolist()) == {0, 1, 2}, seed          # over the batch: see whole_pass_targets


# ---------------------------------------------------------------------------------------------- mutants
def m_acc_into_ignored(dy, wb, cin, h, w, k, stride, acc_into=None, acc2=None):
    if acc_into is None:
        return emu.conv_dgrad(dy, wb, cin, h, w, k, stride, None, acc2)
    acc_into.data.copy_(emu.conv_dgrad(dy, wb, cin, h, w, k, stride, None, acc2))
    return acc_into


def m_acc2_ignored(dy, wb, cin, h, w, k, stride, acc_into=None, acc2=None):
    return emu.conv_dgrad(dy, wb, cin, h, w, k, stride, acc_into, None)


def m_acc_into_shifted(dy, wb, cin, h, w, k, stride, acc_into=None, acc2=None):
    """lands one 16-channel block further down the concat gradient (where the buffer has room)"""
    if acc_into is not None and acc_into.storage_offset() >= 16:
        dx = emu.conv_dgrad(dy, wb, cin, h, w, k, stride, None, acc2)
        moved = acc_into.as_strided(acc_into.shape, acc_into.stride(), acc_into.storage_offset() - 16)
        moved.data.copy_((moved.float() + dx.float()).to(moved.dtype))
        return acc_into
    return emu.conv_dgrad(dy, wb, cin, h, w, k, stride, acc_into, acc2)


def m_res_skipped(y, acc, gamma, beta, running_mean, running_var, momentum, eps, act, res=None, out=None):
    return bn_act_fwd_train(y, acc, gamma, beta, running_mean, running_var, momentum, eps, act, None, out)


def m_stats_start_at_one(c, device):
    return torch.ones(ops.BN_REPL * 2 * c, dtype=F32, device=device)


def m_biased_running_var(y, acc, gamma, beta, running_mean, running_var, momentum, eps, act, res=None, out=None):
    c = y.shape[1]
    cnt = y.numel() // c
    rv = running_var.clone()
    got = bn_act_fwd_train(y, acc, gamma, beta, running_mean, running_var, momentum, eps, act, res, out)
    s = acc.view(ops.BN_REPL, 2, c).sum(0)
    mean = s[0] / cnt
    running_var.copy_(rv * (1 - momentum) + momentum * (s[1] / cnt - mean * mean).clamp_min(0))
    return got


def m_copy_overwrites(src, dst, accumulate=False):
    dst.copy_(src)


def m_idx_shifted(dout, idx, acc_into=None):
    return emu.maxpool5_bwd(dout, (idx + 1).clamp_(max=dout.shape[2] * dout.shape[3] - 1), acc_into)


def m_wgrad_drops_last_image(x, dy, k, stride, w_dtype):
    return emu.conv_wgrad(x[:-1], dy[:-1], k, stride, w_dtype)


def m_write_past_slice(y, acc, gamma, beta, running_mean, running_var, momentum, eps, act, res=None, out=None):
    got = bn_act_fwd_train(y, acc, gamma, beta, running_mean, running_var, momentum, eps, act, res, out)
    if out is not None:
        n, c, h, w = out.shape
        if out.storage_offset() % out.stride(3) + c < out.stride(3):          # a channel past the slice exists in the row
            out.as_strided((n, c + 1, h, w), out.stride(), out.storage_offset())[:, c] = 7.0
    return got


# (mutant, stand-in it replaces, function, block, mode, the launch that must be named, a word of the argument named)
MUTANTS = [
    ("acc_into ignored", "conv_dgrad", m_acc_into_ignored, "residual", "default", "conv_dgrad", "acc_into"),
    ("acc2 ignored", "conv_dgrad", m_acc2_ignored, "c3k2_res", "default", "conv_dgrad", "acc2"),
    ("acc_into one 16-channel block off", "conv_dgrad", m_acc_into_shifted, "c3k2_csp", "default", "conv_dgrad", "acc_into"),
    ("res skipped", "bn_act_fwd_train", m_res_skipped, "residual", "default", "bn_act_fwd_train", "res"),
    ("statistics start at 1.0", "bn_acc_new", m_stats_start_at_one, "conv1x1_id", "default", "conv_fwd", "stats_acc"),
    ("running_var biased", "bn_act_fwd_train", m_biased_running_var, "conv3x3s2", "default", "bn_act_fwd_train", "running_var"),
    ("copy_channels overwrites", "copy_channels", m_copy_overwrites, "c3k2_res", "no_chunk_link", "copy_channels", "dst"),
    ("pool idx one tap off", "maxpool5_bwd", m_idx_shifted, "sppf", "default", "maxpool5_bwd", "idx"),
    ("wgrad drops the last image", "conv_wgrad", m_wgrad_drops_last_image, "conv1x1_id", "default", "conv_wgrad", "result"),
    ("write one channel past the slice", "bn_act_fwd_train", m_write_past_slice, "c3k", "default", "bn_act_fwd_train", "out"),
]


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mutant", MUTANTS, ids=[m[0].replace(" ", "_") for m in MUTANTS])
def test_every_mutant_fails_and_names_its_launch(mutant, dtype, monkeypatch):
    what, name, fn, tag, mode, op, arg = mutant
    R, m, x = run_block(monkeypatch, tag, dtype, mode.replace("no_chunk_link", "default"), mutant=(name, fn),
                        chunk_link=mode != "no_chunk_link")
    with pytest.raises(lr.ReplayMismatch) as e:
        lr.replay(R)
    print(f"[mutant] {what}: launch {e.value.ordinal} {e.value.op} [{e.value.arg}]")
    assert e.value.op == op and e.value.arg == arg, (what, e.value.ordinal, e.value.op, e.value.arg, str(e.value)[:300])
