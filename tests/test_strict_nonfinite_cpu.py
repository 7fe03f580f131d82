"""No GPU: proof of the propagation rule of tests/strict_nonfinite.py on CPU stand-ins.

  * honest stand-ins pass it: fp32 F.conv2d, conv2d_input, conv2d_weight (dense and depthwise), a plain softmax attention
    with its autograd backward, a two-pass BatchNorm -- on cases of the GPU module's own tables;
  * deliberately leaky stand-ins are rejected, with the family and the element set the defect predicts: zero padding done
    as 'load the clamped pixel, multiply by a 0 / 1 mask'; 8 channels read past Cin against zero-padded weights; masked key
    columns multiplied by p = 0 where the clamped row belongs to the next image; a NaN swallowed by nan_to_num; BatchNorm
    statistics that leak into the next channel;
  * every case of tests/nonfinite_cases.py lies inside the two refusal conditions (dep neither empty nor above half of the
    output, no exact zero in a multiplying operand) and reaches the kernel variant it names (the plan query needs no GPU);
  * attention_dep()'s table is what perturbing the inputs of strict_attention's float64 reference shows."""
import pytest
import torch
import torch.nn.functional as F

import nonfinite_cases as nc
import strict_attention as sa
import strict_compare as sc
import strict_nonfinite as sn
from nonfinite_cases import BF, F32, HF, N

NAN = float("nan")


@pytest.fixture(autouse=True)
def _threads():
    torch.set_num_threads(4)


def by_id(id_):
    return next(c for c in nc.DENSE if c["id"] == id_)


# ------------------------------------------------------------------------------------------------- stand-ins
def conv_fwd(x, w, k, s, groups=1):
    """the kernels' contract on the CPU: 16-bit operands, fp32 accumulation, one rounding"""
    return F.conv2d(x.float(), w.float(), None, s, k // 2, 1, groups).to(x.dtype)


def conv_dgrad(dy, w, in_shape, k, s, groups=1):
    return torch.nn.grad.conv2d_input(tuple(in_shape), w.float(), dy.float(), s, k // 2, 1, groups).to(dy.dtype)


def conv_wgrad(x, dy, w_shape, k, s, groups=1):
    return torch.nn.grad.conv2d_weight(x.float(), tuple(w_shape), dy.float(), s, k // 2, 1, groups)


def conv_clamped_mask(x, w, k, s):
    """LEAKY (3x3, stride 1): a padding tap loads the pixel at the CLAMPED flattened (image, row, column) index and multiplies it
    by a 0 / 1 mask -- above the first row that is pixel 0 of the batch, below an image's last row the next image's first row"""
    n, c, h, wd = x.shape
    xf = x.float().permute(0, 2, 3, 1).reshape(n * h * wd, c)
    hh, ww = torch.arange(h).view(1, h, 1), torch.arange(wd).view(1, 1, wd)
    flat = (torch.arange(n).view(n, 1, 1) * h + hh) * wd + ww
    y = torch.zeros(n, w.shape[0], h, wd)
    for kh in range(3):
        for kw in range(3):
            idx = (flat + (kh - 1) * wd + (kw - 1)).clamp(0, n * h * wd - 1)
            valid = ((hh + kh - 1 >= 0) & (hh + kh - 1 < h) & (ww + kw - 1 >= 0) & (ww + kw - 1 < wd)).expand(n, h, wd).float()
            tap = xf[idx] * valid.unsqueeze(-1)                                  # (N, H, W, C): the mask by multiplication
            y += torch.einsum("nhwc,oc->nohw", tap, w[:, :, kh, kw].float())
    return y.to(x.dtype)


def conv_reads_past_cin(xbuf, off, cin, w, k, s):
    """LEAKY: the K loop runs 8 channels past Cin of the wider buffer; the weights are zero-padded there"""
    wide = xbuf[:, off:off + cin + 8].float()
    wpad = torch.cat([w.float(), torch.zeros(w.shape[0], 8, k, k)], 1)
    return F.conv2d(wide, wpad, None, s, k // 2).to(xbuf.dtype)


def conv_swallows(x, w, k, s):
    """WRONG: a NaN / inf in the input is replaced before the products"""
    return conv_fwd(torch.nan_to_num(x.float(), nan=0.0, posinf=0.0, neginf=0.0).to(x.dtype), w, k, s)


def attention(qkv, heads, dk, dh, leaky=False):
    """(N, heads * (2 dk + dh), H, W) -> o (N, heads * dh, H, W).  leaky: the key loop runs to the next multiple of 64; a row
    past T is the clamped row of the FLATTENED (image, token) buffer -- the next image's first tokens -- and its probability
    is multiplied by a 0 / 1 mask instead of being skipped"""
    n, c, h, w = qkv.shape
    t = h * w
    x = qkv.float().reshape(n, heads, c // heads, t)
    q, k, v = x[:, :, :dk].transpose(2, 3), x[:, :, dk:2 * dk].transpose(2, 3), x[:, :, 2 * dk:].transpose(2, 3)     # (N, heads, T, d)
    if not leaky:
        p = torch.softmax(q @ k.mT * dk ** -0.5, -1)
        o = p @ v
    else:
        tp = (t + 63) // 64 * 64
        kf, vf = k.transpose(0, 1).reshape(heads, n * t, dk), v.transpose(0, 1).reshape(heads, n * t, dh)
        o = torch.empty(n, heads, t, dh)
        for i in range(n):
            idx = (i * t + torch.arange(tp)).clamp_max(n * t - 1)
            s_ = q[i] @ kf[:, idx].mT * dk ** -0.5
            valid = (torch.arange(tp) < t).float()
            s_ = torch.where(valid.bool(), s_, torch.full_like(s_, -1e30))
            p = torch.softmax(s_, -1) * valid                                   # p = 0 by multiplication
            o[i] = p @ vf[:, idx]
    return o.transpose(2, 3).reshape(n, heads * dh, h, w).to(qkv.dtype)


def batchnorm(y, gamma, beta, eps=1e-3, leaky=False):
    """two passes, fp32; leaky: channel c's mean is blended with 0 x the next channel's sum"""
    yf = y.float()
    mean = yf.mean((0, 2, 3))
    if leaky:
        mean = mean + 0.0 * torch.roll(yf.sum((0, 2, 3)), -1)
    var = ((yf - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
    inv = (var + eps).rsqrt()
    out = (yf - mean.view(1, -1, 1, 1)) * (gamma * inv).view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    return {"mean": mean, "invstd": inv, "out": out.to(y.dtype)}


# ------------------------------------------------------------------------------------------------- honest stand-ins pass
@pytest.mark.parametrize("kind", sn.KINDS)
@pytest.mark.parametrize("id_,dtype", [("gather-bn32-registers-64x72k3s1", BF), ("gather-bn64-dma-64x64k3s2", HF), ("ring-bk64-64x64-depth4-k1", HF),
                                       ("patch-8", BF), ("generic-cin12", BF), ("fp32", F32)])
def test_honest_convolutions_pass(id_, dtype, kind):
    case = by_id(id_)
    k, s = case["k"], case["s"]
    p, d = nc.dense_plan(case)
    inp = nc.dense_inputs(case, dtype)
    sn.require_nonzero(id_, w=inp["w"], x=inp["x"], dy=inp["dy"])
    x, w, dy = inp["x"], inp["w"], inp["dy"]
    fam = "cpu_conv"
    sn.assert_propagates(conv_fwd(x, w, k, s), conv_fwd(sn.poison(x, p["x"], kind), w, k, s), d["fwd"], kind, id_, fam)
    sn.assert_propagates(conv_fwd(x, w, k, s), conv_fwd(x, sn.poison(w, p["w"], kind), k, s), d["fwd_w"], kind, id_, fam)
    res = inp["res"].float()
    fused = lambda xx, rr: (F.silu(conv_fwd(xx, w, k, s).float() + inp["bias"].view(1, -1, 1, 1)) + rr.float()).to(dtype)
    sn.assert_propagates(fused(x, res), fused(sn.poison(x, p["x"], kind), sn.poison(inp["res"], p["res"], kind)), d["fused"], kind, id_, fam)
    dx = lambda g, b, a: (conv_dgrad(g, w, x.shape, k, s).float() + b.float() + a.float()).to(dtype)
    sn.assert_propagates(dx(dy, inp["base"], inp["acc2"]),
                         dx(sn.poison(dy, p["dy"], kind), sn.poison(inp["base"], p["base"], kind), sn.poison(inp["acc2"], p["acc2"], kind)),
                         d["dgrad_acc2"], kind, id_, fam)
    dw0 = conv_wgrad(x, dy, w.shape, k, s)
    sn.assert_propagates(dw0, conv_wgrad(sn.poison(x, p["x_w"], kind), dy, w.shape, k, s), d["wgrad_x"], kind, id_, fam)
    sn.assert_propagates(dw0, conv_wgrad(x, sn.poison(dy, p["dy_w"], kind), w.shape, k, s), d["wgrad_dy"], kind, id_, fam)


@pytest.mark.parametrize("kind", sn.KINDS)
@pytest.mark.parametrize("c,h,w", [(16, 1, 6), (16, 5, 1), (8, 5, 6), (12, 5, 6)])
def test_honest_depthwise_passes(c, h, w, kind):
    p, d = nc.dw_plan(c, h, w)
    inp = nc.dw_inputs(c, h, w, HF)
    w4 = inp["w9"].view(c, 1, 3, 3)
    x, dy = inp["x"], inp["dy"]
    bad = sn.poison(x, p["x"], kind)
    sn.assert_propagates(conv_fwd(x, w4, 3, 1, c), conv_fwd(bad, w4, 3, 1, c), d["fwd"], kind, "dw fwd", "cpu_dw")
    sn.assert_propagates(conv_dgrad(dy, w4, x.shape, 3, 1, c), conv_dgrad(sn.poison(dy, p["dy"], kind), w4, x.shape, 3, 1, c), d["dgrad"], kind,
                         "dw dgrad", "cpu_dw")
    dw0 = conv_wgrad(x, dy, w4.shape, 3, 1, c)
    taps = d["taps"]
    sn.assert_propagates(dw0[:, :, taps], conv_wgrad(bad, dy, w4.shape, 3, 1, c)[:, :, taps], d["wgrad_x"], kind, "dw wgrad x", "cpu_dw")
    sn.assert_propagates(dw0[:, :, taps], conv_wgrad(x, sn.poison(dy, p["dy"], kind), w4.shape, 3, 1, c)[:, :, taps], d["wgrad_dy"], kind,
                         "dw wgrad dy", "cpu_dw")
    st = lambda xx: torch.stack([conv_fwd(xx, w4, 3, 1, c).float().sum((0, 2, 3)), (conv_fwd(xx, w4, 3, 1, c).float() ** 2).sum((0, 2, 3))])
    sn.assert_propagates(st(x), st(bad), d["stats"], kind, "dw statistics", "cpu_dw")


def _qkv(heads, dk, dh, t, dtype=F32, n=nc.ATTN_N):
    return sn.fix_zeros(sa.make_qkv(n, heads, dk, dh, t, "plain", 60 + t, dtype))


def _row_pos(which, row, heads, dk, dh, hw):
    prob, tok, comp = row if len(row) == 3 else tuple(row) + (3,)
    return (prob // heads, nc.attn_channel(which, prob % heads, comp, heads, dk, dh), tok // hw[1], tok % hw[1])


def _kw(which, row):
    return {"v_elems": [row]} if which == "v" else {f"{which}_rows": [row]}


def _elem(mask, n, hw):
    return sa.merge(mask.double(), n, *hw) > 0


@pytest.mark.parametrize("which,kinds", [("q", sn.KINDS), ("k", ("nan",)), ("v", sn.KINDS)])
def test_honest_attention_passes(which, kinds):
    heads, dk, dh, t = 2, 32, 64, 36
    hw, b = sa.hw(t), nc.ATTN_N * heads
    qkv = _qkv(heads, dk, dh, t)
    rows = nc.attn_plan(heads, t)
    dep = sn.attention_dep(b, t, dk, dh, **_kw(which, rows[which]))
    for kind in kinds:
        bad = sn.poison(qkv, [_row_pos(which, rows[which], heads, dk, dh, hw)], kind)
        sn.assert_propagates(attention(qkv, heads, dk, dh), attention(bad, heads, dk, dh), _elem(dep["o"], nc.ATTN_N, hw), kind,
                             f"attention {which}", "cpu_attn")


def test_a_key_at_minus_infinity_is_a_masked_key_so_k_gets_nan_only():
    """why the GPU module poisons k with NaN alone: q . k = -inf for the rows whose q component is positive; those rows'
    probability of that key is exactly 0 and they stay finite -- legitimately"""
    heads, dk, dh, t = 2, 32, 64, 36
    hw, b = sa.hw(t), nc.ATTN_N * heads
    qkv = _qkv(heads, dk, dh, t)
    rows = nc.attn_plan(heads, t)
    bad = qkv.clone()
    bad[_row_pos("k", rows["k"], heads, dk, dh, hw)] = float("-inf")
    dep = _elem(sn.attention_dep(b, t, dk, dh, k_rows=[rows["k"]])["o"], nc.ATTN_N, hw)
    fams, e = sn.failing(lambda: sn.assert_propagates(attention(qkv, heads, dk, dh), attention(bad, heads, dk, dh), dep, "inf", "k = -inf", "cpu_attn"))
    assert fams == ["cpu_attn"] and "swallowed" in str(e) and 0 < e.count < int(dep.sum())


@pytest.mark.parametrize("kind", sn.KINDS)
@pytest.mark.parametrize("shape", nc.BN[:3], ids=str)
def test_honest_batchnorm_passes(shape, kind):
    n, c, h, w, _, _ = shape
    pos, chan, full = nc.bn_plan(n, c, h, w)
    y = nc.rnd((n, c, h, w), 5, dtype=BF)
    gamma, beta = 1 + 0.1 * nc.rnd((c,), 6, dtype=F32), 0.1 * nc.rnd((c,), 7, dtype=F32)
    r0, r1 = batchnorm(y, gamma, beta), batchnorm(sn.poison(y, pos, kind), gamma, beta)
    for key in r0:
        sn.assert_propagates(r0[key], r1[key], full if r0[key].dim() == 4 else chan, kind, f"bn {key}", "cpu_bn")


# ------------------------------------------------------------------------------------------------- leaky stand-ins are rejected
def test_padding_by_clamped_pixel_times_mask_is_rejected():
    """a NaN in pixel 0 of the batch reaches every output of the first row (their upper taps clamp to it); one in the first
    row of image 1 reaches the last row of image 0: rejected outside dep, on border pixels of exactly those images"""
    case = by_id("gather-bn32-registers-64x72k3s1")
    h, wd = case["h"], case["w"]
    p, d = nc.dense_plan(case)
    inp = nc.dense_inputs(case, BF)
    x, w = inp["x"], inp["w"]
    got, want = conv_clamped_mask(x, w, 3, 1).float(), conv_fwd(x, w, 3, 1).float()
    assert float((got - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max())         # finite data: the stand-in IS the convolution
    bad = sn.poison(x, p["x"], "nan")
    fams, e = sn.failing(lambda: sn.assert_propagates(conv_clamped_mask(x, w, 3, 1), conv_clamped_mask(bad, w, 3, 1), d["fwd"], "nan", "clamped x mask", "cpu_conv"))
    assert fams == ["cpu_conv"] and "leaked" in str(e)
    leak = torch.isnan(conv_clamped_mask(bad, w, 3, 1).float()) & ~d["fwd"]
    hit = {(n_, h_, w_) for n_, _, h_, w_ in leak.nonzero().tolist()}
    assert {(0, 0, w_) for w_ in range(2, wd)} <= hit, "pixel 0 of the batch did not reach the first row"
    assert any(n_ == 0 and h_ == h - 1 for n_, h_, _ in hit), "the first row of image 1 did not reach the last row of image 0"
    assert all(h_ in (0, h - 1) or w_ in (0, wd - 1) for _, h_, w_ in hit), "only border pixels have padding taps"
    assert e.count == int(leak.sum()) and 0 in e.hist["image"]
    sn.assert_propagates(conv_fwd(x, w, 3, 1), conv_fwd(bad, w, 3, 1), d["fwd"], "nan", "honest", "cpu_conv")          # the honest convolution passes


def test_reading_past_cin_against_zero_weights_is_rejected_by_the_surroundings_run():
    """finite neighbours (the 3.0 / 5.0 / 7.0 / SENTINEL guards of the other modules) cannot see it: x 0 cancels them"""
    case = by_id("gather-bn32-registers-64x72k3s1")
    inp = nc.dense_inputs(case, BF)
    x, w, cin = inp["x"], inp["w"], case["cin"]

    def run(hostile, fn):
        buf = torch.full((N, cin + 32, case["h"], case["w"]), NAN if hostile else 3.0, dtype=BF)
        buf[:, 16:16 + cin] = x
        return {"y": fn(buf)}, [(buf, 16, 16 + cin)]
    leaky = lambda buf: conv_reads_past_cin(buf, 16, cin, w, 3, 1)
    honest = lambda buf: conv_fwd(buf[:, 16:16 + cin], w, 3, 1)
    assert torch.equal(leaky(run(False, lambda b: b)[0]["y"]), conv_fwd(x, w, 3, 1))          # finite neighbours: invisible
    fams, e = sn.failing(lambda: sn.assert_unmoved_by_surroundings(lambda hostile: run(hostile, leaky), "reads past Cin", "cpu_conv"))
    assert fams == ["cpu_conv"] and e.count == N * case["cout"] * case["h"] * case["w"]      # every product sum holds 0 x NaN
    sn.assert_unmoved_by_surroundings(lambda hostile: run(hostile, honest), "honest", "cpu_conv")


def test_a_guard_channel_that_was_overwritten_is_reported():
    def run(hostile):
        buf = torch.full((1, 12, 2, 2), NAN if hostile else 3.0)
        buf[:, 4:8] = 1.0
        buf[:, 8] = 2.0                                   # the launch wrote one channel beside its slice
        return {"y": buf[:, 4:8].clone()}, [(buf, 4, 8)]
    fams, e = sn.failing(lambda: sn.assert_unmoved_by_surroundings(run, "writes beside its slice", "cpu_conv"))
    assert fams == ["cpu_conv"] and e.count == 4 and "no longer hold NaN" in str(e)


def test_masked_key_columns_multiplied_by_zero_are_rejected():
    """36 tokens in 64-column blocks: columns 36 .. 63 of image 0 are the clamped rows of image 1.  A NaN in image 1's key or
    value row 0 must stay in image 1; the leaky kernel carries it into every row of image 0's same head"""
    heads, dk, dh, t = 2, 32, 64, 36
    hw, b = sa.hw(t), nc.ATTN_N * heads
    qkv = _qkv(heads, dk, dh, t)
    assert float((attention(qkv, heads, dk, dh, leaky=True) - attention(qkv, heads, dk, dh)).abs().max()) < 1e-5      # finite data: the same
    row = (heads, 0, 3)                                     # image 1, head 0, token 0, component 3
    dep = _elem(sn.attention_dep(b, t, dk, dh, v_elems=[row])["o"], nc.ATTN_N, hw)
    bad = sn.poison(qkv, [_row_pos("v", row, heads, dk, dh, hw)], "nan")
    fams, e = sn.failing(lambda: sn.assert_propagates(attention(qkv, heads, dk, dh, True), attention(bad, heads, dk, dh, True), dep, "nan", "p = 0 by multiplication", "cpu_attn"))
    assert fams == ["cpu_attn"] and "leaked" in str(e)
    assert set(e.hist["image"]) == {0} and e.count == t                  # image 0, head 0, component 3 of every row
    sn.assert_propagates(attention(qkv, heads, dk, dh), attention(bad, heads, dk, dh), dep, "nan", "honest", "cpu_attn")


@pytest.mark.parametrize("kind", sn.KINDS)
def test_a_swallowed_nan_is_rejected(kind):
    case = by_id("gather-bn32-registers-64x72k3s1")
    p, d = nc.dense_plan(case)
    inp = nc.dense_inputs(case, BF)
    x, w = inp["x"], inp["w"]
    fams, e = sn.failing(lambda: sn.assert_propagates(conv_swallows(x, w, 3, 1), conv_swallows(sn.poison(x, p["x"], kind), w, 3, 1), d["fwd"], kind,
                                                      "nan_to_num", "cpu_conv"))
    assert fams == ["cpu_conv"] and "swallowed" in str(e) and e.count == int(d["fwd"].sum())


def test_batchnorm_statistics_leaking_into_the_next_channel_are_rejected():
    n, c, h, w, _, _ = nc.BN[1]
    pos, chan, full = nc.bn_plan(n, c, h, w)
    y = nc.rnd((n, c, h, w), 5, dtype=BF)
    gamma, beta = 1 + 0.1 * nc.rnd((c,), 6, dtype=F32), 0.1 * nc.rnd((c,), 7, dtype=F32)
    r0, r1 = batchnorm(y, gamma, beta, leaky=True), batchnorm(sn.poison(y, pos, "nan"), gamma, beta, leaky=True)
    assert torch.equal(r0["out"], batchnorm(y, gamma, beta)["out"])
    fams, e = sn.failing(lambda: sn.assert_propagates(r0["mean"], r1["mean"], chan, "nan", "bn mean", "cpu_bn"))
    assert fams == ["cpu_bn"] and e.count == 1 and e.worst[0][0] == (pos[0][1] - 1,)          # the channel before the poisoned one
    fams, e = sn.failing(lambda: sn.assert_propagates(r0["out"], r1["out"], full, "nan", "bn out", "cpu_bn"))
    assert fams == ["cpu_bn"] and e.count == n * h * w and set(e.hist["channel_block"]) == {(pos[0][1] - 1) // 16}


# ------------------------------------------------------------------------------------------------- the exemption
def test_exempt_families_are_held_to_their_bound_and_to_nothing_weaker():
    case = nc.wgrad_case(72, 88, 3, 1)
    p, d = nc.dense_plan(case)
    inp = nc.dense_inputs(case, BF)
    x, dy = inp["x"], inp["dy"]
    ref, mass = sc.wgrad_ref(x, dy, (88, 72, 3, 3), 3, 1)
    bound = lambda merged: sc.assert_close(merged, ref, mass, F32, "wgrad", "wgrad_atomics")
    clean = conv_wgrad(x, dy, (88, 72, 3, 3), 3, 1)
    bad = conv_wgrad(sn.poison(x, p["x_w"], "nan"), dy, (88, 72, 3, 3), 3, 1)
    noisy = torch.where(torch.isnan(bad), bad, bad * (1 + 2.0 ** -23))            # another summation order: other bits, inside the bound
    sn.assert_propagates(clean, noisy, d["wgrad_x"], "nan", "atomics", "wgrad_atomics", bound)
    with pytest.raises(sn.Refused):                                              # bit equality is not optional elsewhere
        sn.assert_propagates(clean, noisy, d["wgrad_x"], "nan", "product path", "wgrad", bound)
    with pytest.raises(sn.Refused):
        sn.assert_propagates(clean, noisy, d["wgrad_x"], "nan", "atomics", "wgrad_atomics")
    fams, e = sn.failing(lambda: sn.assert_propagates(clean, noisy, d["wgrad_x"], "nan", "product path", "wgrad"))
    assert fams == ["wgrad"]
    wrong = bad.clone()
    wrong[0, 5, 1, 1] += 1e-2 * float(ref.abs().max())                            # outside dep, outside the bound
    assert not bool(d["wgrad_x"][0, 5, 1, 1])
    fams, e = sn.failing(lambda: sn.assert_propagates(clean, wrong, d["wgrad_x"], "nan", "atomics", "wgrad_atomics", bound))
    assert e is not None and e.count == 1
    leak = bad.clone()
    leak[0, 5, 1, 1] = NAN                                                        # a NaN outside dep under the exemption
    fams, e = sn.failing(lambda: sn.assert_propagates(clean, leak, d["wgrad_x"], "nan", "atomics", "wgrad_atomics", bound))
    assert e is not None
    assert all("atomic" in why for why in sn.EXEMPT.values())


# ------------------------------------------------------------------------------------------------- the refusals
def test_helper_refuses_vacuous_cases():
    a = torch.ones(2, 4, 3, 3)
    with pytest.raises(sn.Refused, match="empty"):
        sn.assert_propagates(a, a, torch.zeros(2, 4, 3, 3, dtype=torch.bool), "nan", "empty", "cpu_conv")
    more = torch.zeros(2, 4, 3, 3, dtype=torch.bool)
    more[:, :3] = True
    with pytest.raises(sn.Refused, match="more than half"):
        sn.assert_propagates(a, a, more, "nan", "most", "cpu_conv")
    half = torch.zeros(2, 4, 3, 3, dtype=torch.bool)
    half[:, :2] = True
    sn.assert_propagates(a, torch.where(half, torch.full_like(a, NAN), a), half, "nan", "exactly half", "cpu_conv")
    with pytest.raises(sn.Refused, match="exact zero"):
        sn.require_nonzero("w", w=torch.tensor([1.0, 0.0]))
    with pytest.raises(sn.Refused, match="not finite"):
        sn.assert_propagates(torch.full_like(a, NAN), a, half, "nan", "dirty clean run", "cpu_conv")
    assert not bool((sn.fix_zeros(torch.tensor([0.0, 1.0, -0.0])) == 0).any())


def test_every_gpu_case_lies_inside_the_refusal_conditions():
    seen = 0
    for name, deps, operands in nc.all_dep_masks():
        for key, dep in deps.items():
            sn.check_dep(dep, f"{name} {key}")
            seen += 1
        sn.require_nonzero(name, **operands)
    assert seen > 1000
    for route, dtype, heads, dk, dh, t in nc.ATTN + nc.ATTN_NOGRAD:
        sn.require_nonzero(f"attention T={t}", qkv=sn.fix_zeros(sa.make_qkv(nc.ATTN_N, heads, dk, dh, t, "plain", 60 + t, dtype)))


def test_every_dense_case_reaches_the_variant_it_names():
    """the plan query and the tune calls touch nothing in the HIP runtime: the cross-compiled library answers here"""
    from src.hipops import lib
    code = {BF: lib.BF16, HF: lib.F16, F32: lib.F32}
    try:
        for case in nc.DENSE:
            cin, cout, h, w, k, s = (case[key] for key in ("cin", "cout", "h", "w", "k", "s"))
            oh, ow = nc.out_hw(h, w, k, s)
            lib.call("yolo_conv_tune_set", *case["tune"])
            for dtype in case["dtypes"]:
                if case["plan"] is not None:
                    assert lib.query("yolo_conv2d_plan", N, h, w, cin, oh, ow, cout, k, s, 0, 0, code[dtype]) == case["plan"], case["id"]
                if case.get("dplan"):
                    assert all(lib.query("yolo_conv2d_plan", N, h, w, cin, oh, ow, cout, k, s, 1, c, code[dtype]) == case["dplan"] for c in range(4)), case["id"]
        assert {c["plan"] for c in nc.DENSE if c["plan"]} >= {1032, 1064, 1128, 3032, 3064, 3128, 3564, 3628, 2001, 2002, 2003, 2004,
                                                             4001, 4002, 4003, 4004, 4006, 4007}
        for to, ti, pf, cin, cout, k, s in nc.WGRAD:
            lib.call("yolo_wgrad_tune_set", to, ti, 0, 0)
            lib.call("yolo_wgrad_tune_pf", pf)
            plan = lib.query("yolo_conv2d_wgrad_plan", N, 7, 11, cin, *nc.out_hw(7, 11, k, s), cout, k, s, lib.BF16)
            assert plan // 10000000 == pf and plan // 1000000 % 10 == to and plan // 100000 % 10 == ti, (to, ti, pf, plan)
        for c, h, w, _, _ in nc.DW:
            for variant, want in ((1, 2), (2, 1)):
                lib.call("yolo_dw_tune_set", variant)
                assert lib.query("yolo_dw_plan", N, h, w, c, 0) == want and lib.query("yolo_dw_plan", N, h, w, c, 12) == want
    finally:
        lib.call("yolo_conv_tune_set", 0, -1, -1, -1, -1, 0, 0, 0)
        lib.call("yolo_wgrad_tune_set", 0, 0, 0, 0)
        lib.call("yolo_wgrad_tune_pf", 0)
        lib.call("yolo_dw_tune_set", 0)


# ------------------------------------------------------------------------------------------------- attention_dep
def test_attention_dep_is_what_the_float64_reference_shows():
    """every operand perturbed in one row (finite: +0.37 on one component) through strict_attention.forward / backward, the
    backward from the perturbed forward's own o and lse: the rows that move are exactly attention_dep()'s"""
    heads, dk, dh, t, n = 2, 8, 8, 12, 2
    b = n * heads
    g = torch.Generator().manual_seed(3)
    q, k, v, d_o, d_vp = (torch.randn(b, t, d, generator=g, dtype=torch.float64) for d in (dk, dk, dh, dh, dh))
    scale = dk ** -0.5

    def run(q, k, v, d_o, d_vp):
        f = sa.forward(q, k, v, scale, BF, "fused")
        r = sa.backward(q, k, v, d_o, d_vp, scale, BF, "fused", o=f["o"], lse=f["lse"])
        return {"o": f["o"], "lse": f["lse"], "dq": r["dq"], "dk": r["dk"], "dv": r["dv"]}
    base = run(q, k, v, d_o, d_vp)
    row = (1, 5, 2)
    for name, i in (("q_rows", 0), ("k_rows", 1), ("v_elems", 2), ("do_elems", 3), ("dvp_elems", 4)):
        args = [q, k, v, d_o, d_vp]
        args[i] = args[i].clone()
        args[i][row] += 0.37
        got = run(*args)
        moved = {key: (val != base[key]) for key, val in got.items()}
        moved["lse"] = moved["lse"][..., 0]
        dep = sn.attention_dep(b, t, dk, dh, **{name: [row[:2] if name.endswith("rows") else row]})
        for key in dep:
            assert torch.equal(moved[key], dep[key]), (name, key, int(moved[key].sum()), int(dep[key].sum()))


def test_the_weight_gradient_positions_make_whole_rows():
    """'NaN in one x channel means exactly dw[:, ci] for the taps that exist, in one dy channel exactly dw[co]': with the
    interior pixels of nonfinite_cases.positions() the indicator reference marks whole rows (every tap that exists at all, on
    one-row / one-column depthwise maps), so the case does not depend on how a kernel treats a tap that pairs the poisoned
    element with padding or with an output pixel past the map"""
    cases = nc.DENSE + [nc.wgrad_case(*c) for c in sorted({c[3:] for c in nc.WGRAD} | set(nc.WGRAD_ATOMICS))]
    for case in cases:
        d = nc.dense_plan(case)[1]
        by_co, by_ci = d["wgrad_dy"], d["wgrad_x"]
        assert torch.equal(by_co, by_co.flatten(1).any(1).view(-1, 1, 1, 1).expand_as(by_co)), case["id"]
        assert torch.equal(by_ci, by_ci.any(0).flatten(1).any(1).view(1, -1, 1, 1).expand_as(by_ci)), case["id"]
    d = nc.stem_plan()[1]
    assert torch.equal(d["wgrad_img"], d["wgrad_img"].any(0).flatten(1).any(1).view(1, -1, 1, 1).expand_as(d["wgrad_img"]))
    assert torch.equal(d["wgrad_dy"], d["wgrad_dy"].flatten(1).any(1).view(-1, 1, 1, 1).expand_as(d["wgrad_dy"]))
    for c, h, w, _, _ in nc.DW + [nc.DW_GENERIC]:
        d = nc.dw_plan(c, h, w)[1]
        for key in ("wgrad_x", "wgrad_dy"):
            assert torch.equal(d[key], d[key].flatten(1).any(1).view(-1, 1, 1).expand_as(d[key])), (c, h, w, key)
        assert int(d["taps"].sum()) == (3 if h > 1 else 1) * (3 if w > 1 else 1)
