"""CPU tests of tests/strict_attention.py: what proves, without a GPU, that the derived per-element attention bound passes
the kernels' arithmetic and fails arithmetic that is subtly wrong.

The stand-ins are fp32 torch code with the kernels' rounding points, each in two summation orders (one fp32 matmul; partial
sums per 8 / 16 channels or 32 tokens added one after another, last chunk first):
  fused   s = (q.k) scale, m = max, p = exp(s - m), l = sum p, o = round(sum round(p) v / l), lse = m + log l;
          backward from the STORED o and lse: P = exp(s - lse), dS = round(P (dP - D) scale), dQ = round(dS k),
          dK = round(dS^T q), dV = round(round(P)^T dO + d_vp)
  long    the same forward over 256-key blocks with the running maximum, sum and accumulator rescaled per block
  gemm    P = round(exp(s - m) / l) materialised, o = round(P v); backward from the stored P: D = sum P dP,
          dS = round(P (dP - D)), dQ = round(scale dS k), dK = round(scale dS^T q), dV = round(P^T dO + d_vp)
  fp32    fp32 inputs, nothing rounded in between
They must pass with ZERO elements out at every length and input class of the GPU tests, in bf16 and f16; every mutant of
MUTANTS must fail.  The guard 'nowhere wider than the limit check() applied before' runs in every comparison.

Recorded maxima of the stand-ins, largest share of the noise budget used ((|got - ref| - 1/2 ulp) / noise, limit 1):
    fused o 0.86, lse 0.17, dq 0.93, dk 0.90, dv 0.97      long o 0.84
    gemm  o 0.95, stashed P 0.24, dq 0.89, dk 0.86, dv 0.001 (its P is the stash itself: B_ij is all slack)
    fp32  o 0.07, lse 0.11, dq 0.15, dk 0.18, dv 0.26
The 16-bit maxima sit where one probability carries a row (sharpened and short cases): there the limit is little more than
the true worst case of the one rounding of that p, 1/2 ulp, and the stand-in comes close to it.
(the module prints the table when it finishes: run with -s)."""
import pytest
import torch

import strict_attention as sa
import strict_compare as sc

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
# the lengths of tests/test_gpu_kernels.py
FUSED_T = [1, 15, 16, 17, 128, 129, 224, 225, 256, 257, 400, 416, 417, 441, 448]
LONG_T = [449, 512, 513, 768, 1073, 1600]
GEMM_CASES = [(16, 32, t) for t in (143, 417, 448, 449, 529)] + [(32, 64, 449), (32, 64, 529)]
FP32_T = [127, 128, 129, 400]


@pytest.fixture(autouse=True, scope="module")
def _threads_and_report():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    yield
    print("\n" + sc.report())


def rT(x, dtype):
    return x if dtype == F32 else x.to(dtype).float()


def mm(a, b, order, chunk):
    """a @ b in fp32: order 0 one matmul, order 1 partial sums per `chunk` of the inner dimension, last chunk first"""
    if order == 0:
        return a @ b
    acc = None
    for c0 in reversed(range(0, a.shape[-1], chunk)):
        part = a[..., c0:c0 + chunk] @ b[..., c0:c0 + chunk, :]
        acc = part if acc is None else acc + part
    return acc


def inputs(n, heads, dk, dh, t, cls, dtype, seed=0):
    """-> qkv, d_o, d_vp as float32 (B, T, d) pieces holding `dtype` values (fp32: full-precision Gaussians)"""
    qkv = sa.make_qkv(n, heads, dk, dh, t, cls, 100 + seed, dtype)
    g = torch.Generator().manual_seed(200 + seed)
    d_o = torch.randn(n, heads * dh, *sa.hw(t), generator=g).to(dtype)
    d_vp = torch.randn(n, heads * dh, *sa.hw(t), generator=g).to(dtype)
    q, k, v = (x.float() for x in sa.split_qkv(qkv, heads, dk, dh))
    return q, k, v, sa.split(d_o, heads).float(), sa.split(d_vp, heads).float()


# ------------------------------------------------------------------------------------------ the stand-ins (fp32)
def scores(q, k, scale, order, mut):
    s = mm(q, k.mT, order, 8) * scale
    return s[..., :-16] if mut == "drop_last_16_keys" else s


def fwd_fused(q, k, v, scale, dtype, order=0, mut=None):
    s = scores(q, k, scale, order, mut)
    if mut == "drop_last_16_keys":
        v = v[:, :-16]
    if mut == "spurious_padded_key":                               # one key past T left unmasked: score 0, v = 0
        s = torch.cat([s, torch.zeros_like(s[..., :1])], -1)
        v = torch.cat([v, torch.zeros_like(v[:, :1])], 1)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    return rT(mm(rT(p, dtype), v, order, 32) / l, dtype), m + torch.log(l)


def fwd_long(q, k, v, scale, dtype, order=0, mut=None, block=256):
    s = scores(q, k, scale, order, mut)
    if mut == "drop_last_16_keys":
        v = v[:, :-16]
    if mut == "spurious_padded_key":
        s = torch.cat([s, torch.zeros_like(s[..., :1])], -1)
        v = torch.cat([v, torch.zeros_like(v[:, :1])], 1)
    m = torch.full_like(s[..., :1], float("-inf"))
    l = torch.zeros_like(m)
    acc = torch.zeros(*s.shape[:2], v.shape[-1])
    for k0 in range(0, s.shape[-1], block):
        sb = s[..., k0:k0 + block]
        mn = torch.maximum(m, sb.amax(-1, keepdim=True))
        corr = torch.exp(m - mn)
        if mut == "no_rescale" and k0 > 0:
            corr = torch.ones_like(corr)
        p = torch.exp(sb - mn)
        l = l * corr + p.sum(-1, keepdim=True)
        acc = acc * corr + mm(rT(p, dtype), v[:, k0:k0 + block], order, 32)
        m = mn
    return rT(acc / l, dtype), m + torch.log(l)


def fwd_gemm(q, k, v, scale, dtype, order=0, mut=None):
    s = scores(q, k, scale, order, mut)
    if mut == "drop_last_16_keys":
        v = v[:, :-16]
    if mut == "spurious_padded_key":
        s = torch.cat([s, torch.zeros_like(s[..., :1])], -1)
        v = torch.cat([v, torch.zeros_like(v[:, :1])], 1)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    p = rT(p * (1.0 / p.sum(-1, keepdim=True)), dtype)
    o = rT(mm(p, v, order, 32), dtype)
    if mut == "drop_last_16_keys":
        p = torch.cat([p, torch.zeros_like(p[..., :16])], -1)
    return o, p[..., :q.shape[1]]


def bwd(route, q, k, v, d_o, d_vp, scale, dtype, order=0, mut=None, o=None, lse=None, p=None, heads=1):
    """fused / fp32: from the stored o, lse; gemm: from the stored p"""
    s = mm(q, k.mT, order, 8) * scale
    dp = mm(d_o, v.mT, order, 16)
    if route == "gemm":
        d = (p * dp).sum(-1, keepdim=True)
    else:
        if mut == "lse_of_neighbouring_head":
            lse = lse.reshape(-1, heads, *lse.shape[1:]).roll(1, 1).reshape(lse.shape)
        p = torch.exp(s - lse)
        d = (d_o * o).sum(-1, keepdim=True)
    if mut == "D_zero_last_query_tile":
        d = d.clone()
        d[:, -16:] = 0
    ds = rT(p * (dp - d), dtype) if route == "gemm" else rT(p * (dp - d) * scale, dtype)
    post = scale if route == "gemm" else 1.0
    dq = rT(mm(ds, k, order, 32) * post, dtype)
    pk, dsk, qk, dok = rT(p, dtype), ds, q, d_o
    if mut == "last_query_tile_missing_from_dkv":
        pk, dsk, qk, dok = pk[:, :-16], dsk[:, :-16], qk[:, :-16], dok[:, :-16]
    dk = rT(mm(dsk.mT, qk, order, 32) * post, dtype)
    dv = mm(pk.mT, dok, order, 32)
    if d_vp is not None and mut != "d_vp_not_added":
        dv = dv + d_vp
    return dq, dk, rT(dv, dtype)


FWD = {"fused": fwd_fused, "long": fwd_long, "gemm": fwd_gemm, "fp32": fwd_fused}
MUTANTS = ["drop_last_16_keys", "spurious_padded_key", "no_rescale", "D_zero_last_query_tile", "last_query_tile_missing_from_dkv",
           "d_vp_not_added", "lse_of_neighbouring_head", "wrong_image"]


def run(route, n, heads, dk, dh, t, cls, dtype, order=0, mut=None, with_vp=True, guard=True):
    """one stand-in run through the comparator exactly as the GPU tests go: forward, stash, backward from what was stored"""
    scale = dk ** -0.5
    q, k, v, d_o, d_vp = inputs(n, heads, dk, dh, t, cls, dtype)
    d64 = [x.double() for x in (q, k, v, d_o, d_vp)]
    what = f"{route} T={t} {cls} order {order}"
    o, stash = FWD[route](q, k, v, scale, dtype, order, mut)
    if mut == "wrong_image":
        o = o.reshape(n, heads, *o.shape[1:]).roll(1, 0).reshape(o.shape)
    sa.check_forward(route, *d64[:3], scale, dtype, o, got_lse=stash if route in ("fused", "fp32") else None,
                     got_p=stash if route == "gemm" else None, what=what, guard=guard)
    if route == "long":
        return
    vp = d_vp if with_vp else None
    kw = {"p": stash} if route == "gemm" else {"o": o, "lse": stash}
    dq, dk_, dv = bwd(route, q, k, v, d_o, vp, scale, dtype, order, mut, heads=heads, **kw)
    kw64 = {"p_stash": stash.double()} if route == "gemm" else {"o": o.double(), "lse": stash.double()}
    sa.check_backward(route, *d64[:4], d64[4] if with_vp else None, scale, dtype, dq, dk_, dv, what=what, guard=guard, **kw64)


# ------------------------------------------------------------------------------------------ the stand-ins pass
def heads_for(t):
    return 1 if t > 600 else 2


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
@pytest.mark.parametrize("t", FUSED_T)
def test_fused_stand_in_has_nothing_outside(t, dtype):
    for cls in sa.CLASSES:
        for order in (0, 1):
            run("fused", 1, 2, 32, 64, t, cls, dtype, order, with_vp=order == 0)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
@pytest.mark.parametrize("t", LONG_T)
def test_key_blocked_stand_in_has_nothing_outside(t, dtype):
    for cls in sa.CLASSES:
        for order in (0, 1):
            run("long", 1, heads_for(t), 32, 64, t, cls, dtype, order)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
@pytest.mark.parametrize("dk,dh,t", GEMM_CASES)
def test_gemm_stand_in_has_nothing_outside(dk, dh, t, dtype):
    for cls in sa.CLASSES:
        for order in (0, 1):
            run("gemm", 1, 2, dk, dh, t, cls, dtype, order, with_vp=order == 0)


@pytest.mark.parametrize("t", FP32_T)
def test_fp32_stand_in_has_nothing_outside(t):
    for cls in sa.CLASSES:
        for order in (0, 1):
            run("fp32", 1, 2, 32, 64, t, cls, F32, order, with_vp=order == 0)


# ------------------------------------------------------------------------------------------ the mutants fail
def fails(route, t, cls, dtype, mut, dk=32, dh=64):
    # the guard 'nowhere wider than before' is for sound outputs (1/2 ulp of a wild `got` is wide): off under a mutant
    try:
        run(route, 2, 2, dk, dh, t, cls, dtype, 0, mut, guard=mut is None)
    except sa.StrictMismatch:
        return True
    return False


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
@pytest.mark.parametrize("mut", [m for m in MUTANTS if m != "no_rescale"])
@pytest.mark.parametrize("route,dk,dh,t", [("fused", 32, 64, 143), ("fused", 32, 64, 400), ("gemm", 16, 32, 143), ("gemm", 32, 64, 449),
                                           ("long", 32, 64, 513), ("fp32", 32, 64, 129)])
def test_every_mutant_fails(route, dk, dh, t, mut, dtype):
    if route == "fp32":
        dtype = F32
    backward_only = mut in ("D_zero_last_query_tile", "last_query_tile_missing_from_dkv", "d_vp_not_added", "lse_of_neighbouring_head")
    if (route == "long" and backward_only) or (route == "gemm" and mut == "lse_of_neighbouring_head"):
        return                                                # no such step on this route
    # the spurious zero-score key is asserted where it is visible at all: on the all-negative scores
    classes = ("negative",) if mut == "spurious_padded_key" else sa.CLASSES
    for cls in classes:
        assert fails(route, t, cls, dtype, mut), (route, t, cls, mut)
    assert not fails(route, t, classes[0], dtype, None)       # and the same call without the mutant passes


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
@pytest.mark.parametrize("t", [513, 1073])
def test_skipped_online_softmax_rescale_fails(t, dtype):
    for cls in sa.CLASSES:
        assert fails("long", t, cls, dtype, "no_rescale"), (t, cls)


def test_spurious_padded_key_is_invisible_on_gaussian_scores():
    """why the all-negative class exists: on the plain inputs one unmasked zero-score key moves no element of o outside
    the limit (it changes the denominator by about exp(-max) / T); only the row log-sum-exp can notice"""
    q, k, v, _, _ = inputs(1, 2, 32, 64, 400, "plain", BF)
    o, _ = fwd_fused(q, k, v, 32 ** -0.5, BF, 0, "spurious_padded_key")
    f = sa.forward(q.double(), k.double(), v.double(), 32 ** -0.5, BF, "fused")
    sa.assert_within(o, f["o"], f["o_noise"], BF, "o with a spurious key, plain inputs", "attn_fused_o")


def test_failure_histograms_name_the_head_and_the_token_block():
    q, k, v, _, _ = inputs(2, 2, 32, 64, 143, "plain", BF)
    o, _ = fwd_fused(q, k, v, 32 ** -0.5, BF)
    o[3, 32:48, 16:32] += 0.5                                 # image 1, head 1, tokens 32..47, channels 16..31
    f = sa.forward(q.double(), k.double(), v.double(), 32 ** -0.5, BF, "fused")
    with pytest.raises(sa.StrictMismatch) as ei:
        sa.assert_within(o, f["o"], f["o_noise"], BF, "o", "attn_fused_o")
    h = ei.value.hist
    assert set(h["image"]) == {3} and set(h["channel_block"]) == {1} and set(h["pixel_block"]) == {3 * 9 + 2}, h
