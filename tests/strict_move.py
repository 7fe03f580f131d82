"""Strict per-element comparator for the memory-bound kernels: the 5x5 max pool, the nearest x2 upsample, the channel-slice
copy / accumulate, the gradient fan-in (add_n), the layout transposes (csrc/elementwise.hip), the gradient buckets' pack and
unpack (csrc/multi_copy.hip) and the batched weight pack (csrc/pack_batched.hip).  float64 references and derived limits on
top of strict_compare.py (its ulp(), assert_close, StrictMismatch, OBSERVED / report()).  Shared by
tests/test_strict_move_cpu.py (the proof of the comparator, no GPU) and tests/test_gpu_move.py (the kernels).

Exact class (assert_exact): bit equality after mapping every NaN to one value.  The pool forward (value and argmax), the
upsample forward, copy_channels without accumulate, the transposes, bucket_copy and the weight pack only move values; with
a dtype change the stored value is the round-to-nearest-even of the fp32 value (what .to(dtype) gives on the CPU), with
`scale` the fp32 product, correctly rounded, then that one rounding.  A mismatch reports the count, the first 64 elements and
histograms by image, by 16-pixel block of the flattened N*H*W index and by 16-channel block.
    pool_ref: a 25-tap scan in float64, taps in (kh, kw) order, out-of-image taps skipped, update on "greater, or NaN, or
    no tap taken yet"; value and kh * 5 + kw.  Pinned to F.max_pool2d(return_indices=True) by the CPU module.

Sum class (assert_sum).  An output element is a sum of K terms t_1 .. t_K, each exact in fp32 (a value of T), added in fp32
in some order and rounded once to T.  With u = 2^-24, M = sum |t_i| and gamma_n = n u / (1 - n u), ANY order of the K - 1
fp32 additions gives |s~ - s| <= gamma_{K-1} M (Higham, Accuracy and Stability of Numerical Algorithms, (4.4)), and the one
rounding adds at most half a spacing of T at the stored magnitude:

    |got - ref| <= 1/2 ulp_T(max(|ref|, |got|)) + gamma_{K-1} M

No constant is fitted.  K = 1 leaves the half spacing alone and is moreover asserted as equality with the reference (a
single term IS a value of T); K = 0 is an exact zero.  A non-finite reference element (NaN, +-inf terms) must be met by the
same non-finite value.  strict_compare.assert_close carries the limit with c = 1 and mass = gamma_{K-1} M / 2^-24, so the
figure it records per family is the share of gamma_{K-1} M used; the former check() limit (2 or 4 ulps of the tensor's
LARGEST element) goes in as old_abs: the new limit is asserted to be nowhere wider.
    add_n                       K = 2, 3, 4                                       family move_add
    copy_channels accumulate    K = 2 (source + destination)                      family move_copy
    upsample backward           K = 4, or 5 with acc_into                         family move_up
    pool backward               K = the windows whose argmax is this pixel, routed by the REFERENCE idx (which the
                                forward check has shown equal to the device's), + 1 with acc_into   family move_pool

Chain (move_chain): SPPF's backward as the model runs it.  x -> y1 = P(x) -> y2 = P(y1) -> y3 = P(y2), concat gradient
(g0, g1, g2, g3); three launches, each accumulating into the concat gradient's slice and rounding once:
    v2 = g2 + R3(g3),   v1 = g1 + R2(v2),   v0 = g0 + R1(v1)           R_k: pool k's routing (scatter by its argmax)
Launch k reads the STORED v~_{k+1} = v_{k+1} + e_{k+1}, |e_{k+1}| <= E_{k+1}, so its exact sum differs from v_k by
R_k(e_{k+1}), at most R_k(E_{k+1}) because routing is linear with coefficients 0 / 1; its fp32 summation adds
gamma_{K-1} M_k on the mass of what it read, M_k <= |g_k| + R_k(|v_{k+1}| + E_{k+1}), and its rounding half a spacing of T at
the stored magnitude, at most 1/2 ulp_T(|v_k| + n_k):
    n_k = gamma_{K_k - 1} M_k + R_k(E_{k+1}),     E_k = 1/2 ulp_T(|v_k| + n_k) + n_k,     E_4 = 0 (g3 is given)
The last stage is compared through assert_close with n_0 as the noise (it grants 1/2 ulp_T(max(|ref|, |got|)) itself).

Guard: a tensor that is a channel slice is compared as the WHOLE underlying buffer; channels outside the slice must still
hold SENTINEL bit for bit (family `guard`).  Repeatability: no kernel here uses atomics; the GPU module runs every case
twice and asserts bit-identical results.

Recorded maxima, share of gamma_{K-1} M used (limit 1), MI355X, tests/test_gpu_move.py: see OBSERVED_GPU below.
CPU stand-ins: tests/test_strict_move_cpu.py, STAND_IN_MAXIMA."""
import torch

import strict_compare as sc
from strict_compare import U24, StrictMismatch, ulp  # noqa: F401  (re-exported for the tests)

F32, BF, HF = torch.float32, torch.bfloat16, torch.float16
FAMILIES = ("move_pool", "move_up", "move_copy", "move_add", "move_chain")
for _f in FAMILIES:
    sc.C[_f] = 1.0
    sc.BUDGET_FAMILIES.add(_f)
OLD_TOL = {F32: 1e-4, BF: 2.0 ** -6, HF: 2.0 ** -9}       # check() of tests/test_gpu_kernels.py
SENTINEL = -1234.0
GUARD = True                  # pass the former limit to assert_close (off only while a mutant is shown to fail)
EXACT = {}                    # family -> [comparisons, elements] of the exact class
OBSERVED_GPU = """MI355X, tests/test_gpu_move.py, 2026-10-19 (264 cases, every one twice; 23 M sum-class and 26 M exact-class elements):
move_pool 0.478, move_up 0.546, move_copy 0.000, move_add 0.476, move_chain 0.390 (of the propagated bound); idx, every exact-class
tensor and every guard bit-equal; no defect found; the module takes 2.7 s (2.1 s inside the tests)"""


def old_abs(ref, dtype, mult=2.0):
    fin = torch.where(torch.isfinite(ref), ref, torch.zeros_like(ref))
    return OLD_TOL[dtype] * mult * max(float(fin.abs().max()) if fin.numel() else 0.0, 1e-6)


def gamma(n):
    n = torch.as_tensor(n, dtype=torch.float64).clamp_min(0.0)
    return n * U24 / (1.0 - n * U24)


def _d(t):
    return t.detach().to("cpu", torch.float64)


def bits(t):
    """integer image of a tensor, every NaN mapped to one value"""
    t = t.detach().cpu()
    if not t.is_floating_point():
        return t.to(torch.int64)
    t = torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t).contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()]).to(torch.int64)


def _raise(what, family, bad, got, want, note):
    """StrictMismatch with the histograms of strict_compare.assert_close; bad: bool mask of got's (logical) shape"""
    idx = bad.nonzero()
    if got.dim() == 4:
        n, c, h, w = got.shape
        img, chan = idx[:, 0], idx[:, 1]
        pix = (idx[:, 0] * h + idx[:, 2]) * w + idx[:, 3]
    else:
        flat = bad.reshape(-1).nonzero()[:, 0]
        img, chan, pix = torch.zeros_like(flat), torch.zeros_like(flat), flat
    hist = {}
    for name, key in (("image", img), ("pixel_block", pix // 16), ("channel_block", chan // 16)):
        hist[name] = {int(k): int(v) for k, v in zip(*torch.unique(key, return_counts=True))}
    worst = [(tuple(i.tolist()), float(got[tuple(i.tolist())]), float(want[tuple(i.tolist())])) for i in idx[:64]]
    lines = [f"{what} [{family}]: {int(bad.sum())} of {got.numel()} elements {note}",
             f"  by image: {sc._top(hist['image'])}",
             f"  by 16-pixel block of N*H*W ({len(hist['pixel_block'])} blocks): {sc._top(hist['pixel_block'])}",
             f"  by 16-channel block: {sc._top(hist['channel_block'])}", "  first (index, got, want):"]
    lines += [f"    {ix}  {g:.9g}  {w_:.9g}" for ix, g, w_ in worst]
    e = StrictMismatch("\n".join(lines), int(bad.sum()), hist, worst)
    e.families = [family]
    raise e


def assert_exact(got, want, what, family="exact"):
    """bit equality (NaN == NaN) of two tensors of one shape and dtype"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    o = EXACT.setdefault(family, [0, 0])
    o[0], o[1] = o[0] + 1, o[1] + got.numel()
    bad = bits(got) != bits(want)
    if bool(bad.any()):
        _raise(what, family, bad, got, want, "differ bit for bit")


def assert_guard(buf, lo, hi, what):
    """channels outside [lo, hi) of the whole buffer (N, C_total, H, W) still hold the sentinel"""
    buf = buf.detach().cpu()
    want = torch.full_like(buf, SENTINEL)
    bad = bits(buf) != bits(want)
    bad[:, lo:hi] = False
    o = EXACT.setdefault("guard", [0, 0])
    o[0], o[1] = o[0] + 1, o[1] + buf.numel() - buf[:, lo:hi].numel()
    if bool(bad.any()):
        _raise(what, "guard", bad, buf, want, "beside the slice no longer hold the sentinel")


def assert_sum(got, ref, mass, k, dtype, what, family, mult=2.0, extra=None):
    """got (N, C, H, W) of `dtype` against the float64 sum `ref` of k terms of mass `mass` (tensors of got's shape);
    extra: noise added to gamma_{k-1} mass (the chain's propagated bound).  -> share of the noise used"""
    g = got.detach().cpu().to(torch.float64)
    ref, mass = ref.to(torch.float64), mass.to(torch.float64)
    k = torch.as_tensor(k).expand(ref.shape)
    try:
        nf = ~torch.isfinite(ref)
        same = torch.where(torch.isnan(ref), torch.isnan(g), g == ref)
        if bool((nf & ~same).any()):
            _raise(what, family, nf & ~same, g, ref, "do not carry the reference's NaN / infinity")
        zero = torch.zeros_like(ref)
        g, r, m = torch.where(nf, zero, g), torch.where(nf, zero, ref), torch.where(nf, zero, mass)
        one = (k <= 1) & ~nf & (extra is None)                # a single term: the value itself
        if bool((one & (g != r)).any()):
            _raise(what, family, one & (g != r), g, r, "with K <= 1 are not the one term itself")
        noise = gamma(k.to(torch.float64) - 1.0) * m
        if extra is not None:
            noise = torch.where(nf, zero, noise + extra)
        return sc.assert_close(g, r, noise / U24, dtype, what, family, c=1.0, old_abs=old_abs(r, dtype, mult) if GUARD else None)
    except StrictMismatch as e:
        e.families = [family]
        raise


def failing_families(fn):
    try:
        fn()
    except StrictMismatch as e:
        return list(e.families)
    return []


# ---------------------------------------------------------------------------------------------- references
def _tap_ranges(kh, kw, h, w):
    """window tap (kh, kw) of output pixel (oh, ow) is input pixel (oh + dh, ow + dw): -> dh, dw and the output ranges
    [h0, h1) x [w0, w1) for which that pixel is inside the image"""
    dh, dw = kh - 2, kw - 2
    return dh, dw, max(0, -dh), min(h, h - dh), max(0, -dw), min(w, w - dw)


def pool_ref(x, mut=None):
    """5x5 stride-1 pad-2 max pool -> (value float64, kh * 5 + kw uint8), both (N, C, H, W)"""
    x = _d(x)
    n, c, h, w = x.shape
    best = torch.full_like(x, float("-inf"))
    bi = torch.full(x.shape, -1, dtype=torch.int16)
    for kh in range(5):
        for kw in range(5):
            dh, dw, h0, h1, w0, w1 = _tap_ranges(kh, kw, h, w)
            if mut == "clip_right":                           # tap must satisfy ww < W - 1
                w1 = min(w1, w - 1 - dw)
            a = torch.zeros_like(x)
            valid = torch.zeros(x.shape, dtype=torch.bool)
            if h1 > h0 and w1 > w0:
                a[:, :, h0:h1, w0:w1] = x[:, :, h0 + dh:h1 + dh, w0 + dw:w1 + dw]
                valid[:, :, h0:h1, w0:w1] = True
            if mut == "pad_zero":
                valid[:] = True
            upd = (a >= best) if mut == "tie_last" else (a > best)
            if mut == "fmax":
                upd = upd | (torch.isnan(best) & ~torch.isnan(a))
            else:
                upd = upd | torch.isnan(a)
            upd = valid & (upd | (bi < 0))
            best = torch.where(upd, a, best)
            bi = torch.where(upd, torch.full_like(bi, kh * 5 + kw), bi)
    return best, bi.to(torch.uint8)


def aten_index(idx):
    """kh * 5 + kw -> the flat h * W + w index of F.max_pool2d(return_indices=True)"""
    n, c, h, w = idx.shape
    i = idx.to(torch.int64)
    hh = torch.arange(h).view(1, 1, h, 1) + torch.div(i, 5, rounding_mode="floor") - 2
    ww = torch.arange(w).view(1, 1, 1, w) + i % 5 - 2
    return hh * w + ww


def pool_bwd_ref(dout, idx, base=None, acc=torch.float64, order=None, mut=None):
    """gradient of the pool routed by idx (N, C, H, W; kh * 5 + kw) -> (sum in `acc`, mass float64, K int32); the taps are
    added in `order` (default 0 .. 24, the kernel's), the base (acc_into) last"""
    d = dout.detach().cpu().to(acc)
    n, c, h, w = d.shape
    s = torch.zeros(d.shape, dtype=acc)
    m = torch.zeros(d.shape, dtype=torch.float64)
    k = torch.zeros(d.shape, dtype=torch.int32)
    for t in (range(25) if order is None else order):
        kh, kw = divmod(t, 5)
        dh, dw, h0, h1, w0, w1 = _tap_ranges(kh, kw, h, w)
        if h1 <= h0 or w1 <= w0:
            continue
        hit = idx[:, :, h0:h1, w0:w1] == (kw * 5 + kh if mut == "swap" else t)
        dd = d[:, :, h0:h1, w0:w1]
        s[:, :, h0 + dh:h1 + dh, w0 + dw:w1 + dw] += torch.where(hit, dd, torch.zeros_like(dd))
        m[:, :, h0 + dh:h1 + dh, w0 + dw:w1 + dw] += torch.where(hit, dd.abs().double(), torch.zeros_like(dd, dtype=torch.float64))
        k[:, :, h0 + dh:h1 + dh, w0 + dw:w1 + dw] += hit.to(torch.int32)
    if base is not None:
        b = base.detach().cpu().to(acc)
        for _ in range({"no_base": 0, "base_twice": 2}.get(mut, 1)):
            s = s + b
        m, k = m + b.abs().double(), k + 1
    return s, m, k


def route(idx, t):
    """pool routing applied to a non-negative float64 tensor (a bound or a mass)"""
    return pool_bwd_ref(t, idx)[0]


def sum_ref(terms, acc=torch.float64, order=None):
    """-> (t[order[0]] + t[order[1]] + ... in `acc`, mass float64, K)"""
    ts = [t.detach().cpu() for t in terms]
    order = range(len(ts)) if order is None else order
    s, m = None, torch.zeros(ts[0].shape, dtype=torch.float64)
    for i in order:
        s = ts[i].to(acc) if s is None else s + ts[i].to(acc)
    for t in ts:
        m = m + t.abs().double()
    return s, m, len(ts)


def up_ref(x, mut=None):
    """nearest x2: out(oh, ow) = x(oh >> 1, ow >> 1); values unchanged (any dtype)"""
    x = x.detach().cpu()
    h, w = x.shape[2], x.shape[3]
    ih, iw = torch.arange(2 * h) >> 1, torch.arange(2 * w) >> 1
    if mut == "round_up":
        ih = ((torch.arange(2 * h) + 1) >> 1).clamp_(max=h - 1)
    return x[:, :, ih][:, :, :, iw]


def up_bwd_terms(dout, base=None, mut=None):
    """the terms of the upsample's backward in the kernel's order: (a, b) = (0,0), (0,1), (1,0), (1,1), then the base"""
    d = dout.detach().cpu()
    ts = [d[:, :, a::2, b::2] for a in range(2) for b in range(2)]
    if mut == "three":
        ts = ts[:3]
    return ts + ([base.detach().cpu()] if base is not None else [])


def cast_ref(src, dtype, scale=None):
    """what a cast (and bucket_copy's scale) stores: the fp32 value, times the fp32 scale correctly rounded, rounded once"""
    v = src.detach().cpu().float()
    if scale is not None:
        v = v * torch.tensor(scale, dtype=F32)
    return v.to(dtype)


def chain_ref(x, g, dtype):
    """SPPF backward (see the module docstring).  x (N, c, H, W) values of T, g (N, 4c, H, W) values of T.
    -> dict(v0 float64 gradient wrt x, noise n_0 float64, idx of the three pools, K of the last stage)"""
    x, g = _d(x), _d(g)
    c = x.shape[1]
    gs = [g[:, i * c:(i + 1) * c] for i in range(4)]
    y1, i1 = pool_ref(x)
    y2, i2 = pool_ref(y1)
    y3, i3 = pool_ref(y2)
    v, e = gs[3], torch.zeros_like(gs[3])                     # E_4 = 0
    for gk, ik in ((gs[2], i3), (gs[1], i2), (gs[0], i1)):
        s, _, k = pool_bwd_ref(v, ik, base=gk)
        re = route(ik, e)
        mass = gk.abs() + route(ik, v.abs() + e)
        n = gamma(k.double() - 1.0) * mass + re
        v, e = s, 0.5 * ulp(s.abs() + n, dtype) + n
    return {"v0": v, "noise": n, "idx": (i1, i2, i3), "k": k, "y": (y1, y2, y3)}


# ---------------------------------------------------------------------------------------------- shapes and inputs
# dense shapes (N, C, H, W), the smallest that reach each path: the present case; windows clipped on both sides and geom()'s ld
# rule for W == 1 and H == W == 1; C % 8 != 0 (V = 1 in 16 bit) and C % 4 != 0 (V = 1 in fp32)
POOL_SHAPES = [(2, 24, 9, 10), (2, 16, 1, 1), (1, 8, 1, 7), (1, 8, 6, 1), (2, 16, 3, 4), (2, 12, 5, 6), (2, 6, 5, 6)]
UP_SHAPES = [(2, 24, 9, 10), (2, 16, 1, 1), (1, 8, 1, 7), (2, 12, 5, 6)]
COPY_SHAPES = [(2, 12, 5, 7), (2, 16, 5, 7), (2, 6, 5, 7), (1, 8, 1, 1)]
SLICE_SHAPE = (2, 16, 7, 9)       # at channel offset 4 (fp32: 2) of a 24-wide buffer: C % V == 0, pointer not 16-byte aligned
SPPF_SHAPE = (2, 32, 20, 20)      # input slice 0, output slice 1 of a 128-wide buffer
GRID_CAP = 4096 * 256             # ew_grid: work items of one trip of the grid-stride loops


def big_shape(dtype):
    """more than GRID_CAP work items at V = 1: the second trip of the grid-stride loop"""
    s = (2, 6, 300, 300) if dtype == F32 else (2, 12, 210, 210)
    assert s[0] * s[1] * s[2] * s[3] > GRID_CAP and s[1] % (4 if dtype == F32 else 8)
    return s


def grid(shape, seed, dtype, edges=True, scale=2.0):
    """values on a half-integer grid (ties are common) with the edge rows, by channel (every shape here has C >= 6):
    0: a NaN, 1: +inf, 2: -inf next to the NaN's column, 3: image 0 all -inf (every window), 4: all negative,
    5: 2^-20 of the grid (rounds into f16's subnormal range)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(*shape, generator=g) * scale).round().div(2.0)
    if edges:
        n, c, h, w = shape
        assert c >= 6
        x[0, 0, 0, 0] = float("nan")
        x[n - 1, 1, h - 1, w - 1] = float("inf")
        x[0, 2, h // 2, w // 2] = float("-inf")
        x[0, 3] = float("-inf")
        x[:, 4] = -x[:, 4].abs() - 0.5
        x[:, 5] *= 2.0 ** -20
    return x.to(dtype)


def smooth(shape, seed, dtype, edges=True, scale=1.0):
    """gradients: randn, with by channel 0: a NaN, 1: +inf, 2: +inf and -inf in one 2x2 block where the map allows it,
    3: 64 + grid (cancellation partner, see cancel()), 5: 2^-18 randn (sums land in f16's subnormal range)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * scale
    if edges:
        n, c, h, w = shape
        assert c >= 6
        x[0, 0, 0, 0] = float("nan")
        x[n - 1, 1, h - 1, w - 1] = float("inf")
        x[0, 2, 0, 0] = float("inf")
        x[0, 2, 0, min(1, w - 1)] = float("-inf")
        x[:, 3] = 64.0 + (x[:, 3] * 2.0).round()
        x[:, 5] *= 2.0 ** -18
    return x.to(dtype)


def edge_vals(shape, seed, dtype):
    """values for the casts (any shape): randn * 3 with, from the front of the flattened tensor, NaN, +-inf, 1e-6 and -3e-8
    (f16: subnormal, and below half the smallest subnormal), 70000 (above f16's largest), 1 + 2^-8 and 1 + 3 2^-8 (bf16 ties),
    2^-140 (an fp32 subnormal), -0.0; a tensor with fewer than 12 elements keeps 1e-6 in front"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * 3.0
    f = x.view(-1)
    edge = [float("nan"), float("inf"), float("-inf"), 1e-6, -3e-8, 70000.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 2.0 ** -140, -0.0]
    if f.numel() >= 12:
        f[:len(edge)] = torch.tensor(edge)
    else:
        f[0] = 1e-6
    return x.to(dtype)


def cancel(xs):
    """add_n's cancellation row: channel 3 of source 1 is minus that of source 0 (large, opposite sign), the further
    sources stay small there"""
    xs = [x.clone() for x in xs]
    xs[1][:, 3] = -xs[0][:, 3]
    for x in xs[2:]:
        x[:, 3] = (x[:, 3].float() - 64.0) * 0.01
    return xs


# ---------------------------------------------------------------------------------------------- one check per operation
# x, dout, base, ...: what the kernel received (values of T, any device, logical N C H W); got: what it left
def check_pool_fwd(x, out, idx, what):
    """out (N, C, H, W) of T and idx (N, C, H, W) uint8, exact -> the reference idx"""
    val, ridx = pool_ref(x)
    assert_exact(idx, ridx, what + " idx", "pool_idx")
    assert_exact(out, val.to(out.dtype), what + " out", "pool_out")
    return ridx


def check_pool_bwd(dout, ridx, got, what, base=None):
    s, m, k = pool_bwd_ref(dout, ridx, base)
    return assert_sum(got, s, m, k, got.dtype, what, "move_pool")


def check_up_fwd(x, got, what):
    assert_exact(got, up_ref(x), what, "move_up")


def check_up_bwd(dout, got, what, base=None):
    s, m, k = sum_ref(up_bwd_terms(dout, base))
    return assert_sum(got, s, m, k, got.dtype, what, "move_up")


def check_copy(src, before, got, what, accumulate):
    """before: the destination as it was"""
    if not accumulate:
        return assert_exact(got, src.detach().cpu(), what, "move_copy")
    s, m, k = sum_ref([src, before])
    return assert_sum(got, s, m, k, got.dtype, what, "move_copy", mult=1.0)


def check_add(xs, got, what):
    s, m, k = sum_ref(xs)
    return assert_sum(got, s, m, k, got.dtype, what, "move_add", mult=1.0)


def check_cast(src, got, what, scale=None, family="exact"):
    assert_exact(got, cast_ref(src, got.dtype, scale).reshape(got.shape), what, family)


def check_chain(x, g, got, what):
    r = chain_ref(x, g, got.dtype)
    return assert_sum(got, r["v0"], torch.zeros_like(r["v0"]), r["k"], got.dtype, what, "move_chain", extra=r["noise"]), r


def report():
    lines =["[strict_move] exact class, comparisons / elements per family:"]
    lines += [f"[strict_move]   {f:16s} {v[0]:6d} {v[1]:12d}" for f, v in sorted(EXACT.items())]
    return "\n".join(lines)
