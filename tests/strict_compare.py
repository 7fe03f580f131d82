"""Strict per-element comparator for the convolution family (shared by the CPU tests of the comparator itself and by the
-m gpu tests of the kernels).

Contract of the kernels: 16-bit inputs, every product exact in fp32, the sum kept in fp32, bias / activation / residual /
accumulate sources added in fp32, ONE rounding to the output type.  For an output element with exact value `ref`
(float64, CPU, from the same rounded inputs) that gives

    |got - ref|  <=  1/2 ulp_T(max(|ref|, |got|))  +  c * 2^-24 * M  +  E_act

  ulp_T  spacing of the output type at that magnitude (bf16 8 significant bits, f16 11 with the exponent clamped at -14,
         fp32 24); exponent by torch.frexp.
  M      "mass": the same operation on absolute values in float64 (+ |bias|, |base|, |acc2| where the launch adds them;
         x 1.1 under SiLU, max |silu'| < 1.1).
  c      16 for every family (C below).  Any fp32 summation of K terms obeys (K-1) * 2^-24 * M; real orders are far
         inside: CPU fp32 F.conv2d and a per-tap / per-32-channel chunked order measure 0.4 .. 2.4 at K = 96 .. 4608, a
         k-ordered fp32 fma chain on the GPU 1.3 .. 5.9 up to K = 4096.  c may not be raised to make a test pass: a family
         that exceeds it is first reported (observed maximum, cause), then set to twice the observed value, never above
         K - 1.
  E_act  only with SiLU: (|v| + 4) * 2^-22 * |silu(v)|, v = conv + bias: __expf is a multiply by log2(e) (relative error
         |v| * 2^-24 in the result), then the hardware exp2 and a reciprocal of about one ulp each; twice that sum.

There is no tensor-wide floor: a small element is held to its own ulp.

Observed on the MI355X, maximum over all elements of all cases of (|got - ref| - 1/2 ulp - E_act) / (2^-24 * M), per
family (the GPU test modules print this table when they finish; c = 16 held for every family):

    tests/test_gpu_conv_variants.py (forced variants, partial tiles, config-2 replays at 32 images; 2.7e9 elements)
        gather 1.24   ring 1.31   rows 1.07   halo 0.97   patch (stride-2 data gradient) 1.21   launcher's choice 0.59
        wgrad product path (partials + reduce) 2.74        wgrad atomics path (algo 3) 1.40
    tests/test_gpu_kernels.py (every leaf on small maps)
        MFMA / launcher's choice 0.85, its wgrad 1.26      generic VALU kernels 0.43, their wgrad (atomics) 1.30 .. 1.41
        fp32 kernels 4.10 (fp32 inputs: the products round too), their wgrad 1.75
        stem 1.27, stem wgrad 1.01                         depthwise 3.10 (fp32 weights: products round), its wgrad 1.59
    The CPU stand-ins of tests/test_strict_compare_cpu.py (fp32 F.conv2d and the chunked order) stay below 5 on the same
    shapes.  No family needed more than c = 16.

Batches are built from THREE base images by image_pattern(): neighbouring images differ, every base appears in the
first, the middle and the last third; the float64 reference is computed for the three bases and every image of the batch
is compared.  A failure reports the count, the 64 worst elements and histograms by image, by 16-pixel block of the
flattened N*H*W index and by 16-channel block, so that one failing run shows the tile pattern."""
import torch
import torch.nn.functional as F

SIG_BITS = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}
EXP_MIN = {torch.bfloat16: -126, torch.float16: -14, torch.float32: -126}
U24 = 2.0 ** -24
C_DEFAULT = 16.0
# noise multiplier per kernel family (see the rule above before touching one)
# ("auto": the launcher's own choice; "generic": the VALU kernels of algo 1; "fp32": fp32 tensors)
C = {f: C_DEFAULT for f in ("gather", "ring", "rows", "halo", "patch", "auto", "generic", "fp32", "stem", "depthwise",
                            "wgrad", "wgrad_atomics", "auto_wgrad", "generic_wgrad", "fp32_wgrad", "stem_wgrad", "depthwise_wgrad")}
OBSERVED = {}          # family -> [max excess in units of 2^-24 M, elements compared, cases]
BUDGET_FAMILIES = set()   # families whose M is a whole noise budget / 2^-24 (strict_attention.py, strict_bn.py): the figure is a share, limit 1


class StrictMismatch(AssertionError):
    def __init__(self, msg, count, hist, worst):
        super().__init__(msg)
        self.count, self.hist, self.worst = count, hist, worst


def ulp(v, dtype):
    """spacing of `dtype` at magnitude |v| (float64 tensor): 2^(e - p + 1) for |v| in [2^e, 2^(e+1)), e clamped at the
    type's smallest normal exponent (so subnormals and zero get the fixed subnormal spacing)."""
    v = torch.as_tensor(v, dtype=torch.float64).abs()
    _, e = torch.frexp(v)                                  # v = m * 2^e, m in [0.5, 1)
    e = torch.where(v == 0, torch.full_like(e, EXP_MIN[dtype]), e - 1).clamp_(min=EXP_MIN[dtype])
    return torch.ldexp(torch.ones_like(v), e - (SIG_BITS[dtype] - 1))


def image_pattern(n, seed=0):
    """-> list of n base indices in {0, 1, 2}: neighbouring images differ; for n >= 9 every base appears in the first,
    the middle and the last third (for n < 9 a third holds fewer than three images: then every base appears at all)."""
    if n <= 3:
        return list(range(n))
    g = torch.Generator().manual_seed(1000 + seed)
    for _ in range(1000):
        p = [int(torch.randint(0, 3, (1,), generator=g))]
        while len(p) < n:
            p.append((p[-1] + 1 + int(torch.randint(0, 2, (1,), generator=g))) % 3)
        t = n // 3
        thirds = [p[:t], p[t:n - t], p[n - t:]] if n >= 9 else [p]
        if all(set(th) == {0, 1, 2} for th in thirds):
            return p
    raise RuntimeError("no pattern found")


def _d(t):
    return t.detach().to("cpu", torch.float64)


def conv_ref(x, w, k, s, groups=1):
    """float64 forward and its mass: (conv(x, w), conv(|x|, |w|))"""
    x, w = _d(x), _d(w)
    return F.conv2d(x, w, None, s, k // 2, 1, groups), F.conv2d(x.abs(), w.abs(), None, s, k // 2, 1, groups)


def dgrad_ref(dy, w, in_shape, k, s, groups=1):
    dy, w = _d(dy), _d(w)
    f = torch.nn.grad.conv2d_input
    return f(tuple(in_shape), w, dy, s, k // 2, 1, groups), f(tuple(in_shape), w.abs(), dy.abs(), s, k // 2, 1, groups)


def wgrad_ref(x, dy, w_shape, k, s, counts=None, groups=1):
    """float64 weight gradient and mass; with `counts` (one per image of x / dy) dw = sum_b counts[b] * dw(x[b], dy[b]):
    the batch gradient of a batch that holds image b counts[b] times."""
    x, dy = _d(x), _d(dy)
    f = torch.nn.grad.conv2d_weight
    if counts is None:
        return f(x, tuple(w_shape), dy, s, k // 2, 1, groups), f(x.abs(), tuple(w_shape), dy.abs(), s, k // 2, 1, groups)
    dw = torch.zeros(tuple(w_shape), dtype=torch.float64)
    m = torch.zeros_like(dw)
    for b, cnt in enumerate(counts):
        if cnt:
            dw += cnt * f(x[b:b + 1], tuple(w_shape), dy[b:b + 1], s, k // 2, 1, groups)
            m += cnt * f(x[b:b + 1].abs(), tuple(w_shape), dy[b:b + 1].abs(), s, k // 2, 1, groups)
    return dw, m


def silu_terms(v, mass):
    """v = conv + bias (float64), mass of v -> (silu(v), mass of silu(v), E_act)"""
    y = v * torch.sigmoid(v)
    return y, 1.1 * mass, (v.abs() + 4.0) * 2.0 ** -22 * y.abs()


def limit(ref, got, mass, dtype, c=C_DEFAULT, e_act=None):
    lim = 0.5 * ulp(torch.maximum(ref.abs(), got.abs()), dtype) + c * U24 * mass
    return lim if e_act is None else lim + e_act


def _top(h, k=16):
    return dict(sorted(h.items(), key=lambda kv: -kv[1])[:k])


def assert_close(got, ref, mass, dtype, what, family="auto", c=None, e_act=None, pattern=None, old_rel=None, old_abs=None):
    """got: (N, C, H, W) tensor of the kernel (any device / layout).  ref, mass, e_act: float64, of got's shape, or -- with
    `pattern` -- of shape (bases, C, H, W), image i of got being compared with base pattern[i].  A weight gradient
    (O, I, kh, kw) goes in as it is: 'image' is then the output channel, 'channel_block' the 16-block of input channels
    and 'pixel_block' the 16-block of the flattened (O, kh, kw) index.
    old_rel / old_abs: the limit the suite asserted before (old_rel * |ref| + old_abs); asserted to be no tighter than
    the new one anywhere, so that this comparator can never be the looser check."""
    c = C.get(family, C_DEFAULT) if c is None else c
    got = got.detach().cpu()
    n, ch = got.shape[0], got.shape[1]
    per = got[0, 0].numel() if got.dim() > 2 else 1
    pattern = list(range(n)) if pattern is None else list(pattern)
    assert len(pattern) == n and tuple(got.shape[1:]) == tuple(ref.shape[1:]) == tuple(mass.shape[1:]), \
        (what, tuple(got.shape), tuple(ref.shape), tuple(mass.shape), len(pattern))
    assert max(pattern) < ref.shape[0], (what, pattern, ref.shape)
    count, rows, excess = 0, [], float("-inf")
    h_img, h_pix, h_ch = {}, {}, {}
    per_base = {}
    for i in range(n):
        g = got[i].to(torch.float64)
        b = pattern[i]
        r = ref[b]
        if b not in per_base:                                # what does not depend on the kernel's output: once per base
            m = mass[b]
            extra = c * U24 * m if e_act is None else c * U24 * m + e_act[b]
            inv = torch.where(m > 0, 1.0 / (U24 * m).clamp_min(1e-300), torch.zeros_like(m))
            old = None if old_rel is None and old_abs is None else (old_rel or 0.0) * r.abs() + (old_abs or 0.0)
            per_base[b] = (r.abs(), extra, extra - c * U24 * m, inv, old)
        r_abs, extra, ea, inv, old = per_base[b]
        half = 0.5 * ulp(torch.maximum(r_abs, g.abs()), dtype)
        lim = half + extra
        err = (g - r).abs()
        if old is not None:
            wider = lim > old
            assert not bool(wider.any()), \
                f"{what}: the derived limit is wider than the limit asserted before on {int(wider.sum())} elements of image {i} " \
                f"(worst ratio {float((lim / old.clamp_min(1e-300)).max()):.3f})"
        excess = max(excess, float(torch.nan_to_num((err - half - ea) * inv, nan=float("inf")).max()))
        bad = ~(err <= lim)                                  # NaN counts as bad
        nb = int(bad.sum())
        if nb:
            count += nb
            idx = bad.nonzero()
            u = ulp(r, dtype)
            chan = idx[:, 0]
            pix = torch.full_like(chan, i * per)             # logical (row-major) index over N, H, W
            step = 1
            for d in range(g.dim() - 1, 0, -1):
                pix = pix + idx[:, d] * step
                step *= g.shape[d]
            h_img[i] = h_img.get(i, 0) + nb
            for key, cnt in zip(*torch.unique(pix // 16, return_counts=True)):
                h_pix[int(key)] = h_pix.get(int(key), 0) + int(cnt)
            for key, cnt in zip(*torch.unique(chan // 16, return_counts=True)):
                h_ch[int(key)] = h_ch.get(int(key), 0) + int(cnt)
            ratio = (err / lim)[bad]
            keep = torch.argsort(torch.nan_to_num(ratio, nan=float("inf")), descending=True)[:64]
            for j in keep.tolist():
                t = tuple(idx[j].tolist())
                rows.append((float(ratio[j]), (i,) + t, float(g[t]), float(r[t]), float(err[t] / u[t]), float(lim[t] / u[t])))
    o = OBSERVED.setdefault(family, [float("-inf"), 0, 0])
    o[0], o[1], o[2] = max(o[0], excess), o[1] + got.numel(), o[2] + 1
    if count:
        rows.sort(key=lambda t: -t[0] if t[0] == t[0] else float("-inf"))
        worst = [t[1:] for t in rows[:64]]
        hist = {"image": h_img, "pixel_block": h_pix, "channel_block": h_ch}
        lines = [f"{what} [{family}, c = {c:g}]: {count} of {got.numel()} elements outside 1/2 ulp + c 2^-24 M"
                 f"{' + E_act' if e_act is not None else ''}; max excess {excess:.2f} x 2^-24 M",
                 f"  by image: {_top(h_img)}", f"  by 16-pixel block of N*H*W ({len(h_pix)} blocks): {_top(h_pix)}",
                 f"  by 16-channel block: {_top(h_ch)}", "  worst (index, got, want, error / ulp, limit / ulp):"]
        lines += [f"    {ix}  {gv:.7g}  {rv:.7g}  {eu:.3f}  {lu:.3f}" for ix, gv, rv, eu, lu in worst]
        raise StrictMismatch("\n".join(lines), count, hist, worst)
    return excess


def assert_stats(acc_sums, y, what):
    """BatchNorm statistics epilogue: (2, C) fp32 sums of the kernel against float64 sums of the STORED values y
    (N, C, H, W); fp32 partial sums and float atomics: 2e-5 of the mass, no absolute term."""
    yd = _d(y)
    want = torch.stack([yd.sum((0, 2, 3)), (yd * yd).sum((0, 2, 3))])
    mass = torch.stack([yd.abs().sum((0, 2, 3)), (yd * yd).sum((0, 2, 3))])
    err = (_d(acc_sums) - want).abs()
    bad = ~(err <= 2e-5 * mass)
    assert not bool(bad.any()), f"{what}: BN statistics epilogue: {int(bad.sum())} sums outside 2e-5 of their mass, worst " \
                                f"{float((err / mass.clamp_min(1e-300)).max()):.3e}; channels {bad.any(0).nonzero().flatten().tolist()[:16]}"


def report():
    lines = ["[strict_compare] max of (|got - ref| - 1/2 ulp - E_act) / (2^-24 M) per family:"]
    for fam in sorted(f for f in OBSERVED if f not in BUDGET_FAMILIES):
        ex, elems, cases = OBSERVED[fam]
        lines.append(f"[strict_compare]   {fam:16s} {ex:8.3f}   (c = {C.get(fam, C_DEFAULT):g}; {cases} comparisons, {elems} elements)")
    att = sorted(f for f in OBSERVED if f in BUDGET_FAMILIES)
    if att:
        lines.append("[strict_compare] attention, BatchNorm: max of (|got - ref| - 1/2 ulp) / noise budget per family (limit 1):")
        for fam in att:
            ex, elems, cases = OBSERVED[fam]
            lines.append(f"[strict_compare]   {fam:16s} {ex:8.3f}   (c = {C.get(fam, C_DEFAULT):g}; {cases} comparisons, {elems} elements)")
    return "\n".join(lines)
