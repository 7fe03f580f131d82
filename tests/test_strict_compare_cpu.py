"""CPU tests of tests/strict_compare.py: what proves, without a GPU, that the derived per-element bound passes the
kernels' arithmetic and fails arithmetic that is subtly wrong.

The stand-in does what the kernels do -- 16-bit inputs, fp32 accumulation, the epilogue in fp32, one rounding -- in two
summation orders: fp32 F.conv2d / conv2d_input / conv2d_weight, and partial sums per tap x per 32-deep K chunk (weight
gradient: per image x per slab of output rows) added one after another.  It must pass with ZERO elements out on every
shape of the forced-variant tests, in bf16 and f16; every mutant must fail on every one of them.  Batches have eight
images built from three bases by image_pattern()."""
import pytest
import torch
import torch.nn.functional as F

import strict_compare as sc

BF, HF = torch.bfloat16, torch.float16
N = 8
# (cin, cout, h, w, k, s): the shapes of tests/test_gpu_conv_variants.py's forced-variant tests
SHAPES = [(64, 128, 37, 41, 3, 1), (96, 200, 37, 41, 1, 1), (64, 64, 37, 41, 3, 2), (32, 136, 37, 41, 3, 1),     # gather / ring
          (64, 128, 23, 29, 3, 1), (160, 136, 37, 41, 3, 1), (128, 72, 37, 41, 3, 2),
          (32, 64, 37, 41, 3, 1), (96, 192, 37, 41, 3, 1),                                                       # halo
          (64, 128, 23, 20, 3, 1), (32, 64, 13, 40, 3, 1), (96, 200, 9, 20, 3, 1), (128, 72, 20, 40, 3, 1),      # rows
          (64, 136, 23, 37, 3, 1), (32, 64, 10, 16, 3, 1), (96, 64, 31, 80, 3, 1),
          (16, 32, 23, 37, 3, 1), (32, 16, 41, 16, 3, 1), (64, 24, 20, 33, 3, 1), (16, 16, 7, 50, 3, 1),
          (96, 72, 13, 40, 3, 1), (64, 64, 23, 37, 3, 1),
          (72, 96, 84, 100, 3, 2), (32, 64, 84, 100, 3, 2), (128, 32, 84, 100, 3, 2), (40, 64, 84, 100, 3, 2),   # stride-2 patch
          (64, 64, 45, 39, 3, 2)]
WGRAD_SHAPES = [(72, 88, 37, 41, 3, 1), (72, 88, 37, 41, 3, 2), (72, 88, 19, 23, 3, 1), (72, 88, 19, 23, 3, 2), (136, 120, 37, 41, 1, 1)]
IDS = [f"{a}-{b}-{c}x{d}-k{e}s{f}" for a, b, c, d, e, f in SHAPES]
WIDS = [f"{a}-{b}-{c}x{d}-k{e}s{f}" for a, b, c, d, e, f in WGRAD_SHAPES]


@pytest.fixture(autouse=True, scope="module")
def _threads():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))


def rnd(shape, seed, scale=1.0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def out_hw(h, w, k, s):
    return (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1


# ------------------------------------------------------------------------------------------ the stand-in (fp32)
def chunks(wt, dim):
    """weights with everything but one tap x one 32-deep chunk of dimension `dim` zeroed (adding the zero products is exact)"""
    for kh in range(wt.shape[2]):
        for kw in range(wt.shape[3]):
            for c0 in range(0, wt.shape[dim], 32):
                m = torch.zeros_like(wt)
                sl = [slice(None)] * 4
                sl[dim], sl[2], sl[3] = slice(c0, c0 + 32), slice(kh, kh + 1), slice(kw, kw + 1)
                m[tuple(sl)] = wt[tuple(sl)]
                yield (kh, kw, c0), m


def fwd32(x, wt, k, s, order, mutate=None):
    """fp32 sums of conv(x, wt); order 0: F.conv2d; order 1: tap x chunk partials added one after another.
    mutate(key, part) may alter one partial (the mutants that lose or misplace a chunk)."""
    x, wt = x.float(), wt.float()
    if order == 0:
        return F.conv2d(x, wt, None, s, k // 2)
    acc = None
    for key, m in chunks(wt, 1):
        part = F.conv2d(x, m, None, s, k // 2)
        if mutate is not None:
            part = mutate(key, part)
        acc = part if acc is None else acc + part
    return acc


def dgrad32(dy, wt, in_shape, k, s, order):
    dy, wt = dy.float(), wt.float()
    f = torch.nn.grad.conv2d_input
    if order == 0:
        return f(in_shape, wt, dy, s, k // 2)
    acc = None
    for _, m in chunks(wt, 0):
        part = f(in_shape, m, dy, s, k // 2)
        acc = part if acc is None else acc + part
    return acc


def wgrad32(x, dy, w_shape, k, s, order, drop=None):
    """fp32 weight gradient; order 1: per image x per slab of 8 output rows, added one after another.
    drop = (image, pixels): that image's last `pixels` output pixels are left out (mutant f)."""
    x, dy = x.float(), dy.float().clone()
    f = torch.nn.grad.conv2d_weight
    if drop is not None:
        dy[drop[0]].flatten(1)[:, -drop[1]:] = 0
    if order == 0:
        return f(x, w_shape, dy, s, k // 2)
    acc = torch.zeros(w_shape)
    for b in range(x.shape[0]):
        for r0 in range(0, dy.shape[2], 8):
            m = torch.zeros_like(dy[b:b + 1])
            m[:, :, r0:r0 + 8] = dy[b:b + 1, :, r0:r0 + 8]
            acc = acc + f(x[b:b + 1], w_shape, m, s, k // 2)
    return acc


def silu32(v):
    return v * (1.0 / (1.0 + torch.exp(-v)))


def case(cin, cout, h, w, k, s, dtype, seed=0):
    """three base images / gradients / accumulate sources, weights, bias, the batch pattern"""
    oh, ow = out_hw(h, w, k, s)
    d = dict(x=rnd((3, cin, h, w), seed + 1, dtype=dtype), wt=rnd((cout, cin, k, k), seed + 2, (cin * k * k) ** -0.5, dtype),
             dy=rnd((3, cout, oh, ow), seed + 3, dtype=dtype), base=rnd((3, cin, h, w), seed + 4, dtype=dtype),
             acc2=rnd((3, cin, h, w), seed + 5, dtype=dtype), res=rnd((3, cout, oh, ow), seed + 6, dtype=dtype),
             bias=rnd((cout,), seed + 7, 0.5, torch.float32), pat=sc.image_pattern(N, seed))
    return d


def old_abs(ref, frac=1e-3):
    return frac * float(ref.abs().max())


def old_rel(dtype):
    return 2.0 ** -8 if dtype == BF else 2.0 ** -10


# ------------------------------------------------------------------------------------------ ulp
def test_ulp_at_and_below_powers_of_two_subnormals_and_zero():
    t = lambda *v: torch.tensor(v, dtype=torch.float64)
    below = 1.0 - 2.0 ** -30
    assert sc.ulp(t(1.0, below, 2.0, 2.0 * below, 0.75, 3.0), BF).tolist() == [2.0 ** -7, 2.0 ** -8, 2.0 ** -6, 2.0 ** -7, 2.0 ** -8, 2.0 ** -6]
    assert sc.ulp(t(1.0, below, 1024.0, 1024.0 * below), HF).tolist() == [2.0 ** -10, 2.0 ** -11, 1.0, 0.5]
    assert sc.ulp(t(1.0, below, -1.0), torch.float32).tolist() == [2.0 ** -23, 2.0 ** -24, 2.0 ** -23]
    # f16: smallest normal 2^-14 has spacing 2^-24; everything below (subnormals, zero) keeps that spacing
    assert sc.ulp(t(2.0 ** -14, 2.0 ** -14 * below, 2.0 ** -20, 2.0 ** -24, 0.0, 2.0 ** -13), HF).tolist() == \
        [2.0 ** -24] * 5 + [2.0 ** -23]
    assert sc.ulp(t(0.0), BF).item() == 2.0 ** -133 and sc.ulp(t(0.0), torch.float32).item() == 2.0 ** -149
    # every representable neighbour is exactly one ulp away
    for dtype in (BF, HF):
        v = torch.tensor([0.3, 1.0, 1.5, 77.0, 1e-3], dtype=dtype)
        up = torch.nextafter(v, torch.full_like(v, 1e4))
        assert torch.equal((up.double() - v.double()), sc.ulp(v.double(), dtype))


def test_image_pattern_neighbours_differ_and_every_third_holds_every_base():
    for n in (2, 3, 4, 8, 9, 12, 32, 33):
        for seed in range(5):
            p = sc.image_pattern(n, seed)
            assert len(p) == n and all(a != b for a, b in zip(p, p[1:]))
            assert set(p) == set(range(min(n, 3)))
            if n >= 9:
                t = n // 3
                assert all(set(th) == {0, 1, 2} for th in (p[:t], p[t:n - t], p[n - t:]))
    assert sc.image_pattern(32, 1) == sc.image_pattern(32, 1)


def test_failure_report_counts_lists_and_histograms():
    ref = torch.ones(4, 32, 5, 8, dtype=torch.float64)
    got = ref.clone().to(BF)
    got[2, 17, 3, 1:4] += 2.0 ** -6
    got[3, 1, 0, 0] += 2.0 ** -6
    with pytest.raises(sc.StrictMismatch) as e:
        sc.assert_close(got, ref, ref, BF, "report", family="cpu_selftest")
    assert e.value.count == 4 and e.value.hist["image"] == {2: 3, 3: 1}
    assert e.value.hist["channel_block"] == {1: 3, 0: 1}
    assert e.value.hist["pixel_block"] == {(2 * 40 + 3 * 8 + 1) // 16: 3, (3 * 40) // 16: 1}
    assert len(e.value.worst) == 4 and "by 16-pixel block" in str(e.value) and "(2, 17, 3, 1)" in str(e.value)
    nan = got.clone()
    nan[0, 0, 0, 0] = float("nan")
    with pytest.raises(sc.StrictMismatch):
        sc.assert_close(nan, ref, ref, BF, "nan", family="cpu_selftest")


# ------------------------------------------------------------------------------------------ stand-in passes, mutants fail
def expand(t, pat):
    return t[pat]


def fails(got, ref, mass, dtype, what, **kw):
    with pytest.raises(sc.StrictMismatch) as e:
        sc.assert_close(got, ref, mass, dtype, what, family="cpu_selftest", **kw)
    return e.value


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_standin_passes_and_mutants_fail(shape, dtype):
    cin, cout, h, w, k, s = shape
    d = case(*shape, dtype, seed=cin + cout)
    pat = d["pat"]
    ref, mass = sc.conv_ref(d["x"], d["wt"], k, s)
    kw = dict(pattern=pat, old_rel=old_rel(dtype), old_abs=old_abs(ref))
    sums = [fwd32(d["x"], d["wt"], k, s, order) for order in (0, 1)]
    for order in (0, 1):
        sc.assert_close(expand(sums[order].to(dtype), pat), ref, mass, dtype, f"forward order {order}", family="cpu_selftest", **kw)
    good = expand(sums[0].to(dtype), pat)
    # (c) / (d): one 32-deep chunk of the centre tap missing in / taken from the next pixel tile for ONE 16 x 16 fragment
    npix = ref.shape[2] * ref.shape[3]
    p0, o0 = (3 * npix // 2) // 16 * 16, (cout // 2) // 16 * 16            # a fragment in the middle of base image 1
    frag_img, frag_p = divmod(p0, npix)
    for stale in (False, True):
        def mutate(key, part):
            if key != (k // 2, k // 2, 0):
                return part
            flat = part.permute(1, 0, 2, 3).reshape(cout, -1).clone()    # (O, bases * H * W)
            flat[o0:o0 + 16, p0:p0 + 16] = flat[o0:o0 + 16, p0 + 16:p0 + 32] if stale else 0.0
            return flat.view(cout, 3, *part.shape[2:]).permute(1, 0, 2, 3)
        bad = fwd32(d["x"], d["wt"], k, s, 1, mutate).to(dtype)
        e = fails(bad, ref, mass, dtype, "chunk " + ("stale" if stale else "missing"))
        assert set(e.hist["pixel_block"]) == {p0 // 16} and set(e.hist["channel_block"]) == {o0 // 16}, e.hist
        assert set(e.hist["image"]) == {frag_img} and e.count >= 128, (e.count, e.hist)
        assert f"{p0 // 16}: {e.count}" in str(e)
    # (e) three elements of ordinary size moved by two ulps
    moved = good.clone()
    big = (ref[pat].abs() >= 2.0 ** -4 * float(ref.abs().max())).flatten().nonzero().flatten()
    pick = big[torch.tensor([len(big) // 7, len(big) // 2, len(big) - 5])]
    v = moved.flatten()[pick]
    for _ in range(2):                                      # away from zero: each step is a whole ulp of the element
        v = torch.nextafter(v, torch.sign(v) * float("inf"))
    moved.view(-1)[pick] = v
    assert fails(moved, ref, mass, dtype, "three elements two ulps off", pattern=pat).count == 3
    # (g) image 5 computed from image 4's input
    swapped = good.clone()
    swapped[5] = good[4]
    e = fails(swapped, ref, mass, dtype, "image 5 from image 4's input", pattern=pat)
    assert set(e.hist["image"]) == {5} and e.count > 0.5 * swapped[5].numel()


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fused_epilogue_standin_passes_and_mutants_fail(shape, dtype):
    """act(conv + bias) + residual: one rounding passes; residual or bias added after the rounding fails"""
    cin, cout, h, w, k, s = shape
    d = case(*shape, dtype, seed=cin + cout + 1)
    pat = d["pat"]
    conv, cmass = sc.conv_ref(d["x"], d["wt"], k, s)
    b64, b32 = d["bias"].double().view(1, -1, 1, 1), d["bias"].view(1, -1, 1, 1)
    v, vmass = conv + b64, cmass + b64.abs()
    res64, res32 = d["res"].double(), d["res"].float()
    sy, smass, e_act = sc.silu_terms(v, vmass)
    sums = [fwd32(d["x"], d["wt"], k, s, order) for order in (0, 1)]
    for act in (1, 0):
        for with_res in (False, True):
            ref = (sy if act else v) + (res64 if with_res else 0.0)
            mass = (smass if act else vmass) + (res64.abs() if with_res else 0.0)
            kw = dict(pattern=pat, e_act=e_act if act else None)
            tol = {BF: 2.0 ** -6, HF: 2.0 ** -9}[dtype] * 2.0 * float(ref.abs().max())     # check(..., mult=2.0) of test_gpu_kernels.py
            for order in (0, 1):
                a = sums[order] + b32
                a = silu32(a) if act else a
                got = (a + res32 if with_res else a).to(dtype)
                sc.assert_close(expand(got, pat), ref, mass, dtype, f"fused act={act} res={with_res} order {order}",
                                family="cpu_selftest", old_abs=tol, **kw)
            # (b) bias added after the rounding
            a = sums[0].to(dtype).float() + b32
            a = silu32(a) if act else a
            late_bias = (a + res32 if with_res else a).to(dtype)
            if not act:        # under SiLU a late bias is a different function altogether; the identity form is the subtle one
                fails(expand(late_bias, pat), ref, mass, dtype, "bias after rounding", **kw)
            # (a) residual added after the rounding
            if with_res:
                a = sums[0] + b32
                a = silu32(a) if act else a
                late_res = (a.to(dtype).float() + res32).to(dtype)
                e = fails(expand(late_res, pat), ref, mass, dtype, "residual after rounding", **kw)
                assert e.count > 0.02 * ref[pat].numel(), e.count


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_data_gradient_standin_passes_and_double_rounding_fails(shape, dtype):
    cin, cout, h, w, k, s = shape
    d = case(*shape, dtype, seed=cin + cout + 2)
    pat = d["pat"]
    in_shape = (3, cin, h, w)
    ref, mass = sc.dgrad_ref(d["dy"], d["wt"], in_shape, k, s)
    base64, a264 = d["base"].double(), d["acc2"].double()
    sums = [dgrad32(d["dy"], d["wt"], in_shape, k, s, order) for order in (0, 1)]
    forms = [("plain", ref, mass, lambda a: a),
             ("accumulate", ref + base64, mass + base64.abs(), lambda a: a + d["base"].float())]
    if s == 1:
        forms.append(("acc2", ref + base64 + a264, mass + base64.abs() + a264.abs(), lambda a: a + d["base"].float() + d["acc2"].float()))
    for name, r, m, epi in forms:
        for order in (0, 1):
            sc.assert_close(expand(epi(sums[order]).to(dtype), pat), r, m, dtype, f"dgrad {name} order {order}", family="cpu_selftest",
                            pattern=pat, old_rel=old_rel(dtype), old_abs=old_abs(r))
    # (a) the accumulate form rounded twice: round(dgrad), then + base
    twice = (sums[0].to(dtype).float() + d["base"].float()).to(dtype)
    e = fails(expand(twice, pat), ref + base64, mass + base64.abs(), dtype, "accumulate after rounding", pattern=pat)
    assert e.count > 0.02 * twice[pat].numel(), e.count
    if s == 1:
        twice = (sums[0].to(dtype).float() + d["base"].float() + d["acc2"].float()).to(dtype)
        fails(expand(twice, pat), ref + base64 + a264, mass + base64.abs() + a264.abs(), dtype, "acc2 after rounding", pattern=pat)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=WIDS)
def test_weight_gradient_standin_passes_and_a_missing_slab_fails(shape, dtype):
    cin, cout, h, w, k, s = shape
    d = case(*shape, dtype, seed=cin + cout + 3)
    pat = d["pat"]
    counts = [pat.count(b) for b in range(3)]
    w_shape = (cout, cin, k, k)
    ref, mass = sc.wgrad_ref(d["x"], d["dy"], w_shape, k, s, counts)
    full, _ = sc.wgrad_ref(d["x"][pat], d["dy"][pat], w_shape, k, s)
    assert float((full - ref).abs().max()) <= 1e-12 * float(mass.max())        # the count-weighted sum IS the batch gradient
    x, dy = d["x"][pat], d["dy"][pat]
    for order in (0, 1):
        sc.assert_close(wgrad32(x, dy, w_shape, k, s, order), ref, mass, torch.float32, f"wgrad order {order}", family="cpu_selftest",
                        old_abs=3e-4 * float(ref.abs().max()))
    # (f) the last 64 pixels of one image left out
    e = fails(wgrad32(x, dy, w_shape, k, s, 0, drop=(5, 64)), ref, mass, torch.float32, "64 pixels of image 5 missing")
    assert e.count > 0.5 * ref.numel(), e.count


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
def test_statistics_standin_stays_inside_2e5_of_the_mass_without_an_absolute_term(dtype):
    """eight replicas, each an fp32 sum in a shuffled order (float atomics): the BatchNorm statistics bound needs no
    absolute floor; a statistics epilogue that skips one 16-pixel block of one image fails it."""
    for cin, cout, h, w, k, s in SHAPES[:4] + [(128, 128, 160, 160, 3, 2)]:
        oh, ow = out_hw(h, w, k, s)
        n = 32 if h == 160 else 3
        c = min(cout, 16)
        y = rnd((n, c, oh, ow), cout, dtype=dtype)
        flat = y.float().permute(1, 0, 2, 3).reshape(c, -1)
        perm = torch.randperm(flat.shape[1], generator=torch.Generator().manual_seed(3))
        flat = flat[:, perm]
        acc = torch.zeros(2, c)
        for r in range(8):                              # torch.cumsum in fp32 is a serial chain
            part = flat[:, r::8]
            acc[0] += part.cumsum(1)[:, -1]
            acc[1] += (part * part).cumsum(1)[:, -1]
        sc.assert_stats(acc, y, "stand-in")
        if n == 3:
            short = y.float().clone()
            short[1, :, 0, :16] = 0
            with pytest.raises(AssertionError):
                sc.assert_stats(torch.stack([short.sum((0, 2, 3)), (short * short).sum((0, 2, 3))]), y, "16 pixels missing")
