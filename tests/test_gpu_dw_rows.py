"""-m gpu: the depthwise rows kernels (k_dw3x3_rows, k_dw3x3_wgrad_rows in csrc/dwconv.hip) against the strip kernels they
replace (bit for bit where the contract says so) and against the float64 references of strict_compare / strict_bn.

Shapes: three distinct images, the smallest maps at which the walk can go wrong -- bands shorter than the 3-row window
(H = 1, 2, 3), a partial last band (H = 7, 37 at the 4-row minimum band), one column, fewer columns than a workgroup holds,
a partial last column block (W = 21), the re-planned 10 + 10 columns (W = 20, C = 128), one channel group, channel-group
counts that do not divide a workgroup (3, 17) and a second grid-y block of one packet (C = 2056); x or dy as a channel slice
of a wider buffer.  Maps this small take the strip kernels by default (forward / data gradient), so both variants are
forced through yolo_dw_tune_set.  Every case runs each launch once per variant; the references are computed once per case."""
import functools

import pytest
import torch

import strict_bn as sb
import strict_compare as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 3
# (C, H, W, x is a slice of a wider buffer, dy is one)
CASES = [(16, 1, 6, 0, 1), (16, 2, 6, 1, 0), (16, 3, 6, 0, 1), (16, 7, 6, 1, 0), (16, 37, 6, 0, 1), (16, 5, 1, 1, 0), (16, 5, 5, 0, 1),
         (128, 5, 21, 1, 0), (128, 5, 20, 0, 1), (8, 5, 6, 1, 0), (24, 6, 7, 0, 1), (136, 5, 6, 1, 0), (2056, 3, 5, 0, 1)]
DTYPES = [torch.bfloat16, torch.float16]
PAD = 16


def ops():
    from src.hipops import ops as o
    return o


def lib():
    from src.hipops import lib as l
    return l


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def place(t, pad, fill=7.0):
    """(N, C, H, W) values -> NHWC tensor on the GPU, as channels [pad/2, pad/2 + C) of a buffer of C + pad channels"""
    n, c, h, w = t.shape
    buf = ops().new_nhwc(n, c + pad, h, w, t.dtype, DEV)
    buf.fill_(fill)
    view = buf[:, pad // 2:pad // 2 + c]
    view.copy_(t.to(DEV))
    return buf, view


def outside(buf, c, pad):
    """the channels of `buf` that do not belong to the slice"""
    return torch.cat([buf[:, :pad // 2], buf[:, pad // 2 + c:]], 1).cpu()


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_variant(variant, case):
    """every launch of the case with the strip (1) or the rows (2) kernels forced -> dict of CPU results"""
    o, l = ops(), lib()
    c, h, w = case["chw"]
    dtype, code = case["dtype"], (l.BF16 if case["dtype"] == torch.bfloat16 else l.F16)
    x, dy, w9, bias = case["x_dev"], case["dy_dev"], case["w9"].to(DEV), case["bias"].to(DEV)
    l.call("yolo_dw_tune_set", variant)
    try:
        want = 1 if variant == 2 else 2                                             # the launches below really take that kernel
        assert l.query("yolo_dw_plan", N, h, w, c, 0) == want and l.query("yolo_dw_plan", N, h, w, c, 12) == want
        r = {"fwd": o.dw_fwd(x, w9).cpu()}
        acc = o.bn_acc_new(c, DEV)
        r["fwd_stats"], r["acc"] = o.dw_fwd(x, w9, acc).cpu(), acc.cpu()
        for act in (0, 1):
            y = o.dw_fwd_act(x, w9, bias, act)
            assert y is not None
            r[f"act{act}"] = y.cpu()
        r["dgrad"] = o.dw_dgrad(dy, w9).cpu()
        buf, view = place(case["prev"], PAD)                                        # fan-in into a slice of a wider buffer
        got = o.dw_dgrad(dy, w9, acc_into=view)
        r["dgrad_acc"], r["dgrad_acc_outside"] = got.cpu(), outside(buf, c, PAD)
        buf, view = place(torch.zeros(N, c, h, w, dtype=dtype), PAD)               # forward into a slice of a wider buffer
        l.call("yolo_dwconv3x3_fwd", x.data_ptr(), o.geom(x)[4], w9.data_ptr(), view.data_ptr(), c + PAD, N, h, w, c, code, stream())
        r["fwd_slice"], r["fwd_slice_outside"] = view.cpu(), outside(buf, c, PAD)
        nslab = l.query("yolo_dw_wgrad_nslab", N, h)
        r["wgrad"] = []
        for fill in (float("nan"), float("nan")):                                  # two runs, each into NaN-filled outputs
            part = torch.full((nslab * c * 9,), fill, dtype=torch.float32, device=DEV)
            dw = torch.full((c, 1, 3, 3), fill, dtype=torch.float32, device=DEV)
            l.call("yolo_dwconv3x3_wgrad", x.data_ptr(), o.geom(x)[4], dy.data_ptr(), o.geom(dy)[4], dw.data_ptr(), part.data_ptr(),
                   N, h, w, c, code, stream())
            r["wgrad"].append(dw.cpu())
        torch.cuda.synchronize()
        return r
    finally:
        l.call("yolo_dw_tune_set", 0)


@functools.lru_cache(maxsize=None)
def case_of(dtype, c, h, w, padx, pady):
    """inputs, float64 references and the results of both variants, once per case"""
    x = rnd(N, c, h, w, seed=50).to(dtype)
    dy = rnd(N, c, h, w, seed=51).to(dtype)
    case = {"chw": (c, h, w), "dtype": dtype, "x": x, "dy": dy, "w9": rnd(c, 9, seed=52, scale=0.3), "bias": rnd(c, seed=53, scale=0.5),
            "prev": rnd(N, c, h, w, seed=54).to(dtype)}
    case["x_dev"], case["dy_dev"] = place(x, PAD * padx)[1], place(dy, PAD * pady)[1]
    assert ops().geom(case["x_dev"])[4] == c + PAD * padx and ops().geom(case["dy_dev"])[4] == c + PAD * pady
    case["rows"], case["strip"] = run_variant(2, case), run_variant(1, case)
    return case


def params(f):
    f = pytest.mark.parametrize("c,h,w,padx,pady", CASES)(f)
    return pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])(f)


@pytest.fixture(autouse=True, scope="module")
def _print_observed_maxima():
    yield
    print("\n" + sc.report())


@params
def test_rows_equal_strip_bit_for_bit(dtype, c, h, w, padx, pady):
    """forward, forward with statistics, fused inference forward (act 0 / 1), data gradient, data gradient with acc_into"""
    case = case_of(dtype, c, h, w, padx, pady)
    rows, strip = case["rows"], case["strip"]
    for key in ("fwd", "fwd_stats", "act0", "act1", "dgrad", "dgrad_acc", "fwd_slice"):
        assert torch.equal(rows[key], strip[key]), (key, int((rows[key] != strip[key]).sum()))
    assert torch.equal(rows["fwd"], rows["fwd_stats"]) and torch.equal(rows["fwd"], rows["fwd_slice"])


@params
def test_rows_against_float64(dtype, c, h, w, padx, pady):
    case = case_of(dtype, c, h, w, padx, pady)
    rows, w4 = case["rows"], case["w9"].view(c, 1, 3, 3)
    y_ref, y_mass = sc.conv_ref(case["x"], w4, 3, 1, groups=c)
    sc.assert_close(rows["fwd"], y_ref, y_mass, dtype, "rows dw_fwd", "depthwise")
    b64 = case["bias"].double().view(1, -1, 1, 1)
    v, vmass = y_ref + b64, y_mass + b64.abs()
    sc.assert_close(rows["act0"], v, vmass, dtype, "rows dw_fwd_act act=0", "depthwise")
    sy, smass, e_act = sc.silu_terms(v, vmass)
    sc.assert_close(rows["act1"], sy, smass, dtype, "rows dw_fwd_act act=1", "depthwise", e_act=e_act)
    dx_ref, dx_mass = sc.dgrad_ref(case["dy"], w4, (N, c, h, w), 3, 1, groups=c)
    sc.assert_close(rows["dgrad"], dx_ref, dx_mass, dtype, "rows dw_dgrad", "depthwise")
    prev = case["prev"].double()
    sc.assert_close(rows["dgrad_acc"], dx_ref + prev, dx_mass + prev.abs(), dtype, "rows dw_dgrad acc_into", "depthwise")


@params
def test_rows_statistics(dtype, c, h, w, padx, pady):
    """the folded accumulator against the float64 sums of the STORED values, within strict_bn's limit for a sum"""
    case = case_of(dtype, c, h, w, padx, pady)
    r = sb.sums_fwd(case["rows"]["fwd_stats"], dtype)
    s, q = sb.fold(case["rows"]["acc"], c)
    sb.assert_within(s.float(), r["s"], torch.float32, f"rows dw_fwd stats sum {c}x{h}x{w}", "bn_sum")
    sb.assert_within(q.float(), r["q"], torch.float32, f"rows dw_fwd stats sumsq {c}x{h}x{w}", "bn_sumsq")


@params
def test_rows_weight_gradient(dtype, c, h, w, padx, pady):
    """bounded against float64 (another summation order than the strip kernel), bit-stable from run to run, every partial
    block the finalize reads written (the partial buffer and dw start as NaN)"""
    case = case_of(dtype, c, h, w, padx, pady)
    a, b = case["rows"]["wgrad"]
    assert torch.equal(a, b), int((a != b).sum())
    dw_ref, dw_mass = sc.wgrad_ref(case["x"], case["dy"], (c, 1, 3, 3), 3, 1, groups=c)
    sc.assert_close(a, dw_ref, dw_mass, torch.float32, "rows dw_wgrad", "depthwise_wgrad")
    sc.assert_close(case["strip"]["wgrad"][0], dw_ref, dw_mass, torch.float32, "strip dw_wgrad", "depthwise_wgrad")


@params
def test_rows_leave_the_neighbouring_channels_alone(dtype, c, h, w, padx, pady):
    case = case_of(dtype, c, h, w, padx, pady)
    for key in ("fwd_slice_outside", "dgrad_acc_outside"):
        t = case["rows"][key]
        assert t.shape[1] == PAD and bool((t == 7.0).all()), key


# ---------------------------------------------------------------------------------------------------------------------
# The maps above are too small for a band taller than four rows, so their walks never go round the register ring.  The
# layers the step runs do: 20- and 10-row bands (whole ring passes), 14-row bands on a 56-wide map (a partial last pass),
# 27- and 14-row bands in the weight gradient.  At these sizes the strip kernels are the reference (they are held to
# float64 on the small maps): forward and data gradient bit for bit, the weight gradient within twice the family's limit
# (each variant within c * 2^-24 * M of the exact sums, M taken from the strip kernel run on |x| and |dy|) plus an fp32 ulp.
LARGE = [(32, 128, 80, 80), (32, 256, 40, 40), (32, 128, 56, 56)]


@pytest.mark.parametrize("n,c,h,w", LARGE)
def test_rows_equal_strip_on_tall_bands(n, c, h, w):
    o, l = ops(), lib()
    g = torch.Generator(device=DEV).manual_seed(60)
    x = torch.randn(n, h, w, c, device=DEV, generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)
    dy = torch.randn(n, h, w, c, device=DEV, generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)
    prev = torch.randn(n, h, w, c, device=DEV, generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)
    w9 = torch.randn(c, 9, device=DEV, generator=g) * 0.3
    assert l.query("yolo_dw_plan", n, h, w, c, 5) > 5 and l.query("yolo_dw_plan", n, h, w, c, 8) > 4   # taller than the rings
    res = {}
    try:
        for name, variant in (("rows", 2), ("strip", 1)):
            l.call("yolo_dw_tune_set", variant)
            assert l.query("yolo_dw_plan", n, h, w, c, 0) == (1 if variant == 2 else 2)
            acc = o.bn_acc_new(c, DEV)
            res[name] = {"fwd": o.dw_fwd(x, w9, acc), "acc": acc, "dgrad": o.dw_dgrad(dy, w9),
                         "dgrad_acc": o.dw_dgrad(dy, w9, acc_into=prev.clone(memory_format=torch.preserve_format)),
                         "wgrad": o.dw_wgrad(x, dy), "wgrad2": o.dw_wgrad(x, dy), "mass": o.dw_wgrad(x.abs(), dy.abs())}
    finally:
        l.call("yolo_dw_tune_set", 0)
    rows, strip = res["rows"], res["strip"]
    for key in ("fwd", "dgrad", "dgrad_acc"):
        assert torch.equal(rows[key], strip[key]), (key, int((rows[key] != strip[key]).sum()))
    assert torch.equal(rows["wgrad"], rows["wgrad2"])
    a, b, m = rows["wgrad"].double(), strip["wgrad"].double(), strip["mass"].double()
    lim = 2 * sc.C["depthwise_wgrad"] * sc.U24 * m + sc.ulp(torch.maximum(a.abs(), b.abs()).cpu(), torch.float32).to(DEV)
    assert bool(((a - b).abs() <= lim).all()), float(((a - b).abs() / lim).max())
    sa, sq = sb.fold(rows["acc"], c)
    r = sb.sums_fwd(rows["fwd"], torch.bfloat16)
    sb.assert_within(sa.float(), r["s"], torch.float32, f"rows dw_fwd stats sum {c}x{h}x{w}", "bn_sum")
    sb.assert_within(sq.float(), r["q"], torch.float32, f"rows dw_fwd stats sumsq {c}x{h}x{w}", "bn_sumsq")
