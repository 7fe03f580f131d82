"""-m gpu: every kernel family at and across its 32-bit addressing limit (the contract: tests/strict_addressing.py; the audit
of each family's largest index expression: DESIGN.md, "Addressing limits").

Construction: the tensor under test is a channel slice (16 or 64 channels) of an NHWC buffer of nine 61 x 59 images whose ROW
STRIDE carries the span across the limit -- the work stays small, the descriptors, byte offsets and element indices do not:
    conv / flat, under   the largest ld % 8 == 0 that keeps what the family's guard counts below 2^30 elements (2^31 bytes):
                         the fast family runs with offsets just below the wrap -- the dangerous side
    conv / flat, over    ld + 8: the guard must have moved the launch to the fallback.  In the "flat" pair (weight-gradient dy,
                         depthwise) the slice itself then ends past 2^31 bytes; in the "conv" pair only the shifted
                         descriptor's count (+ W + 1 rows) passes 2^30 and the slice still ends 3.5 MB below 2^31 bytes: that
                         pair tests the guard's position, not the fallback's arithmetic -- for which there is
    2g                   the buffer crosses 2^31 ELEMENTS (4.3 GB): an `int` byte offset or element index would wrap; for the
                         fallbacks' sources ("over2g"), the unguarded kernels and every destination (no guard covers one)
Every layout comes from strict_addressing.layout / layout_2g, the constructors the wrap-mutant test enumerates.  bf16
throughout, with an f16 twin per guarded family (gather, ring, the fallback, both weight-gradient designs, the depthwise
kernels) and the GEMM-route attention case.
Buffers are filled and their guard channels compared on the device; only the slice comes to the CPU, for the unchanged
bounds of strict_compare / strict_move / strict_bn / strict_stem_bwd / strict_attention.  Every image is compared (three base images, strict_compare.image_pattern), every
case asserts the family it reaches (plan query under a forced tune setting and algo 2 = "MFMA or error" at the real row
strides; the weight gradient by its workspace size; depthwise by the fused entry points' "not taken" code), the
argument-range checker is installed around lib.call / lib.query, and a case frees its buffers before the next."""
import gc

import pytest
import torch

import strict_addressing as sa
import strict_compare as sc
import strict_move as sm

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, HF = torch.bfloat16, torch.float16
N, H, W = sa.NPIX_IMG
DEFAULT_TUNE = (0, -1, -1, -1, -1, 0, 0, 0)
PAT = sc.image_pattern(N, 0)
# family -> (yolo_conv_tune_set arguments that force it for 64 -> 64 channels 3x3 stride 1 on a 61 x 59 map, its plan code)
FORCE = {"gather": ((64, -1, 0, -1, 0, 0, 0, 0), 1064), "halo": ((0, -1, 3, -1, 0, 0, 0, 0), 2003),
         "rows": ((0, -1, 14, -1, 0, 0, 0, 0), 4006), "ring": ((64, -1, 0, -1, 1, 128, 0, 0), 3064)}


def ops():
    from src.hipops import ops as o
    return o


def lib():
    from src.hipops import lib as l
    return l


@pytest.fixture(autouse=True)
def _checked_and_clean(monkeypatch):
    seen = sa.install_checker(monkeypatch)
    yield
    assert seen, "no call went through the argument-range checker"
    from src.hipops import lib as l
    l.call("yolo_conv_tune_set", *DEFAULT_TUNE)
    l.call("yolo_dw_tune_set", 0)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True, scope="module")
def _print_observed_maxima():
    yield
    print("\n" + sc.report() + "\n" + sm.report())


def rnd(shape, seed, scale=1.0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def code(T):
    return sa.BF16 if T == BF else sa.F16


def batch(c, h, w, seed, scale=1.0, dtype=BF):
    """-> (three base images, pattern, the nine-image batch); ONE pattern for every tensor of the module, so that image i of
    x, dy, a residual and an accumulate base all come from base PAT[i]"""
    base = rnd((3, c, h, w), seed, scale, dtype)
    return base, PAT, base[PAT]


def stream():
    return torch.cuda.current_stream().cuda_stream


def expect_no_mfma(fn, what):
    """algo 2 = "an MFMA kernel or an error": past the limit the launcher must refuse before it launches anything"""
    with pytest.raises(RuntimeError, match=str(sa.ERR_ARG)):
        fn()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ dense conv, source side
# "over": ld + 8, only the shifted descriptor's count passes 2^30 (the slice itself still ends below 2^31 bytes); "over2g": the
# source slice in the 4.3 GB buffer, so the fallback's own source offsets pass 2^31 bytes AND 2^31 elements
CONV_CASES = [("gather", "under", "top", BF), ("halo", "under", "bottom", BF), ("rows", "under", "top", BF), ("ring", "under", "mid", BF),
              ("gather", "under", "mid", HF), ("ring", "under", "top", HF),
              ("generic", "over", "top", BF), ("generic", "over", "bottom", BF), ("generic", "over2g", "top", BF),
              ("generic", "over2g", "mid", HF)]


@pytest.mark.parametrize("family,side,where,T", CONV_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_conv_forward_and_data_gradient_source_across_the_limit(family, side, where, T, monkeypatch):
    o, l = ops(), lib()
    c, k, s = 64, 3, 1
    lay = sa.layout("2g" if side == "over2g" else "conv", c, side, where)
    geom = sa.Geom(0, N, H, W, c, H, W, c, k, s, 0, lay.ld, c)
    assert sa.mfma_conv_eligible(geom, code(T)) == (side == "under") and (lay.conv_desc_elems < sa.DESC_ELEMS) == (side == "under")
    if side == "under":
        l.call("yolo_conv_tune_set", *FORCE[family][0])
        for mode in (0, 1):
            got = l.query("yolo_conv2d_plan", N, H, W, c, H, W, c, k, s, mode, 0, code(T))
            assert got == FORCE[family][1], f"the forced setting does not reach {family}: plan {got}"
        monkeypatch.setattr(o, "ALGO", 2)                    # MFMA or error, at the real row strides
    xb, pat, x9 = batch(c, H, W, 11, dtype=T)
    wt = rnd((c, c, k, k), 12, (c * k * k) ** -0.5, T)
    wp, wb = o.pack_weights(wt.float().to(DEV), k, s, 0, T), o.pack_weights(wt.float().to(DEV), k, s, 1, T)
    what = f"{family} {str(T)[6:]} {lay}"
    # ---- forward + statistics
    xbuf, xv = sa.put(lay, x9, 3.0)
    if side != "under":
        monkeypatch.setattr(o, "ALGO", 2)
        ytmp = o.new_nhwc(N, c, H, W, T, DEV).fill_(5.0)
        expect_no_mfma(lambda: o.conv_fwd(xv, wp, None, c, k, s, out=ytmp), what)
        assert bool((ytmp == 5.0).all()), "the refused launch wrote its destination"
        assert o.conv_fwd_act(xv, wp, torch.zeros(c, device=DEV), c, k, s, 1) is None, "the fused epilogue found an MFMA kernel past the limit"
        monkeypatch.setattr(o, "ALGO", 0)
        del ytmp
    acc = o.bn_acc_new(c, DEV)
    y = o.conv_fwd(xv, wp, None, c, k, s, acc)
    y_ref, y_mass = sc.conv_ref(xb, wt, k, s)
    sc.assert_close(y, y_ref, y_mass, T, f"conv_fwd {what}", family, pattern=pat)
    sc.assert_stats(acc.view(o.BN_REPL, 2, c).sum(0), y, f"conv_fwd {what}")
    sa.assert_guard_channels(xbuf, lay, 3.0, f"conv_fwd {what}")
    del xbuf, xv, y
    torch.cuda.empty_cache()
    # ---- data gradient, plain and accumulate (the source is dy)
    dyb, _, dy9 = batch(c, H, W, 13, dtype=T)
    dbuf, dv = sa.put(lay, dy9, -2.0)
    dx_ref, dx_mass = sc.dgrad_ref(dyb, wt, (3, c, H, W), k, s)
    if side != "under":
        monkeypatch.setattr(o, "ALGO", 2)
        expect_no_mfma(lambda: o.conv_dgrad(dv, wb, c, H, W, k, s), what)
        monkeypatch.setattr(o, "ALGO", 0)
    dx = o.conv_dgrad(dv, wb, c, H, W, k, s)
    sc.assert_close(dx, dx_ref, dx_mass, T, f"conv_dgrad plain {what}", family, pattern=pat)
    baseb, _, base9 = batch(c, H, W, 14, dtype=T)
    small = sa.Layout("dx", N, H, W, c, c + 32, 16)
    bbuf, bv = sa.put(small, base9, 9.0)
    o.conv_dgrad(dv, wb, c, H, W, k, s, acc_into=bv)
    sa.assert_guard_channels(bbuf, small, 9.0, f"conv_dgrad acc {what}")
    sc.assert_close(bv, dx_ref + baseb.double(), dx_mass + baseb.double().abs(), T, f"conv_dgrad acc {what}", family, pattern=pat)
    sa.assert_guard_channels(dbuf, lay, -2.0, f"conv_dgrad {what}")


S2_CASES = [("patch", "under"), ("gather", "under"), ("generic", "over")]


@pytest.mark.parametrize("family,side", S2_CASES, ids=lambda v: str(v))
def test_stride2_forward_and_parity_classes_across_the_limit(family, side, monkeypatch):
    """3x3 stride 2: the data gradient's source is dy (61 x 59, the wide buffer), dx is 122 x 118 (even: the patch kernel) or
    121 x 117 (odd: four parity classes of different sizes through the gather kernel)"""
    o, l = ops(), lib()
    c, k, s = 64, 3, 2
    h, w = (2 * H, 2 * W) if family != "gather" else (2 * H - 1, 2 * W - 1)
    assert o.conv_out_hw(h, w, k, s) == (H, W)
    lay = sa.layout("conv", c, side, "top")
    if side == "under":
        if family == "gather":
            l.call("yolo_conv_tune_set", *FORCE["gather"][0])
        for cls in range(4):
            got = l.query("yolo_conv2d_plan", N, h, w, c, H, W, c, k, s, 1, cls, sa.BF16)
            assert got // 1000 == (5 if family == "patch" else 1), f"class {cls}: plan {got}"
        monkeypatch.setattr(o, "ALGO", 2)
    wt = rnd((c, c, k, k), 22, (c * k * k) ** -0.5)
    wb = o.pack_weights(wt.float().to(DEV), k, s, 1, BF)
    dyb, pat, dy9 = batch(c, H, W, 23)
    dbuf, dv = sa.put(lay, dy9, -2.0)
    what = f"{family} {lay}"
    if side == "over":
        monkeypatch.setattr(o, "ALGO", 2)
        expect_no_mfma(lambda: o.conv_dgrad(dv, wb, c, h, w, k, s), what)
        monkeypatch.setattr(o, "ALGO", 0)
    dx_ref, dx_mass = sc.dgrad_ref(dyb, wt, (3, c, h, w), k, s)
    dx = o.conv_dgrad(dv, wb, c, h, w, k, s)
    sc.assert_close(dx, dx_ref, dx_mass, BF, f"conv_dgrad s2 plain {what}", family, pattern=pat)
    baseb, _, base9 = batch(c, h, w, 24)
    small = sa.Layout("dx", N, h, w, c, c + 32, 16)
    bbuf, bv = sa.put(small, base9, 9.0)
    o.conv_dgrad(dv, wb, c, h, w, k, s, acc_into=bv)
    sa.assert_guard_channels(bbuf, small, 9.0, f"conv_dgrad s2 acc {what}")
    sc.assert_close(bv, dx_ref + baseb.double(), dx_mass + baseb.double().abs(), BF, f"conv_dgrad s2 acc {what}", family, pattern=pat)
    sa.assert_guard_channels(dbuf, lay, -2.0, what)
    del dbuf, dv, bbuf, bv, dx
    torch.cuda.empty_cache()
    # ---- forward stride 2 from a 61 x 59 source in the wide buffer
    wp = o.pack_weights(wt.float().to(DEV), k, s, 0, BF)
    xb, pat, x9 = batch(c, H, W, 25)
    xbuf, xv = sa.put(lay, x9, 3.0)
    if side == "over":
        monkeypatch.setattr(o, "ALGO", 2)
        expect_no_mfma(lambda: o.conv_fwd(xv, wp, None, c, k, s), what)
        monkeypatch.setattr(o, "ALGO", 0)
    y = o.conv_fwd(xv, wp, None, c, k, s)
    y_ref, y_mass = sc.conv_ref(xb, wt, k, s)
    sc.assert_close(y, y_ref, y_mass, BF, f"conv_fwd s2 {what}", "generic" if side == "over" else "auto", pattern=pat)
    sa.assert_guard_channels(xbuf, lay, 3.0, what)


# ------------------------------------------------------------------------------------------ dense conv, destination side
@pytest.mark.parametrize("family", ["gather", "halo", "rows", "ring", "patch"])
def test_conv_destination_slice_in_a_buffer_past_2_31_elements(family, monkeypatch):
    """small dense source, the destination a slice of a 4.3 GB buffer: no guard looks at the destination, so the MFMA family
    itself stores (and, accumulating, reads) past 2^31 elements"""
    o, l = ops(), lib()
    c, k = 64, 3
    s = 2 if family == "patch" else 1
    lay = sa.layout("2g", c, "over", "top" if family in ("gather", "rows") else "bottom")
    assert lay.elems >= (1 << 31)
    if family != "patch":
        l.call("yolo_conv_tune_set", *FORCE[family][0])
    monkeypatch.setattr(o, "ALGO", 2)
    wt = rnd((c, c, k, k), 32, (c * k * k) ** -0.5)
    what = f"{family} -> {lay}"
    if family != "patch":
        assert l.query("yolo_conv2d_plan", N, H, W, c, H, W, c, k, s, 0, 0, sa.BF16) == FORCE[family][1]
        wp = o.pack_weights(wt.float().to(DEV), k, s, 0, BF)
        xb, pat, x9 = batch(c, H, W, 33)
        ybuf, yv = sa.wide_buffer(lay, BF, 5.0)
        acc = o.bn_acc_new(c, DEV)
        o.conv_fwd(x9.to(DEV).contiguous(memory_format=torch.channels_last), wp, None, c, k, s, acc, out=yv)
        sa.assert_guard_channels(ybuf, lay, 5.0, f"conv_fwd {what}")
        y_ref, y_mass = sc.conv_ref(xb, wt, k, s)
        sc.assert_close(yv, y_ref, y_mass, BF, f"conv_fwd {what}", family, pattern=pat)
        sc.assert_stats(acc.view(o.BN_REPL, 2, c).sum(0), yv, f"conv_fwd {what}")
        # the fused inference epilogue into the same slice: bias, SiLU
        bias = rnd((c,), 34, 0.5, torch.float32)
        ybuf.fill_(-6.0)
        assert o.conv_fwd_act(x9.to(DEV).contiguous(memory_format=torch.channels_last), wp, bias.to(DEV), c, k, s, 1, out=yv) is not None
        sa.assert_guard_channels(ybuf, lay, -6.0, f"conv_fwd_act {what}")
        b64 = bias.double().view(1, -1, 1, 1)
        sy, smass, e_act = sc.silu_terms(y_ref + b64, y_mass + b64.abs())
        sc.assert_close(yv, sy, smass, BF, f"conv_fwd_act {what}", family, e_act=e_act, pattern=pat)
        del ybuf, yv
        torch.cuda.empty_cache()
        h, w = H, W
    else:
        h, w = 2 * H, 2 * W
        lay = sa.layout_2g(N, h, w, c, "bottom")
        assert l.query("yolo_conv2d_plan", N, h, w, c, H, W, c, k, s, 1, 3, sa.BF16) // 1000 == 5
    # ---- data gradient accumulated into a slice of the 4.3 GB buffer
    wb = o.pack_weights(wt.float().to(DEV), k, s, 1, BF)
    dyb, pat, dy9 = batch(c, H, W, 35)
    baseb, _, base9 = batch(c, h, w, 36)
    dxbuf, dxv = sa.put(lay, base9, 9.0)
    o.conv_dgrad(dy9.to(DEV).contiguous(memory_format=torch.channels_last), wb, c, h, w, k, s, acc_into=dxv)
    sa.assert_guard_channels(dxbuf, lay, 9.0, f"conv_dgrad acc {what}")
    dx_ref, dx_mass = sc.dgrad_ref(dyb, wt, (3, c, h, w), k, s)
    sc.assert_close(dxv, dx_ref + baseb.double(), dx_mass + baseb.double().abs(), BF, f"conv_dgrad acc {what}", family, pattern=pat)


@pytest.mark.parametrize("family", ["gather", "halo", "rows", "ring"])
def test_fused_epilogue_residual_and_output_in_over_limit_buffers(family, monkeypatch):
    """act(conv + bias) + residual: the residual slice and the output slice each in a buffer past 2^30 elements (2 x 2.2 GB)"""
    o, l = ops(), lib()
    c, k, s = 64, 3, 1
    l.call("yolo_conv_tune_set", *FORCE[family][0])
    assert l.query("yolo_conv2d_plan", N, H, W, c, H, W, c, k, s, 0, 0, sa.BF16) == FORCE[family][1]
    rlay, ylay = sa.layout("flat", c, "over", "top"), sa.layout("conv", c, "over", "bottom")
    wt, bias = rnd((c, c, k, k), 42, (c * k * k) ** -0.5), rnd((c,), 43, 0.5, torch.float32)
    wp = o.pack_weights(wt.float().to(DEV), k, s, 0, BF)
    xb, pat, x9 = batch(c, H, W, 44)
    resb, _, res9 = batch(c, H, W, 45)
    rbuf, rv = sa.put(rlay, res9, 2.0)
    ybuf, yv = sa.wide_buffer(ylay, BF, 5.0)
    assert o.conv_fwd_act(x9.to(DEV).contiguous(memory_format=torch.channels_last), wp, bias.to(DEV), c, k, s, 1, rv, out=yv) is not None
    sa.assert_guard_channels(ybuf, ylay, 5.0, f"conv_fwd_act {family}")
    sa.assert_guard_channels(rbuf, rlay, 2.0, f"conv_fwd_act {family}")
    conv, cmass = sc.conv_ref(xb, wt, k, s)
    b64 = bias.double().view(1, -1, 1, 1)
    sy, smass, e_act = sc.silu_terms(conv + b64, cmass + b64.abs())
    sc.assert_close(yv, sy + resb.double(), smass + resb.double().abs(), BF, f"conv_fwd_act res {family} {rlay} -> {ylay}", family,
                    e_act=e_act, pattern=pat)


# ------------------------------------------------------------------------------------------ weight gradient
@pytest.mark.parametrize("k,s", [(1, 1), (3, 1), (3, 2)])
@pytest.mark.parametrize("operand,side,T", [("x", "under", BF), ("x", "over", BF), ("dy", "under", BF), ("dy", "over", BF),
                                            ("x", "over2g", BF), ("dy", "over2g", HF), ("x", "under", HF)], ids=lambda v: str(v).replace("torch.", ""))
def test_weight_gradient_switches_design_at_the_limit(operand, side, T, k, s):
    """the partial-matrix design just under the `big` test, the first design (atomics) by the launcher's own choice just over
    it; x (shifted descriptor: + (W + 1) rows) and dy (unshifted) cross independently.  "over": the guard's count alone passes
    2^30 (x: the slice still ends below 2^31 bytes); "over2g": the operand in the 4.3 GB buffer, the first design's own
    offsets past 2^31 bytes and elements"""
    o, l = ops(), lib()
    c = 16
    h, w = (H, W) if s == 1 else (2 * H - 1, 2 * W - 1)                # stride 2: dy is the 61 x 59 map
    oh, ow = o.conv_out_hw(h, w, k, s)
    if operand == "x":
        h, w = H, W
        oh, ow = o.conv_out_hw(h, w, k, s)
    xb, pat, x9 = batch(c, h, w, 51 + k + s, dtype=T)
    dyb, _, dy9 = batch(c, oh, ow, 52 + k + s, dtype=T)
    lay = sa.layout("2g" if side == "over2g" else "conv" if operand == "x" else "flat", c, side, "top" if k == 1 else "bottom")
    if operand == "x":
        buf, xv = sa.put(lay, x9, 3.0)
        dv = dy9.to(DEV).contiguous(memory_format=torch.channels_last)
    else:
        buf, dv = sa.put(lay, dy9, 3.0)
        xv = x9.to(DEV).contiguous(memory_format=torch.channels_last)
    ldx, ldy = o.geom(xv)[4], o.geom(dv)[4]
    path = sa.wgrad_path(N, h, w, c, oh, ow, c, code(T), ldx, ldy)
    assert path == (2 if side == "under" else 3)
    args = (N, h, w, c, oh, ow, c, k, s, code(T), 0)
    ws = l.query("yolo_conv2d_wgrad_ws_elems", xv.data_ptr(), ldx, dv.data_ptr(), ldy, *args)
    one_matrix = c * sa.round_up32(k * k * c)
    dense_ws = l.query("yolo_conv2d_wgrad_ws_elems", xv.data_ptr(), c, dv.data_ptr(), c, *args)
    assert dense_ws != one_matrix and ws == (dense_ws if side == "under" else one_matrix), (ws, dense_ws, one_matrix)
    dw = o.conv_wgrad(xv, dv, k, s, torch.float32)
    dw_ref, mass = sc.wgrad_ref(xb, dyb, (c, c, k, k), k, s, [pat.count(b) for b in range(3)])
    sc.assert_close(dw, dw_ref, mass, torch.float32, f"conv_wgrad k{k} s{s} {operand} in {lay}", "wgrad" if side == "under" else "wgrad_atomics")
    sa.assert_guard_channels(buf, lay, 3.0, f"conv_wgrad {lay}")


# ------------------------------------------------------------------------------------------ depthwise
@pytest.mark.parametrize("kernel,side", [("rows", "under"), ("strip", "under"), ("generic", "over")])
@pytest.mark.parametrize("operand,T", [("source", BF), ("destination", BF), ("source", HF)], ids=lambda v: str(v).replace("torch.", ""))
def test_depthwise_across_2_31_bytes(kernel, side, operand, T):
    """the limit is N*H*W*ld*2 bytes, for the source and for the destination independently"""
    o, l = ops(), lib()
    c = 16
    l.call("yolo_dw_tune_set", {"rows": 2, "strip": 1, "generic": 0}[kernel])
    if side == "under":
        want = 1 if kernel == "rows" else 2
        assert l.query("yolo_dw_plan", N, H, W, c, 0) == want and l.query("yolo_dw_plan", N, H, W, c, 12) == want
    lay = sa.layout("flat", c, side, "top" if operand == "source" else "bottom")
    dense = sa.Layout("dense", N, H, W, c, c, 0)
    slay, dlay = (lay, dense) if operand == "source" else (dense, lay)
    assert sa.dw16_takes(N, H, W, c, slay.ld, dlay.ld) == (side == "under")
    w9 = rnd((c, 9), 61, 0.3, torch.float32)
    w4, w9d = w9.view(c, 1, 3, 3), w9.to(DEV)
    bias = rnd((c,), 62, 0.5, torch.float32)
    xb, pat, x9 = batch(c, H, W, 63, dtype=T)
    what = f"{kernel} {operand} {str(T)[6:]} {lay}"
    dtc, st = code(T), stream()
    sbuf, sv = sa.put(slay, x9, 3.0)
    dbuf, dv = sa.wide_buffer(dlay, T, 5.0)
    y_ref, y_mass = sc.conv_ref(xb, w4, 3, 1, groups=c)
    # ---- forward with statistics: taken by the 16-bit kernels under the limit, "not taken" (1, nothing launched) over it
    acc = o.bn_acc_new(c, DEV)
    rc = l.query("yolo_dwconv3x3_fwd_stats", sv.data_ptr(), slay.ld, w9d.data_ptr(), dv.data_ptr(), dlay.ld, acc.data_ptr(), N, H, W, c, dtc, st)
    assert rc == (0 if side == "under" else 1), f"{what}: yolo_dwconv3x3_fwd_stats returned {rc}"
    if side == "over":
        assert bool((dv == 5.0).all()) and bool((acc == 0).all()), "the launch that was not taken wrote"
        l.call("yolo_dwconv3x3_fwd", sv.data_ptr(), slay.ld, w9d.data_ptr(), dv.data_ptr(), dlay.ld, N, H, W, c, dtc, st)
        o.bn_stats_acc(dv, acc)
    sc.assert_close(dv, y_ref, y_mass, T, f"dw_fwd {what}", "depthwise", pattern=pat)
    sc.assert_stats(acc.view(o.BN_REPL, 2, c).sum(0), dv, f"dw_fwd {what}")
    sa.assert_guard_channels(dbuf, dlay, 5.0, f"dw_fwd {what}")
    # ---- fused bias + SiLU
    dbuf.fill_(-6.0)
    rc = l.query("yolo_dwconv3x3_fwd_act", sv.data_ptr(), slay.ld, w9d.data_ptr(), bias.to(DEV).data_ptr(), dv.data_ptr(), dlay.ld, N, H, W, c, 1, dtc, st)
    assert rc == (0 if side == "under" else 1), f"{what}: yolo_dwconv3x3_fwd_act returned {rc}"
    if side == "under":
        b64 = bias.double().view(1, -1, 1, 1)
        sy, smass, e_act = sc.silu_terms(y_ref + b64, y_mass + b64.abs())
        sc.assert_close(dv, sy, smass, T, f"dw_fwd_act {what}", "depthwise", e_act=e_act, pattern=pat)
    sa.assert_guard_channels(dbuf, dlay, -6.0, f"dw_fwd_act {what}")
    # ---- data gradient, plain and accumulate (sv plays dy)
    dx_ref, dx_mass = sc.dgrad_ref(xb, w4, (3, c, H, W), 3, 1, groups=c)
    for accumulate in (0, 1):
        baseb, _, base9 = batch(c, H, W, 64, dtype=T)
        dv.copy_(base9.to(DEV))
        l.call("yolo_dwconv3x3_dgrad", sv.data_ptr(), slay.ld, w9d.data_ptr(), dv.data_ptr(), dlay.ld, N, H, W, c, accumulate, dtc, st)
        ref, mass = (dx_ref + baseb.double(), dx_mass + baseb.double().abs()) if accumulate else (dx_ref, dx_mass)
        sc.assert_close(dv, ref, mass, T, f"dw_dgrad acc={accumulate} {what}", "depthwise", pattern=pat)
        sa.assert_guard_channels(dbuf, dlay, -6.0, f"dw_dgrad {what}")
    # ---- weight gradient: x = the source slice, dy = the destination slice
    dyb, _, dy9 = batch(c, H, W, 65, dtype=T)
    dv.copy_(dy9.to(DEV))
    dw = o.dw_wgrad(sv, dv)
    dw_ref, dw_mass = sc.wgrad_ref(xb, dyb, (c, 1, 3, 3), 3, 1, [pat.count(b) for b in range(3)], groups=c)
    sc.assert_close(dw, dw_ref, dw_mass, torch.float32, f"dw_wgrad {what}", "depthwise_wgrad")
    sa.assert_guard_channels(sbuf, slay, 3.0, f"dw {what}")
    sa.assert_guard_channels(dbuf, dlay, -6.0, f"dw_wgrad {what}")


# ------------------------------------------------------------------------------------------ unguarded kernels: 4.3 GB buffers
def on2g(t, fill, where):
    lay = sa.layout_2g(t.shape[0], t.shape[2], t.shape[3], t.shape[1], where)
    return (lay,) + sa.put(lay, t, fill)


def dense(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("where", ["top", "mid"])
def test_copy_and_add_n_past_2_31_elements(where):
    o = ops()
    c = 16
    src = sm.grid((N, c, H, W), 71, BF)
    before = sm.grid((N, c, H, W), 72, BF)
    # source slice in the 4.3 GB buffer -> dense destination, plain and accumulate
    lay, sbuf, sv = on2g(src, sm.SENTINEL, where)
    dst = dense(before)
    o.copy_channels(sv, dst)
    sm.check_copy(src, before, dst, f"copy from {lay}", False)
    dst = dense(before)
    o.copy_channels(sv, dst, accumulate=True)
    sm.check_copy(src, before, dst, f"copy acc from {lay}", True)
    # add_n: one source in the big buffer, two dense
    xs = [src, before, sm.grid((N, c, H, W), 73, BF)]
    got = o.add_n([sv, dense(xs[1]), dense(xs[2])])
    sm.check_add(xs, got, f"add_n from {lay}")
    sa.assert_guard_channels(sbuf, lay, sm.SENTINEL, f"copy / add_n {lay}")
    del sbuf, sv
    torch.cuda.empty_cache()
    # dense source -> destination slice in the 4.3 GB buffer
    lay, dbuf, dv = on2g(before, sm.SENTINEL, where)
    o.copy_channels(dense(src), dv, accumulate=True)
    sm.check_copy(src, before, dv, f"copy acc into {lay}", True)
    o.copy_channels(dense(src), dv)
    sm.check_copy(src, before, dv, f"copy into {lay}", False)
    o.add_n([dense(x) for x in xs], out=dv)
    sm.check_add(xs, dv, f"add_n into {lay}")
    sa.assert_guard_channels(dbuf, lay, sm.SENTINEL, f"copy / add_n into {lay}")


def test_maxpool5_past_2_31_elements():
    o = ops()
    c = 16
    x, dout, base = sm.grid((N, c, H, W), 81, BF), sm.smooth((N, c, H, W), 82, BF), sm.smooth((N, c, H, W), 83, BF)
    lay, xbuf, xv = on2g(x, sm.SENTINEL, "top")
    out, idx = o.maxpool5_fwd(xv)
    ridx = sm.check_pool_fwd(x, out, idx.permute(0, 3, 1, 2), f"maxpool5_fwd from {lay}")
    sa.assert_guard_channels(xbuf, lay, sm.SENTINEL, f"maxpool5_fwd {lay}")
    # forward into the big buffer (reuse it: the slice becomes the output)
    out2, idx2 = o.maxpool5_fwd(dense(x), out=xv)
    sm.check_pool_fwd(x, xv, idx2.permute(0, 3, 1, 2), f"maxpool5_fwd into {lay}")
    sa.assert_guard_channels(xbuf, lay, sm.SENTINEL, f"maxpool5_fwd into {lay}")
    # backward: dout read from the big buffer; then accumulated into it
    xv.copy_(dout.to(DEV))
    dx = o.maxpool5_bwd(xv, idx)
    sm.check_pool_bwd(dout, ridx, dx, f"maxpool5_bwd from {lay}")
    xv.copy_(base.to(DEV))
    o.maxpool5_bwd(dense(dout), idx, acc_into=xv)
    sm.check_pool_bwd(dout, ridx, xv, f"maxpool5_bwd acc into {lay}", base=base)
    sa.assert_guard_channels(xbuf, lay, sm.SENTINEL, f"maxpool5_bwd {lay}")


def test_upsample2x_past_2_31_elements():
    o = ops()
    c = 16
    h, w = 31, 29
    x, dout, base = sm.grid((N, c, h, w), 91, BF), sm.smooth((N, c, 2 * h, 2 * w), 92, BF), sm.smooth((N, c, h, w), 93, BF)
    lay, xbuf, xv = on2g(x, sm.SENTINEL, "top")
    sm.check_up_fwd(x, o.upsample2x_fwd(xv), f"upsample2x_fwd from {lay}")
    xv.copy_(base.to(DEV))
    o.upsample2x_bwd(dense(dout), acc_into=xv)
    sm.check_up_bwd(dout, xv, f"upsample2x_bwd acc into {lay}", base=base)
    sa.assert_guard_channels(xbuf, lay, sm.SENTINEL, f"upsample2x {lay}")
    del xbuf, xv
    torch.cuda.empty_cache()
    lay, obuf, ov = on2g(dout, sm.SENTINEL, "bottom")
    sm.check_up_bwd(dout, o.upsample2x_bwd(ov), f"upsample2x_bwd from {lay}")
    o.upsample2x_fwd(dense(x), out=ov)
    sm.check_up_fwd(x, ov, f"upsample2x_fwd into {lay}")
    sa.assert_guard_channels(obuf, lay, sm.SENTINEL, f"upsample2x {lay}")


# ------------------------------------------------------------------------------------------ BatchNorm
def bn_both_paths(case, y, dout, out_view=None):
    """the flow of tests/test_gpu_bn.py on given device tensors (any of them a slice of a big buffer)"""
    import strict_bn as sb
    o = ops()
    c = case.shape[1]
    gamma, beta = case.gamma.to(DEV), case.beta.to(DEV)
    mom, eps, act = case.momentum, case.eps, case.act
    acc_f, acc_b = o.bn_acc_new(c, DEV), o.bn_acc_new(c, DEV)
    o.bn_stats_acc(y, acc_f)
    rm, rv = case.rmean.to(DEV), case.rvar.to(DEV)
    out, mean, invstd, scale, shift = o.bn_act_fwd_train(y, acc_f, gamma, beta, rm, rv, mom, eps, act, None, out=out_view)
    dy, dgamma, dbeta = o.bn_act_bwd_train(dout, y, scale, shift, mean, invstd, gamma, act, acc_b)
    sb.verify_accumulator_path(case, {"acc_f": acc_f, "acc_b": acc_b, "mean": mean, "invstd": invstd, "scale": scale, "shift": shift,
                                      "rmean": rm, "rvar": rv, "out": out, "dy": dy, "dgamma": dgamma, "dbeta": dbeta})
    rm, rv = case.rmean.to(DEV), case.rvar.to(DEV)
    mean, invstd, scale, shift = o.bn_train_stats(y, gamma, beta, rm, rv, mom, eps)
    r = {"mean": mean, "invstd": invstd, "scale": scale, "shift": shift, "rmean": rm, "rvar": rv,
         "out": o.bn_act_fwd(y, scale, shift, act, None, out=out_view)}
    r["dy"], r["dgamma"], r["dbeta"] = o.bn_act_bwd(dout, y, scale, shift, mean, invstd, gamma, act)
    r["dy_eval"] = o.bn_act_bwd_eval(dout, y, scale, shift, act)
    r["csum"] = o.channel_sum(dout)
    r["eval_scale"], r["eval_shift"] = o.bn_eval_coeffs(gamma, beta, rm, rv, eps)
    sb.verify_deterministic_path(case, r)


@pytest.mark.parametrize("big", ["y", "dout", "out"])
def test_batchnorm_past_2_31_elements(big):
    """statistics (accumulator and partial-row form, channel_sum), forward and both backward launches, training and eval
    form: y, dout or the forward's destination a slice of a 4.3 GB buffer; strict_bn's own limits at 32391 pixels"""
    import strict_bn as sb
    case = sb.Case("plain", N, 16, H, W, BF, 1)
    y, dout, out_view, lay, buf = dense(case.y), dense(case.dout), None, None, None
    if big == "y":
        lay, buf, y = on2g(case.y, 3.0, "top")
    elif big == "dout":
        lay, buf, dout = on2g(case.dout, 3.0, "bottom")
    else:
        lay, buf, out_view = on2g(torch.zeros_like(case.y), 3.0, "mid")
    bn_both_paths(case, y, dout, out_view)
    sa.assert_guard_channels(buf, lay, 3.0, f"batchnorm {big} in {lay}")


# ------------------------------------------------------------------------------------------ stem
def test_stem_slices_past_2_31_elements():
    """forward (+ statistics) and weight gradient with the y / dy slices in a 4.3 GB buffer; the NCHW image stays small
    (the one-pass backward: the next test)"""
    o, l = ops(), lib()
    cout, h, w = 16, 2 * H, 2 * W
    assert l.query("yolo_stem_conv_eligible", sa.F32, sa.BF16, cout) == 1
    g = torch.Generator().manual_seed(101)
    imgb = torch.randn(3, 3, h, w, generator=g)
    img = imgb[PAT].contiguous().to(DEV)
    wt = rnd((cout, 3, 3, 3), 102, 27 ** -0.5, torch.float32)
    wp = o.stem_pack_weights(wt.to(DEV), BF)
    lay = sa.layout("2g", cout, "over", "top")
    ybuf, yv = sa.wide_buffer(lay, BF, 5.0)
    acc = o.bn_acc_new(cout, DEV)
    l.call("yolo_stem_conv_fwd", img.data_ptr(), wp.data_ptr(), yv.data_ptr(), lay.ld, acc.data_ptr(), N, h, w, H, W, cout, 0, 0, sa.BF16, stream())
    sa.assert_guard_channels(ybuf, lay, 5.0, f"stem_conv_fwd {lay}")
    y_ref, y_mass = sc.conv_ref(imgb.to(BF), wt.to(BF), 3, 2)
    sc.assert_close(yv, y_ref, y_mass, BF, f"stem_conv_fwd -> {lay}", "stem", pattern=PAT)
    sc.assert_stats(acc.view(o.BN_REPL, 2, cout).sum(0), yv, f"stem_conv_fwd -> {lay}")
    # weight gradient with dy read from the slice
    dyb, _, dy9 = batch(cout, H, W, 103)
    yv.copy_(dy9.to(DEV))
    dw = o.stem_wgrad(img, yv, torch.float32)
    dw_ref, mass = sc.wgrad_ref(imgb.to(BF), dyb, (cout, 3, 3, 3), 3, 2, [PAT.count(b) for b in range(3)])
    sc.assert_close(dw, dw_ref, mass, torch.float32, f"stem_wgrad <- {lay}", "stem_wgrad")
    sa.assert_guard_channels(ybuf, lay, 5.0, f"stem_wgrad {lay}")


# ------------------------------------------------------------------------------------------ transposes, head group
def test_layout_transposes_and_head_group_past_2_31_elements():
    """nhwc_to_ncm / ncm_to_nhwc and head_group (pack and unpack) with the NHWC side a slice of a 4.3 GB buffer: exact copies"""
    o, l = ops(), lib()
    c, hw = 16, H * W
    x = sm.grid((N, c, H, W), 111, BF)
    flat = x.reshape(N, c, hw)
    lay, buf, xv = on2g(x, sm.SENTINEL, "top")
    # NHWC slice -> channels [4, 4 + c) and anchors [7, 7 + hw) of a (N, c + 8, hw + 16) prediction tensor
    preds = torch.full((N, c + 8, hw + 16), sm.SENTINEL, dtype=BF, device=DEV)
    o.head_pack(xv, preds, 4, 7)
    want = torch.full((N, c + 8, hw + 16), sm.SENTINEL, dtype=BF)
    want[:, 4:4 + c, 7:7 + hw] = flat
    sm.assert_exact(preds, want, f"nhwc_to_ncm from {lay}", "move_copy")
    got = torch.full_like(preds, sm.SENTINEL)
    o.head_group([xv], got, [4], [7], True)
    sm.assert_exact(got, want, f"head_group pack from {lay}", "move_copy")
    sa.assert_guard_channels(buf, lay, sm.SENTINEL, f"pack {lay}")
    # ... and back into the slice
    for how in ("ncm_to_nhwc", "head_group"):
        xv.fill_(0.0)
        if how == "head_group":
            o.head_group([xv], preds, [4], [7], False)
        else:
            l.call("yolo_ncm_to_nhwc", preds.data_ptr() + 4 * (hw + 16) * 2, sa.BF16, (c + 8) * (hw + 16), hw + 16, 7, xv.data_ptr(), sa.BF16,
                   lay.ld, N, c, hw, stream())
        sm.assert_exact(xv, x, f"{how} into {lay}", "move_copy")
        sa.assert_guard_channels(buf, lay, sm.SENTINEL, f"{how} into {lay}")


@pytest.mark.parametrize("big", ["dout", "y"])
def test_stem_one_pass_backward_past_2_31_elements(big):
    """yolo_stem_bn_wgrad (BatchNorm sums and weight gradient from one pass over dout, y and the image) with dout or y a slice
    of a 4.3 GB buffer, held to strict_stem_bwd's reference and limit; y and the coefficients come from the project's own
    forward, as in tests/test_gpu_stem_bwd_fused.py"""
    import strict_stem_bwd as ss
    o = ops()
    cout, act, h, w = 16, 1, 2 * H, 2 * W
    img, wt, gamma, beta, dout = ss.make_inputs(N, h, w, cout, BF, torch.float32, seed=7)
    dout = (dout.float() + 0.25).to(BF)                              # D carries the mean of dz
    imgd, gd, bd = img.to(DEV), gamma.to(DEV), beta.to(DEV)
    acc = o.bn_acc_new(cout, DEV)
    y = o.stem_conv_fwd(imgd, o.stem_pack_weights(wt.to(DEV), BF), cout, BF, acc)
    rm, rv = torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV)
    _, mean, invstd, scale, shift = o.bn_act_fwd_train(y, acc, gd, bd, rm, rv, 0.03, 1e-3, act)
    y_cpu = y.cpu()
    assert tuple(y_cpu.shape) == (N, cout, H, W)
    if big == "dout":
        lay, buf, dv = on2g(dout, 3.0, "top")
        yv = y
    else:
        lay, buf, yv = on2g(y_cpu, 3.0, "bottom")
        dv = dense(dout)
    dw, dgamma, dbeta = o.stem_bn_wgrad(imgd, dv, yv, scale, shift, mean, invstd, gd, act, torch.float32)
    sa.assert_guard_channels(buf, lay, 3.0, f"stem_bn_wgrad {big} in {lay}")
    ref = ss.reference(img, dout, y_cpu, scale.cpu(), shift.cpu(), mean.cpu(), invstd.cpu(), gamma, act)
    ss.check(dw, dgamma, dbeta, ref, f"one pass, {big} in {lay}")


# ------------------------------------------------------------------------------------------ attention
def _attn_stash(route, stash, b, t, T):
    """-> (lse (B, T, 1) or None, P (B, T, T) or None), as tests/test_gpu_kernels.py reads the stash"""
    if route != "gemm":
        return stash.view(torch.float32).reshape(b, t, 1).cpu().double(), None
    tp = (t + 31) // 32 * 32
    pm = stash.view(T).reshape(b, t, tp).cpu()
    assert not bool(pm[..., t:].any()), "stashed P: pad columns not zero"
    return None, pm[..., :t].double()


@pytest.mark.parametrize("big", ["qkv", "o_vp", "d_o_d_vp", "dqkv"])
@pytest.mark.parametrize("route,T,heads,dk,dh,t", [("fused", BF, 2, 32, 64, 400), ("gemm", HF, 3, 16, 32, 143)],
                         ids=["fused-bf16", "gemm-f16"])
def test_attention_slices_past_2_31_elements(route, T, heads, dk, dh, t, big):
    """yolo_attn_fwd / _nograd / _bwd with one group of their row-strided tensors at a time in a 4.3 GB buffer: qkv; o and vp
    (two slices of one buffer); d_o and d_vp (two slices of one buffer); dqkv.  Three images, strict_attention's bounds for o,
    the stash and dQ, dK, dV; vp must be v bit for bit."""
    import strict_attention as sat
    o, l = ops(), lib()
    n, scale, b = 3, dk ** -0.5, 3 * heads
    cq, co = heads * (2 * dk + dh), heads * dh
    qkv_cpu = sat.make_qkv(n, heads, dk, dh, t, "sharp", 120 + t, T)
    h, w = qkv_cpu.shape[2:]
    d_o, d_vp = rnd((n, co, h, w), 121, dtype=T), rnd((n, co, h, w), 122, dtype=T)
    q, k, v = sat.split_qkv(qkv_cpu, heads, dk, dh)
    st, dtc = stream(), code(T)
    bufs = []

    def place(tensor, name, where="top"):
        """dense unless this case puts the group `name` into the big buffer"""
        if big != name:
            return dense(tensor)
        lay, buf, view = on2g(tensor, 3.0, where)
        bufs.append((lay, buf))
        return view

    def pair(a_cpu, b_cpu, name):
        """two tensors of co channels: dense, or the bottom and the top slice of ONE big buffer"""
        if big != name:
            return dense(a_cpu), dense(b_cpu)
        lay, buf, va = on2g(a_cpu, 3.0, "bottom")
        top = lay.top()
        vb = buf[:, top.off:top.off + co]
        vb.copy_(b_cpu.to(DEV))
        bufs.append((sa.Layout(lay.name, lay.n, lay.h, lay.w, co, lay.ld, 0), buf, top))
        return va, vb

    def guards(what):
        for item in bufs:
            if len(item) == 2:
                sa.assert_guard_channels(item[1], item[0], 3.0, what)
            else:                                            # two slices: the guard is everything between them
                lay, buf, top = item
                sa.assert_guard_channels(buf, lay, 3.0, what, also=[(top.off, co)])

    qd = place(qkv_cpu, "qkv")
    ov, vpv = pair(torch.zeros(n, co, h, w, dtype=T), torch.zeros(n, co, h, w, dtype=T), "o_vp")
    stash = torch.empty(l.query("yolo_attn_stash_bytes_for", n, t, heads, dk, dh, dtc), dtype=torch.uint8, device=DEV)
    ws = torch.empty(l.query("yolo_attn_workspace_bytes_for", n, t, heads, dk, dh, dtc), dtype=torch.uint8, device=DEV)
    l.call("yolo_attn_fwd", qd.data_ptr(), o.geom(qd)[4], ov.data_ptr(), o.geom(ov)[4], vpv.data_ptr(), o.geom(vpv)[4], stash.data_ptr(),
           ws.data_ptr(), n, t, heads, dk, dh, float(scale), dtc, st)
    got_route = "fused" if stash.numel() == n * heads * t * 4 else "gemm"
    assert got_route == route, f"the case does not reach the {route} route: {got_route}"
    guards(f"attn_fwd {big}")
    lse, pm = _attn_stash(route, stash, b, t, T)
    o_st = sat.split(ov, heads)
    sat.check_forward(route, q, k, v, scale, T, o_st, got_lse=lse, got_p=pm, what=f"attn_fwd [{route}] {big} in the big buffer")
    assert torch.equal(sat.split(vpv, heads), v), "vp is not v bit for bit"
    if route == "fused" and big in ("qkv", "o_vp"):          # the forward with no stash: the same slices
        o2, vp2 = pair(torch.zeros(n, co, h, w, dtype=T), torch.zeros(n, co, h, w, dtype=T), "none") if big == "qkv" else (ov.zero_(), vpv.zero_())
        rc = l.query("yolo_attn_fwd_nograd", qd.data_ptr(), o.geom(qd)[4], o2.data_ptr(), o.geom(o2)[4], vp2.data_ptr(), o.geom(vp2)[4],
                     n, t, heads, dk, dh, float(scale), dtc, st)
        assert rc == 0, f"yolo_attn_fwd_nograd returned {rc}"
        guards(f"attn_fwd_nograd {big}")
        sat.check_forward("fused", q, k, v, scale, T, sat.split(o2, heads), what=f"attn_fwd_nograd {big} in the big buffer")
        assert torch.equal(sat.split(vp2, heads), v)
        if big == "o_vp":                                    # the backward below reads the o of the stashing forward
            l.call("yolo_attn_fwd", qd.data_ptr(), o.geom(qd)[4], ov.data_ptr(), o.geom(ov)[4], vpv.data_ptr(), o.geom(vpv)[4],
                   stash.data_ptr(), ws.data_ptr(), n, t, heads, dk, dh, float(scale), dtc, st)
            lse, pm = _attn_stash(route, stash, b, t, T)
            o_st = sat.split(ov, heads)
    dod, dvd = pair(d_o, d_vp, "d_o_d_vp")
    dq = place(torch.zeros_like(qkv_cpu), "dqkv", "mid")
    l.call("yolo_attn_bwd", qd.data_ptr(), o.geom(qd)[4], ov.data_ptr(), o.geom(ov)[4], dod.data_ptr(), o.geom(dod)[4], dvd.data_ptr(),
           o.geom(dvd)[4], stash.data_ptr(), ws.data_ptr(), dq.data_ptr(), o.geom(dq)[4], n, t, heads, dk, dh, float(scale), dtc, st)
    guards(f"attn_bwd {big}")
    sat.check_backward(route, q, k, v, sat.split(d_o, heads), sat.split(d_vp, heads), scale, T, *sat.split_qkv(dq, heads, dk, dh),
                       o=o_st, lse=lse, p_stash=pm, what=f"attn_bwd [{route}] {big} in the big buffer")
