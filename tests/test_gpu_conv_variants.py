"""-m gpu: element-wise parity of the conv kernels THAT THE BENCH RUNS against a float64 reference on the CPU, at the
per-element bound that the kernels' arithmetic gives (tests/strict_compare.py: half an ulp of the element + 16 * 2^-24 of
the element's mass; no tensor-wide floor).

tests/test_gpu_kernels.py covers every leaf on small maps, where the launcher always picks the narrowest tile.
Here the variants that carry the measured step are selected on purpose:
  * forced (yolo_conv_tune_set / yolo_wgrad_tune_set) on maps whose pixel count is not a multiple of any tile size, so
    the last tile is partial: every channel-tile width of the gather kernel in its register-staged and LDS-DMA forms,
    every ring tile and depth, every halo and rows variant, every weight-gradient tile; bf16 and f16; the training form
    (forward + statistics, data gradient plain / accumulate / two accumulate sources) and the fused inference epilogue
    (bias, SiLU, residual slice, output slice);
  * by the launcher's own choice on the shapes, row strides and batch size of BASELINE config 2 (preset s, 640x640,
    32 images): the calls of one real training step are recorded and each distinct one is replayed on seeded data.
Batches are built from three base images (strict_compare.image_pattern), the reference is computed for the three and
EVERY image is compared.  Every forward / data-gradient / product-path weight-gradient case is launched twice into
separately filled destinations and the two results must be bit-identical (no atomics on y / dx / dw there)."""
import os

import pytest
import torch

import strict_compare as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
HF = torch.float16


def ops():
    from src.hipops import ops as o
    return o


def lib():
    from src.hipops import lib as l
    return l


@pytest.fixture(autouse=True)
def _reset_tuning():
    torch.set_num_threads(max(1, min(32, len(os.sched_getaffinity(0)))))
    yield
    lib().call("yolo_conv_tune_set", 0, -1, -1, -1, -1, 0, 0, 0)
    lib().call("yolo_wgrad_tune_set", 0, 0, 0, 0)
    lib().call("yolo_wgrad_tune_pf", 0)
    lib().call("yolo_conv_wide_set", 2)


@pytest.fixture(autouse=True, scope="module")
def _print_observed_maxima():
    yield
    print("\n" + sc.report())


def rnd(shape, seed, scale=1.0, dtype=None):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype or BF)


def on_dev(t, ld=None, fill=3.0):
    """NCHW-shaped CPU tensor -> NHWC device tensor; with ld > C a channel slice in the middle of a wider buffer whose
    other channels hold `fill` (a kernel that strays outside its slice reads or clobbers them)."""
    o = ops()
    n, c, h, w = t.shape
    ld = c if ld is None else ld
    buf = o.new_nhwc(n, ld, h, w, t.dtype, DEV)
    buf.fill_(fill)
    off = ((ld - c) // 2) // 8 * 8
    view = buf[:, off:off + c]
    view.copy_(t.to(DEV))
    return view, buf, off


def assert_slice_untouched(buf, off, c, fill, what):
    """channels of the wider buffer outside [off, off+c) still hold the fill value"""
    outside = torch.cat([buf[:, :off], buf[:, off + c:]], 1)
    assert bool((outside.float() == fill).all()), f"{what}: wrote outside its channel slice"


def assert_same_twice(a, b, what):
    if not torch.equal(a, b):
        bad = a != b
        imgs = bad.flatten(1).any(1).nonzero().flatten().tolist()
        raise AssertionError(f"{what}: two launches on the same inputs differ in {int(bad.sum())} elements, images {imgs[:16]}")


def old_limits(ref, dtype):
    """the limit this file asserted before the derived bound (2^-8 / 2^-10 |want| + 1e-3 max|ref|): kept only as the guard
    'the new limit is nowhere wider'"""
    return dict(old_rel=2.0 ** -8 if dtype == BF else 2.0 ** -10, old_abs=1e-3 * float(ref.abs().max()))


def lib_dt(dtype):
    return lib().BF16 if dtype == BF else lib().F16


def run_fwd_dgrad_case(n, cin, cout, h, w, k, s, family="auto", dgrad_family=None, ldx=None, ldy=None, stats=True,
                       acc=(False, True), acc2=False, seed=0, want_plan=None, dtype=None):
    """forward (+ BatchNorm statistics epilogue) and data gradient (plain, accumulate, two accumulate sources) of one shape:
    every image against the float64 reference of its base image, every launch twice."""
    o = ops()
    T = dtype or BF
    dgrad_family = dgrad_family or family
    oh, ow = o.conv_out_hw(h, w, k, s)
    if want_plan is not None:
        got = lib().query("yolo_conv2d_plan", n, h, w, cin, oh, ow, cout, k, s, 0, 0, lib_dt(T))
        assert got == want_plan, f"test does not reach the variant it is written for: plan {got}, wanted {want_plan}"
    pat = sc.image_pattern(n, seed)
    nb = min(n, 3)
    xb, wt = rnd((nb, cin, h, w), seed + 1, dtype=T), rnd((cout, cin, k, k), seed + 2, (cin * k * k) ** -0.5, dtype=T)
    wp, wb = o.pack_weights(wt.float().to(DEV), k, s, 0, T), o.pack_weights(wt.float().to(DEV), k, s, 1, T)
    shape = f"{(n, cin, h, w, cout, k, s)} {str(T)[6:]}"
    # ---- forward, twice
    xd, _, _ = on_dev(xb[pat], ldx)
    outs = []
    for fill in (5.0, -6.0):
        ybuf = o.new_nhwc(n, ldy or cout, oh, ow, T, DEV).fill_(fill)
        yoff = (((ldy or cout) - cout) // 2) // 8 * 8
        acc_s = o.bn_acc_new(cout, DEV) if stats else None
        y = o.conv_fwd(xd, wp, None, cout, k, s, acc_s, out=ybuf[:, yoff:yoff + cout])
        assert_slice_untouched(ybuf, yoff, cout, fill, "conv_fwd")
        outs.append((y, acc_s))
    assert_same_twice(outs[0][0], outs[1][0], f"conv_fwd {shape}")
    y, acc_s = outs[0]
    y_ref, y_mass = sc.conv_ref(xb, wt, k, s)
    sc.assert_close(y, y_ref, y_mass, T, f"conv_fwd {shape}", family, pattern=pat, **old_limits(y_ref, T))
    if stats:
        for y_i, acc_i in outs:                      # float atomics: the two accumulators may differ, each is held to the bound
            sc.assert_stats(acc_i.view(o.BN_REPL, 2, cout).sum(0), y_i, f"conv_fwd {shape}")
    # ---- data gradient, every form twice
    if cin % 8:
        return
    dyb = rnd((nb, cout, oh, ow), seed + 3, dtype=T)
    dyd, _, _ = on_dev(dyb[pat], ldy)
    dx_ref, dx_mass = sc.dgrad_ref(dyb, wt, (nb, cin, h, w), k, s)
    forms = [("acc" if a else "plain") for a in acc] + (["acc2"] if acc2 and s == 1 else [])
    for form in forms:
        baseb, a2b = rnd((nb, cin, h, w), seed + 4, dtype=T), rnd((nb, cin, h, w), seed + 5, dtype=T)
        res = []
        for fill in (9.0, -7.0):
            if form == "plain":
                res.append(o.conv_dgrad(dyd, wb, cin, h, w, k, s))
                continue
            dxv, dxbuf, dxoff = on_dev(baseb[pat], ldx, fill=fill)
            a2v = on_dev(a2b[pat], cin + 24, fill=fill)[0] if form == "acc2" else None
            o.conv_dgrad(dyd, wb, cin, h, w, k, s, acc_into=dxv, acc2=a2v)
            assert_slice_untouched(dxbuf, dxoff, cin, fill, "conv_dgrad")
            res.append(dxv)
        assert_same_twice(res[0], res[1], f"conv_dgrad {form} {shape}")
        want, mass = dx_ref, dx_mass
        if form != "plain":
            want, mass = want + baseb.double(), mass + baseb.double().abs()
        if form == "acc2":
            want, mass = want + a2b.double(), mass + a2b.double().abs()
        sc.assert_close(res[0], want, mass, T, f"conv_dgrad {form} {shape}", dgrad_family, pattern=pat, **old_limits(want, T))


def run_fused_case(n, cin, cout, h, w, k, s, family, want_plan, dtype, seed=0):
    """the fused inference block act(conv(x) + bias) (+ residual) under the forced variant: SiLU and identity, with and
    without a residual that is a channel slice of a wider buffer, output into a channel slice; every launch twice."""
    o = ops()
    T = dtype
    oh, ow = o.conv_out_hw(h, w, k, s)
    got = lib().query("yolo_conv2d_plan", n, h, w, cin, oh, ow, cout, k, s, 0, 0, lib_dt(T))
    assert got == want_plan, f"test does not reach the variant it is written for: plan {got}, wanted {want_plan}"
    pat = sc.image_pattern(n, seed)
    nb = min(n, 3)
    xb, wt = rnd((nb, cin, h, w), seed + 1, dtype=T), rnd((cout, cin, k, k), seed + 2, (cin * k * k) ** -0.5, dtype=T)
    bias, resb = rnd((cout,), seed + 6, 0.5, torch.float32), rnd((nb, cout, oh, ow), seed + 7, dtype=T)
    wp = o.pack_weights(wt.float().to(DEV), k, s, 0, T)
    xd, _, _ = on_dev(xb[pat], cin + 32)
    resd, _, _ = on_dev(resb[pat], cout + 24, fill=2.0)
    conv, cmass = sc.conv_ref(xb, wt, k, s)
    b64 = bias.double().view(1, -1, 1, 1)
    v, vmass = conv + b64, cmass + b64.abs()
    sy, smass, e_act = sc.silu_terms(v, vmass)
    shape = f"{(n, cin, h, w, cout, k, s)} {str(T)[6:]}"
    for act in (1, 0):
        for with_res in (False, True):
            outs = []
            for fill in (5.0, -6.0):
                ybuf = o.new_nhwc(n, cout + 16, oh, ow, T, DEV).fill_(fill)
                y = o.conv_fwd_act(xd, wp, bias.to(DEV), cout, k, s, act, resd if with_res else None, out=ybuf[:, 8:8 + cout])
                assert y is not None, "no MFMA kernel took this shape"
                assert_slice_untouched(ybuf, 8, cout, fill, "conv_fwd_act")
                outs.append(y)
            what = f"conv_fwd_act act={act} res={with_res} {shape}"
            assert_same_twice(outs[0], outs[1], what)
            ref = (sy if act else v) + (resb.double() if with_res else 0.0)
            mass = (smass if act else vmass) + (resb.double().abs() if with_res else 0.0)
            # the limit asserted before: check(..., mult=2.0) of tests/test_gpu_kernels.py
            sc.assert_close(outs[0], ref, mass, T, what, family, e_act=e_act if act else None, pattern=pat,
                            old_abs={BF: 2.0 ** -6, HF: 2.0 ** -9}[T] * 2.0 * float(ref.abs().max()))


def run_wgrad_case(n, cin, cout, h, w, k, s, ldx=None, ldy=None, seed=0, family="wgrad", dtype=None, twice=True):
    """weight gradient of a batch built from three base (x, dy) pairs: dw = sum_b count_b dw(x_b, dy_b) in float64; the
    product path (partials + reduce, no atomics) launched twice must repeat bit for bit"""
    o = ops()
    T = dtype or BF
    oh, ow = o.conv_out_hw(h, w, k, s)
    pat = sc.image_pattern(n, seed)
    nb = min(n, 3)
    xb, dyb = rnd((nb, cin, h, w), seed + 5, dtype=T), rnd((nb, cout, oh, ow), seed + 6, dtype=T)
    xd, _, _ = on_dev(xb[pat], ldx)
    dyd, _, _ = on_dev(dyb[pat], ldy)
    dw = o.conv_wgrad(xd, dyd, k, s, torch.float32)
    what = f"conv_wgrad {(n, cin, h, w, cout, k, s)} {str(T)[6:]}"
    if twice:
        again = o.conv_wgrad(xd, dyd, k, s, torch.float32, out=torch.full_like(dw, 11.0))
        assert_same_twice(dw, again, what)
    dw_ref, mass = sc.wgrad_ref(xb, dyb, (cout, cin, k, k), k, s, [pat.count(b) for b in range(nb)])
    sc.assert_close(dw, dw_ref, mass, torch.float32, what, family, old_abs=3e-4 * float(dw_ref.abs().max()))


# ------------------------------------------------------------------------------------------ forced variants
# maps of 37 x 41 (1517 pixels per image: no multiple of 128, 16 or 8) so the last pixel tile of every kernel is partial;
# channel counts that are / are not multiples of the channel tile
GATHER_SHAPES = [(64, 128, 3, 1), (96, 200, 1, 1), (64, 64, 3, 2), (32, 136, 3, 1)]
RING_TILES = [(64, 128, 128), (64, 128, 64), (64, 64, 128), (64, 64, 64), (64, 128, 32),
              (32, 128, 128), (32, 128, 64), (32, 64, 128), (32, 64, 64)]
RING_SHAPES = [(64, 128, 3, 1), (96, 200, 1, 1), (64, 64, 3, 2), (160, 136, 3, 1), (128, 72, 3, 2)]
RING_TILE_DEPTH = [t + (2 + i % 3,) for i, t in enumerate(RING_TILES)]          # a representative ring depth per tile
DTYPES = [pytest.param(BF, id="bf16"), pytest.param(HF, id="f16")]


def ring_plan(bm, bn):
    return 3000 + (500 if bm == 64 else 0) + bn


def rows_plan(force, cout):
    return 4000 + {6: 1, 7: 2 if cout > 64 else 1, 8: 3, 12: 4, 14: 6, 16: 7}[force]


@pytest.mark.parametrize("bn", [32, 64, 128])
@pytest.mark.parametrize("dma", [0, 1])
@pytest.mark.parametrize("cin,cout,k,s", GATHER_SHAPES)
def test_gather_kernel_every_tile_width_and_staging_mode(bn, dma, cin, cout, k, s):
    lib().call("yolo_conv_tune_set", bn, -1, 0, dma, 0, 0, 0, 0)
    run_fwd_dgrad_case(3, cin, cout, 37, 41, k, s, "gather", ldx=cin + 32, ldy=cout + 16, want_plan=1000 + bn, acc2=True,
                       seed=bn + dma)


@pytest.mark.parametrize("bn", [32, 64, 128])
@pytest.mark.parametrize("dma", [0, 1])
@pytest.mark.parametrize("cin,cout,k,s", GATHER_SHAPES[:3])
def test_gather_kernel_f16(bn, dma, cin, cout, k, s):
    """the f16 instantiations (config 5 runs in f16), at f16's own ulp"""
    lib().call("yolo_conv_tune_set", bn, -1, 0, dma, 0, 0, 0, 0)
    run_fwd_dgrad_case(3, cin, cout, 37, 41, k, s, "gather", ldx=cin + 32, ldy=cout + 16, want_plan=1000 + bn, acc2=True,
                       seed=bn + dma + 1, dtype=HF)


@pytest.mark.parametrize("bn", [64, 128])
def test_gather_kernel_tap_inner_order(bn):
    lib().call("yolo_conv_tune_set", bn, 1, 0, 1, 0, 0, 0, 0)
    run_fwd_dgrad_case(2, 64, 128, 23, 29, 3, 1, "gather", want_plan=1000 + bn, acc2=True, seed=7)


@pytest.mark.parametrize("bk,bm,bn", RING_TILES)
@pytest.mark.parametrize("nst", [2, 3, 4])
@pytest.mark.parametrize("cin,cout,k,s", RING_SHAPES)
def test_ring_kernel_every_tile_and_depth(bk, bm, bn, nst, cin, cout, k, s):
    """The pipelined ring kernel: every tile shape and K-step at every ring depth; channel counts that are not multiples
    of the 64-deep K-step (96, 160: partial last chunk step) or of the channel tile (200, 136, 72); stride-2 data
    gradients (four parity classes in one launch, odd map: the classes differ in size); partial last pixel tile."""
    lib().call("yolo_conv_tune_set", bn, -1, 0, -1, 1, bm, nst, bk)
    run_fwd_dgrad_case(3, cin, cout, 37, 41, k, s, "ring", ldx=cin + 32, ldy=cout + 16, want_plan=ring_plan(bm, bn), acc2=True,
                       seed=bm + bn + nst)


@pytest.mark.parametrize("bk,bm,bn,nst", RING_TILE_DEPTH)
@pytest.mark.parametrize("cin,cout,k,s", [RING_SHAPES[1], RING_SHAPES[3], RING_SHAPES[4]])
def test_ring_kernel_f16(bk, bm, bn, nst, cin, cout, k, s):
    lib().call("yolo_conv_tune_set", bn, -1, 0, -1, 1, bm, nst, bk)
    run_fwd_dgrad_case(3, cin, cout, 37, 41, k, s, "ring", ldx=cin + 32, ldy=cout + 16, want_plan=ring_plan(bm, bn), acc2=True,
                       seed=bm + bn + nst + 1, dtype=HF)


@pytest.mark.parametrize("variant", [1, 2, 3, 4])
@pytest.mark.parametrize("cin,cout", [(64, 128), (32, 64), (96, 192)])
def test_halo_kernel_every_variant(variant, cin, cout):
    lib().call("yolo_conv_tune_set", 0, -1, variant, -1, -1, 0, 0, 0)
    run_fwd_dgrad_case(3, cin, cout, 37, 41, 3, 1, "halo", ldx=cin + 32, ldy=cout + 16, want_plan=2000 + variant, acc2=True,
                       seed=variant)


@pytest.mark.parametrize("variant", [1, 2, 3, 4])
@pytest.mark.parametrize("cin,cout", [(64, 128), (96, 192)])
def test_halo_kernel_f16(variant, cin, cout):
    lib().call("yolo_conv_tune_set", 0, -1, variant, -1, -1, 0, 0, 0)
    run_fwd_dgrad_case(3, cin, cout, 37, 41, 3, 1, "halo", ldx=cin + 32, ldy=cout + 16, want_plan=2000 + variant, acc2=True,
                       seed=variant + 1, dtype=HF)


@pytest.mark.parametrize("force", [6, 7, 8, 12])
@pytest.mark.parametrize("cin,cout,h,w", [(64, 128, 23, 20), (32, 64, 13, 40), (96, 200, 9, 20), (128, 72, 20, 40)])
def test_rows_kernel_both_tiles_on_narrow_maps(force, cin, cout, h, w):
    """conv_rows.hip: 20- and 40-pixel-wide maps whose height is no multiple of the 4- / 2-row block, channel counts
    that do not fill the last channel tile"""
    lib().call("yolo_conv_tune_set", 0, -1, force, -1, -1, 0, 0, 0)
    run_fwd_dgrad_case(3, cin, cout, h, w, 3, 1, "rows", ldx=cin + 32, ldy=cout + 16, want_plan=rows_plan(force, cout), acc2=True,
                       seed=force)


@pytest.mark.parametrize("cin,cout,h,w", [(64, 136, 23, 37), (32, 64, 10, 16), (96, 64, 31, 80)])
def test_rows_kernel_16_pixel_wide_blocks(cin, cout, h, w):
    """conv_rows.hip with 10 x 16-pixel blocks on maps of any size: partial blocks in both directions"""
    lib().call("yolo_conv_tune_set", 0, -1, 14, -1, -1, 0, 0, 0)
    run_fwd_dgrad_case(3, cin, cout, h, w, 3, 1, "rows", ldx=cin + 32, ldy=cout + 16, want_plan=4006, acc2=True, seed=cin)


@pytest.mark.parametrize("cin,cout,h,w", [(16, 32, 23, 37), (32, 16, 41, 16), (64, 24, 20, 33), (16, 16, 7, 50)])
def test_rows_kernel_narrow_layers(cin, cout, h, w):
    """conv_rows.hip, 20 x 16-pixel blocks x 32 channels: fewer than 64 destination channels, 16-channel sources (half a chunk)"""
    lib().call("yolo_conv_tune_set", 0, -1, 16, -1, -1, 0, 0, 0)
    run_fwd_dgrad_case(3, cin, cout, h, w, 3, 1, "rows", ldx=cin + 32, ldy=cout + 16, want_plan=4007, acc2=True, seed=cin + cout)


@pytest.mark.parametrize("force,cin,cout,h,w,plan", [(8, 64, 128, 23, 20, 4003), (12, 96, 72, 13, 40, 4004), (14, 64, 64, 23, 37, 4006)])
def test_rows_kernel_f16(force, cin, cout, h, w, plan):
    """the f16 instantiations of conv_rows.hip (config 5 trains in f16), at f16's own ulp"""
    lib().call("yolo_conv_tune_set", 0, -1, force, -1, -1, 0, 0, 0)
    run_fwd_dgrad_case(3, cin, cout, h, w, 3, 1, "rows", ldx=cin + 32, ldy=cout + 16, want_plan=plan, acc2=True, seed=force,
                       dtype=HF)


# ---- the statistics epilogue ADDS into its accumulator and stays inside it.  assert_stats on a zeroed accumulator of its
# own cannot tell an overwrite from an add, nor see a write past the [8][2][cout] slice.  cout 72: a partial second channel
# tile; 7 x 11 / 9 x 20 maps: a partial last pixel tile.  (tune arguments of yolo_conv_tune_set, h, w, plan)
STATS_ADD_CASES = [
    pytest.param((32, -1, 0, 0, 0, 0, 0, 0), 7, 11, 1032, id="gather-bn32-registers"),
    pytest.param((32, -1, 0, 1, 0, 0, 0, 0), 7, 11, 1032, id="gather-bn32-dma"),
    pytest.param((128, -1, 0, 0, 0, 0, 0, 0), 7, 11, 1128, id="gather-bn128-registers"),
    pytest.param((128, -1, 0, 1, 0, 0, 0, 0), 7, 11, 1128, id="gather-bn128-dma"),
    pytest.param((64, -1, 0, -1, 1, 64, 3, 64), 7, 11, ring_plan(64, 64), id="ring-64x64"),
    pytest.param((128, -1, 0, -1, 1, 128, 2, 64), 7, 11, ring_plan(128, 128), id="ring-128x128"),
    pytest.param((0, -1, 1, -1, -1, 0, 0, 0), 7, 11, 2001, id="halo-1"),
    pytest.param((0, -1, 4, -1, -1, 0, 0, 0), 7, 11, 2004, id="halo-4"),
    pytest.param((0, -1, 6, -1, -1, 0, 0, 0), 9, 20, rows_plan(6, 72), id="rows-full-row"),
    pytest.param((0, -1, 14, -1, -1, 0, 0, 0), 7, 11, rows_plan(14, 72), id="rows-16-wide"),
    pytest.param(None, 18, 22, None, id="stem"),
]
STATS_GUARD, STATS_SENTINEL, STATS_PREFILL = 64, -777.25, 0.5


@pytest.mark.parametrize("tune,h,w,plan", STATS_ADD_CASES)
def test_statistics_epilogue_adds_into_its_slice_only(tune, h, w, plan):
    """One forward with statistics per kernel family; the accumulator is a [8][2][cout] slice, pre-filled with 0.5, of a
    larger fp32 buffer whose guard regions on both sides hold a sentinel.  The guards must come back bit-unchanged, and the
    sum over the replicas minus 8 * 0.5 must be the sums of the stored y at assert_stats' bound (2e-5 of the mass)."""
    o = ops()
    if tune is None:                                 # the fused stem: fp32 NCHW image, 3 -> 32
        cout = 32
        img = rnd((2, 3, h, w), 41, dtype=torch.float32).to(DEV)
        assert o.stem_conv_eligible(img, BF, cout)
        wp = o.stem_pack_weights(rnd((cout, 3, 3, 3), 42, 0.2, torch.float32).to(DEV), BF)
        run = lambda acc: o.stem_conv_fwd(img, wp, cout, BF, acc)
    else:
        cin, cout = 64, 72
        lib().call("yolo_conv_tune_set", *tune)
        got = lib().query("yolo_conv2d_plan", 2, h, w, cin, h, w, cout, 3, 1, 0, 0, lib().BF16)
        assert got == plan, f"test does not reach the variant it is written for: plan {got}, wanted {plan}"
        xd, _, _ = on_dev(rnd((2, cin, h, w), 43))
        wp = o.pack_weights(rnd((cout, cin, 3, 3), 44, (cin * 9) ** -0.5).float().to(DEV), 3, 1, 0, BF)
        run = lambda acc: o.conv_fwd(xd, wp, None, cout, 3, 1, acc)
    n_acc = o.BN_REPL * 2 * cout
    buf = torch.full((STATS_GUARD + n_acc + STATS_GUARD,), STATS_SENTINEL, dtype=torch.float32, device=DEV)
    acc = buf[STATS_GUARD:STATS_GUARD + n_acc]
    acc.fill_(STATS_PREFILL)
    y = run(acc)
    guards = torch.cat([buf[:STATS_GUARD], buf[STATS_GUARD + n_acc:]]).cpu()
    assert torch.equal(guards.view(torch.int32), torch.full_like(guards, STATS_SENTINEL).view(torch.int32)), \
        "the statistics epilogue wrote outside its [8][2][cout] accumulator"
    added = acc.double().view(o.BN_REPL, 2, cout).sum(0) - o.BN_REPL * STATS_PREFILL
    sc.assert_stats(added, y, f"statistics added to a pre-filled accumulator, {h}x{w} plan {plan}")


# ---- the fused inference epilogue (bias, SiLU, residual) under every forced forward variant, bf16 and f16 (config 5 runs
# exactly these instantiations; yolo_conv2d_fwd_act goes through the same launcher, so yolo_conv_tune_set steers it)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bn", [32, 64, 128])
@pytest.mark.parametrize("dma", [0, 1])
@pytest.mark.parametrize("cin,cout,k,s", GATHER_SHAPES[:3])
def test_fused_inference_epilogue_gather_kernel(bn, dma, cin, cout, k, s, dtype):
    lib().call("yolo_conv_tune_set", bn, -1, 0, dma, 0, 0, 0, 0)
    run_fused_case(3, cin, cout, 37, 41, k, s, "gather", 1000 + bn, dtype, seed=bn + dma)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bk,bm,bn,nst", RING_TILE_DEPTH)
@pytest.mark.parametrize("cin,cout,k,s", [RING_SHAPES[1], RING_SHAPES[3], RING_SHAPES[4]])
def test_fused_inference_epilogue_ring_kernel(bk, bm, bn, nst, cin, cout, k, s, dtype):
    lib().call("yolo_conv_tune_set", bn, -1, 0, -1, 1, bm, nst, bk)
    run_fused_case(3, cin, cout, 37, 41, k, s, "ring", ring_plan(bm, bn), dtype, seed=bm + bn + nst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", [1, 2, 3, 4])
@pytest.mark.parametrize("cin,cout", [(64, 128), (96, 192)])
def test_fused_inference_epilogue_halo_kernel(variant, cin, cout, dtype):
    lib().call("yolo_conv_tune_set", 0, -1, variant, -1, -1, 0, 0, 0)
    run_fused_case(3, cin, cout, 37, 41, 3, 1, "halo", 2000 + variant, dtype, seed=variant)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("force,cin,cout,h,w", [(6, 64, 128, 23, 20), (7, 96, 200, 9, 20), (7, 32, 64, 13, 40), (8, 64, 128, 23, 20),
                                                (12, 128, 72, 20, 40), (14, 64, 136, 23, 37), (16, 64, 24, 20, 33), (16, 16, 32, 23, 37)])
def test_fused_inference_epilogue_rows_kernel(force, cin, cout, h, w, dtype):
    lib().call("yolo_conv_tune_set", 0, -1, force, -1, -1, 0, 0, 0)
    run_fused_case(3, cin, cout, h, w, 3, 1, "rows", rows_plan(force, cout), dtype, seed=force)


def test_stride2_dgrad_patch_kernel_f16():
    q = lib().query
    got = [q("yolo_conv2d_plan", 3, 84, 100, 72, 42, 50, 96, 3, 2, 1, c, lib().F16) for c in range(4)]
    assert all(g == 5008 for g in got), got
    run_fwd_dgrad_case(3, 72, 96, 84, 100, 3, 2, "auto", "patch", ldx=72 + 32, ldy=96 + 16, stats=False, seed=5, dtype=HF)


@pytest.mark.parametrize("pf", [1, 4])          # patches in flight: the big-layer and the small-layer variant of k_wgrad2
@pytest.mark.parametrize("to,ti", [(1, 1), (1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize("k,s", [(3, 1), (3, 2)])
def test_wgrad_3x3_every_tile(to, ti, k, s, pf):
    lib().call("yolo_wgrad_tune_set", to, ti, 0, 0)
    lib().call("yolo_wgrad_tune_pf", pf)
    assert lib().query("yolo_conv2d_wgrad_plan", 3, 37, 41, 72, *ops().conv_out_hw(37, 41, k, s), 88, k, s, lib().BF16) // 10000000 == pf
    run_wgrad_case(3, 72, 88, 37, 41, k, s, ldx=104, ldy=96, seed=to * 4 + ti)
    if pf == 4:         # a slab of 1, 2, 3, 5 patches: the prefetch ring's prologue / tail shorter than its depth
        for blocks in (4000, 700):
            lib().call("yolo_wgrad_tune_set", to, ti, blocks, 1)
            run_wgrad_case(2, 72, 88, 19, 23, k, s, ldx=104, ldy=96, seed=to * 4 + ti + blocks)


@pytest.mark.parametrize("pf", [1, 4])
@pytest.mark.parametrize("to", [1, 2, 3, 4])
@pytest.mark.parametrize("ti", [1, 2, 3, 4])
def test_wgrad_1x1_every_tile(to, ti, pf):
    lib().call("yolo_wgrad_tune_set", to, ti, 0, 0)
    lib().call("yolo_wgrad_tune_pf", pf)
    run_wgrad_case(3, 136, 120, 37, 41, 1, 1, ldx=160, ldy=128, seed=to * 4 + ti)


@pytest.mark.parametrize("cin,cout,k,s", [(72, 88, 3, 1), (72, 88, 3, 2), (136, 120, 1, 1)])
def test_wgrad_first_mfma_design_with_atomics(cin, cout, k, s, monkeypatch):
    """algo 3 (conv_generic.hip: wgrad_path): the first MFMA weight-gradient design, float atomics into one matrix -- the
    automatic route for tensors of 2^30 elements and more (reached by size, by the launcher's own choice, in
    tests/test_gpu_addressing.py; here it is forced on small maps with partial tiles).  Held to the same bound; no
    bit-equality of two launches (atomics)."""
    monkeypatch.setattr(ops(), "ALGO", 3)
    assert lib().query("yolo_conv2d_wgrad_plan", 3, 37, 41, cin, *ops().conv_out_hw(37, 41, k, s), cout, k, s, lib().BF16) > 0   # MFMA-eligible: algo 3 takes the first design
    run_wgrad_case(3, cin, cout, 37, 41, k, s, ldx=cin + 32, ldy=cout + 8, seed=cin, family="wgrad_atomics", twice=False)


# ------------------------------------------------------------------------------------------ the bench's own calls
def _record_step_calls(cfg, n, res):
    """One real bf16 training step of the model; -> distinct dense-conv calls as the launcher saw them."""
    from oracle import blocks as ob
    from oracle.params import det_fill_
    from src.model.losses import YoloDFLQFLoss
    from src.model.model_builder import Model
    o = ops()
    calls = {"fwd": set(), "dgrad": set(), "wgrad": set()}
    real = (o.conv_fwd, o.conv_dgrad, o.conv_wgrad)

    def fwd(x, wp, bias, cout, k, stride, stats_acc=None, out=None):
        y = real[0](x, wp, bias, cout, k, stride, stats_acc, out)
        nn, cin, h, w, ldx = o.geom(x)
        calls["fwd"].add((nn, cin, cout, h, w, k, stride, ldx, o.geom(y)[4], stats_acc is not None))
        return y

    def dgrad(dy, wb, cin, h, w, k, stride, acc_into=None, acc2=None):
        dx = real[1](dy, wb, cin, h, w, k, stride, acc_into, acc2)
        nn, cout, _, _, lddy = o.geom(dy)
        calls["dgrad"].add((nn, cin, cout, h, w, k, stride, o.geom(dx)[4], lddy, acc_into is not None))
        return dx

    def wgrad(x, dy, k, stride, w_dtype, out=None):
        nn, cin, h, w, ldx = o.geom(x)
        calls["wgrad"].add((nn, cin, dy.shape[1], h, w, k, stride, ldx, o.geom(dy)[4]))
        return real[2](x, dy, k, stride, w_dtype, out)

    o.conv_fwd, o.conv_dgrad, o.conv_wgrad = fwd, dgrad, wgrad
    try:
        model = Model(**ob.PRESETS[cfg], num_classes=80)
        det_fill_(model.state_dict(), 1)
        model = model.cuda().train()
        g = torch.Generator().manual_seed(3)
        img = torch.randn(n, 3, res, res, generator=g).cuda()
        gts = [torch.tensor([[res * 0.5, res * 0.4, res * 0.2, res * 0.1, 4.]]).cuda() for _ in range(n)]
        with torch.autocast("cuda", dtype=BF):
            preds, a, st = model(img)
            loss, _ = YoloDFLQFLoss(num_classes=80)(preds, gts, a, st)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        o.conv_fwd, o.conv_dgrad, o.conv_wgrad = real
    return calls


FAMILY = {1: "gather", 2: "halo", 3: "ring", 4: "rows", 5: "patch"}        # plan // 1000 -> kernel family


@pytest.fixture(scope="module")
def config2_calls():
    return _record_step_calls("s", 32, 640)


def test_config2_forward_and_dgrad_calls_elementwise(config2_calls):
    """Every distinct forward / data-gradient call of preset s @640, 32 images, replayed with the recorded strides and
    the launcher's own variant choice; all 32 images against the float64 reference of their base image."""
    q = lib().query
    plans, failures = {}, []
    shapes = {}
    for (n, cin, cout, h, w, k, s, ldx, ldy, st) in sorted(config2_calls["fwd"]):
        shapes.setdefault((n, cin, cout, h, w, k, s), [ldx, ldy, st, False])
    for (n, cin, cout, h, w, k, s, lddx, lddy, acc) in sorted(config2_calls["dgrad"]):
        e = shapes.setdefault((n, cin, cout, h, w, k, s), [lddx, lddy, False, acc])
        e[3] = e[3] or acc
    assert len(shapes) >= 20
    for (n, cin, cout, h, w, k, s), (ldx, ldy, st, acc) in shapes.items():
        if cin < 8:
            continue                                     # the 3-channel stem has its own kernels and tests
        oh, ow = ops().conv_out_hw(h, w, k, s)
        p = q("yolo_conv2d_plan", n, h, w, cin, oh, ow, cout, k, s, 0, 0, lib().BF16)
        plans[p] = plans.get(p, 0) + 1
        pd = q("yolo_conv2d_plan", n, h, w, cin, oh, ow, cout, k, s, 1, 0, lib().BF16)
        try:
            run_fwd_dgrad_case(n, cin, cout, h, w, k, s, FAMILY.get(p // 1000, "auto"), FAMILY.get(pd // 1000, "auto"), ldx=ldx, ldy=ldy,
                               stats=st, acc=(False, True) if acc else (False,), seed=cin + cout)
        except AssertionError as e:
            failures.append(str(e))
    print(f"\n[config-2 conv calls] {len(shapes)} distinct shapes, forward plans (kind*1000+width -> count): {plans}")
    assert not failures, "\n".join(failures)
    # the step must have exercised the wide tiles and the halo kernel (what the bench's time is made of)
    assert any(p // 1000 == 3 for p in plans) and any(p // 1000 == 2 for p in plans), plans


def test_config2_wide_and_narrow_epilogue_stores_are_bit_identical_on_every_image(config2_calls):
    """The 16-byte epilogue (store_pixel_blocks: a lane-pair exchange -- by v_permlane16_swap, the default, or by ds_bpermute --
    then one 16-byte store) against the 8-byte form over the WHOLE output of every distinct forward / data-gradient call of
    preset s @640 at 32 images: same values, only the exchange and store instructions differ, so the three must be
    bit-identical on all 32 images, accumulate forms included.  (This all-image test is what found the ring race of round 3 -- a whole workgroup tile of the stride-2
    patch kernel short of one product in images those tests do not look at: DESIGN section 6.)"""
    o, q = ops(), lib().query
    failures, plans = [], {}
    cases = [("fwd",) + c[:9] + (False,) for c in sorted(config2_calls["fwd"])] + [("dgrad",) + c for c in sorted(config2_calls["dgrad"])]
    seen = set()
    for kind, n, cin, cout, h, w, k, s, ld_a, ld_b, acc in cases:
        if cin < 8 or cin % 8 or (kind, n, cin, cout, h, w, k, s, ld_a, ld_b, acc) in seen:
            continue
        seen.add((kind, n, cin, cout, h, w, k, s, ld_a, ld_b, acc))
        oh, ow = o.conv_out_hw(h, w, k, s)
        plan = q("yolo_conv2d_plan", n, h, w, cin, oh, ow, cout, k, s, 1 if kind == "dgrad" else 0, 0, lib().BF16)
        wt = rnd((cout, cin, k, k), 3, (cin * k * k) ** -0.5).float().to(DEV)
        if kind == "fwd":
            src, _, _ = on_dev(rnd((n, cin, h, w), 1), ld_a)
            wp = o.pack_weights(wt, k, s, 0, BF)
            run = lambda out: o.conv_fwd(src, wp, None, cout, k, s, None, out=out)
            shape, ld_out = (n, cout, oh, ow), ld_b
        else:
            src, _, _ = on_dev(rnd((n, cout, oh, ow), 1), ld_b)
            wb = o.pack_weights(wt, k, s, 1, BF)
            run = lambda out: o.conv_dgrad(src, wb, cin, h, w, k, s, acc_into=out if acc else None) if acc else _dgrad_into(o, src, wb, cin, h, w, k, s, out)
            shape, ld_out = (n, cin, h, w), ld_a
        outs = []
        for wide in (2, 1, 0):              # exchange by v_permlane16_swap (default) / by ds_bpermute / 8-byte stores
            lib().call("yolo_conv_wide_set", wide)
            base = rnd(shape, 5)
            dst, _, _ = on_dev(base, ld_out)
            r = run(dst)
            outs.append((r if r is not None else dst).clone())
        lib().call("yolo_conv_wide_set", 2)
        plans[plan // 1000] = plans.get(plan // 1000, 0) + 1
        for name, other in (("permlane vs 8-byte", outs[2]), ("permlane vs bpermute", outs[1])):
            if not torch.equal(outs[0], other):
                bad = (outs[0] != other)
                imgs = bad.flatten(1).any(1).nonzero().flatten().tolist()
                failures.append(f"{kind} {(n, cin, cout, h, w, k, s)} acc={acc} plan {plan} ({name}): {int(bad.sum())} elements differ, images {imgs[:8]}")
    print(f"\n[wide vs narrow stores] {len(seen)} calls, kernel kinds (plan // 1000 -> count): {plans}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("wide", [1, 2, 0])
def test_stride2_patch_kernel_repeats_bit_for_bit_on_every_image(wide):
    """Regression for round 3's ring race (conv_stage.h: dma_wait): the 128 -> 128 3x3 / 2 data gradient @160x160 at 32 images,
    the launch in which whole workgroup tiles used to come out one product short in a few runs of a hundred (with the
    ds_bpermute epilogue, wide = 1, within a dozen).  Twelve launches, every image, each compared bit for bit with the first;
    the first against the 8-byte-store form."""
    o = ops()
    n, c, h, w = 32, 128, 160, 160
    dy, _, _ = on_dev(rnd((n, c, h // 2, w // 2), 61))
    wt = rnd((c, c, 3, 3), 62, (c * 9) ** -0.5).float().to(DEV)
    wb = o.pack_weights(wt, 3, 2, 1, BF)
    lib().call("yolo_conv_wide_set", 0)
    ref = o.conv_dgrad(dy, wb, c, h, w, 3, 2).clone()
    lib().call("yolo_conv_wide_set", wide)
    side = torch.cuda.Stream()
    a, b = torch.empty(32 << 20, device=DEV), torch.empty(32 << 20, device=DEV)
    for rep in range(12):
        with torch.cuda.stream(side):           # a bandwidth-hungry neighbour, as in the training step
            b.copy_(a)
        got = o.conv_dgrad(dy, wb, c, h, w, 3, 2)
        if not torch.equal(got, ref):
            bad = got != ref
            imgs = bad.flatten(1).any(1).nonzero().flatten().tolist()
            raise AssertionError(f"launch {rep}: {int(bad.sum())} elements differ from the 8-byte form, images {imgs}")
    torch.cuda.synchronize()


def _dgrad_into(o, src, wb, cin, h, w, k, s, out):
    """plain (non-accumulating) data gradient; the result tensor is the kernel's own allocation"""
    return o.conv_dgrad(src, wb, cin, h, w, k, s)


def test_config2_weight_gradient_calls_elementwise(config2_calls):
    """Every distinct weight-gradient call of preset s @640 at the full 32 images (the slab plan depends on the batch),
    x and dy built from three base images by the same pattern."""
    q = lib().query
    failures, plans = [], set()
    calls = sorted(config2_calls["wgrad"])
    assert len(calls) >= 20
    for (n, cin, cout, h, w, k, s, ldx, ldy) in calls:
        if cin % 8:
            continue
        oh, ow = ops().conv_out_hw(h, w, k, s)
        plans.add(q("yolo_conv2d_wgrad_plan", n, h, w, cin, oh, ow, cout, k, s, lib().BF16))
        try:
            run_wgrad_case(n, cin, cout, h, w, k, s, ldx=ldx, ldy=ldy, seed=cin * 3 + cout)
        except AssertionError as e:
            failures.append(str(e))
    print(f"\n[config-2 wgrad calls] {len(calls)} distinct calls, {len(plans)} distinct plans")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("cin,cout,variant", [(32, 64, 16), (72, 96, 8), (128, 32, 8), (40, 64, 8)])
def test_stride2_dgrad_patch_kernel(cin, cout, variant):
    """conv_up2.hip: all four parity classes from one staged dy patch; dy grid 42 x 50 (no multiple of the 8- / 16-row and
    16-column tiles), dx channel counts that do not fill the last 64-channel tile, channel slices of wider buffers,
    accumulate on and off"""
    q = lib().query
    got = [q("yolo_conv2d_plan", 3, 84, 100, cin, 42, 50, cout, 3, 2, 1, c, lib().BF16) for c in range(4)]
    assert all(g == 5000 + variant for g in got), got
    run_fwd_dgrad_case(3, cin, cout, 84, 100, 3, 2, "auto", "patch", ldx=cin + 32, ldy=cout + 16, stats=False, seed=cin + cout)


def test_stride2_dgrad_real_shape_all_parity_classes():
    """128 -> 128 3x3 stride 2 on a 160 x 160 map, 32 images (the biggest conv of preset s): four parity-class launches."""
    q = lib().query
    got = [q("yolo_conv2d_plan", 32, 160, 160, 128, 80, 80, 128, 3, 2, 1, c, lib().BF16) for c in range(4)]
    assert all(g == 5008 for g in got), got                 # conv_up2.hip: the dy patch once for all four classes
    run_fwd_dgrad_case(32, 128, 128, 160, 160, 3, 2, "auto", "patch", stats=True, acc=(False, True), seed=77)
    # the same layer on a 40 x 40 map (dy grid 20 x 20: partial tiles in both directions)
    got = [q("yolo_conv2d_plan", 32, 40, 40, 256, 20, 20, 256, 3, 2, 1, c, lib().BF16) for c in range(4)]
    assert all(g == 5008 for g in got), got
    run_fwd_dgrad_case(32, 256, 256, 40, 40, 3, 2, "auto", "patch", stats=True, acc=(False, True), seed=79)
    # odd map: the parity classes have different sizes
    run_fwd_dgrad_case(2, 64, 64, 45, 39, 3, 2, "auto", stats=False, seed=78)
