"""No GPU: the 32-bit addressing contract (tests/strict_addressing.py, restated from the documented rule) against the host-only
queries of the library on either side of every limit, the argument-range checker on made-up prototypes, and the wrap mutants
on a scaled-down copy of every layout tests/test_gpu_addressing.py uses.

The queries (yolo_conv2d_plan, yolo_conv2d_wgrad_plan, yolo_conv2d_wgrad_ws_elems, yolo_dw_plan, yolo_stem_conv_eligible)
call nothing in the HIP runtime; pointer arguments are looked at for alignment only and are dummy 16-byte aligned integers."""
import ctypes

import numpy as np
import pytest
import torch

import strict_addressing as sa
import strict_compare as sc
from src.hipops import lib

PTR = 1 << 20                      # a 16-byte aligned "pointer" (alignment is all the queries look at)
DEFAULT_TUNE = (0, -1, -1, -1, -1, 0, 0, 0)
INT_MAX = (1 << 31) - 1


@pytest.fixture(autouse=True)
def _default_tune():
    lib.call("yolo_conv_tune_set", *DEFAULT_TUNE)
    lib.call("yolo_dw_tune_set", 0)
    yield
    lib.call("yolo_conv_tune_set", *DEFAULT_TUNE)


def plan(mode, n, h, w, cin, cout, k, s, cls, dtype):
    oh, ow = sa.conv_out_hw(h, w, k, s)
    args = (n, h, w, cin, oh, ow, cout, k, s, mode, cls, dtype)
    assert all(0 <= a <= INT_MAX for a in args), args          # nothing is truncated on the way through ctypes
    sa.check_args("yolo_conv2d_plan", lib._protos, args)
    return lib.query("yolo_conv2d_plan", *args)


# (H, W, Cin, Cout, k, s, dtype): maps from 8x8 to 640x640, one-tap and nine-tap, both strides, both 16-bit types, channel
# counts that are / are not multiples of 32 (ring, up2 and halo want 32)
CONV_SWEEP = [(640, 640, 64, 64, 3, 1, sa.BF16), (640, 640, 64, 128, 1, 1, sa.F16), (320, 320, 32, 64, 3, 2, sa.BF16),
              (160, 160, 128, 128, 3, 2, sa.F16), (80, 80, 256, 256, 3, 1, sa.BF16), (61, 59, 64, 64, 3, 1, sa.BF16),
              (37, 41, 96, 200, 1, 1, sa.BF16), (8, 8, 8, 8, 3, 1, sa.F16), (122, 118, 64, 64, 3, 2, sa.BF16),
              (40, 40, 512, 512, 3, 1, sa.BF16), (20, 20, 1024, 256, 1, 1, sa.F16), (193, 7, 24, 40, 3, 2, sa.BF16)]
LAUNCHES = [(0, 0), (1, 0), (1, 1), (1, 2), (1, 3)]            # (mode, parity class)


@pytest.mark.parametrize("h,w,cin,cout,k,s,dtype", CONV_SWEEP)
def test_conv_plan_names_a_fast_family_exactly_up_to_the_limit(h, w, cin, cout, k, s, dtype):
    lib.load()
    for mode, cls in LAUNCHES:
        if cls and not (mode == 1 and s == 2):
            continue
        oh, ow = sa.conv_out_hw(h, w, k, s)

        def fast(n):
            # a stride-2 data gradient is planned per class; the launcher's joint launches need every class eligible, which
            # only ever narrows towards the same limit (all four classes share the source descriptor)
            return sa.conv_plan_is_fast(mode, n, h, w, cin, oh, ow, cout, k, s, cls, dtype)

        n_under = sa.largest_under(fast, 1, 1 << 24)
        for n in sorted({1, 2, n_under // 2, n_under - 1, n_under}):
            if n < 1:
                continue
            code = plan(mode, n, h, w, cin, cout, k, s, cls, dtype)
            assert code >= 1000, f"mode {mode} class {cls} N={n}: contract allows an MFMA family, plan says {code}"
            g = sa.Geom(mode, n, h, w, cin, oh, ow, cout, k, s, cls)
            if code // 1000 == 3:
                assert sa.ring_conv_eligible(g, dtype), f"N={n}: ring named outside its contract"
            if code // 1000 == 5:
                assert sa.up2_conv_eligible(sa.Geom(1, n, h, w, cin, oh, ow, cout, k, s, 0), dtype), f"N={n}: up2 named outside its contract"
            # the pixel limit is implied: a descriptor of >= 8-channel rows under 2^30 elements holds fewer than 2^27 pixels
            assert sa.pixels_addressable(g.N * g.Hg * g.Wg + 256) and sa.pixels_addressable(g.N * g.Hd * g.Wd)
        for n in (n_under + 1, n_under + 2, 2 * n_under, min(INT_MAX // (h * w), 64 * n_under)):
            code = plan(mode, n, h, w, cin, cout, k, s, cls, dtype)
            assert code == 0, f"mode {mode} class {cls} N={n} (limit {n_under}): past the descriptor's reach, plan says {code}"


def test_conv_plan_fallback_for_what_no_fast_family_takes():
    lib.load()
    assert plan(0, 2, 16, 16, 12, 16, 3, 1, 0, sa.BF16) == 0          # Cin % 8
    assert plan(0, 2, 16, 16, 16, 12, 3, 1, 0, sa.BF16) == 0          # Cout % 8
    assert plan(0, 2, 16, 16, 16, 16, 3, 1, 0, sa.F32) == 0           # fp32
    assert plan(0, 2, 16, 16, 16, 16, 3, 1, 0, sa.BF16) >= 1000
    assert plan(0, 2, 16, 16, 16, 16, 5, 1, 0, sa.BF16) == -1         # unsupported k
    assert plan(0, 2, 16, 16, 16, 16, 1, 2, 0, sa.BF16) == -1
    # the weight matrix has a descriptor of its own: Cd * Kpad < 2^30 (ring: * 4)
    assert not sa.mfma_conv_eligible(sa.Geom(0, 1, 4, 4, 32768, 4, 4, 4096, 3, 1), sa.BF16)
    assert plan(0, 1, 4, 4, 32768, 4096, 3, 1, 0, sa.BF16) == 0
    assert plan(0, 1, 4, 4, 16384, 4096, 3, 1, 0, sa.BF16) >= 1000


# (H, W, Cin, Cout, k, s, ldx, ldy): dense rows and channel slices of wide buffers; the x side or the dy side crosses first
WGRAD_SWEEP = [(61, 59, 16, 16, 1, 1, sa.LD_CONV[0], 16), (61, 59, 16, 16, 3, 1, 16, sa.LD_FLAT[0]), (61, 59, 16, 16, 3, 2, sa.LD_CONV[0], 16),
               (640, 640, 64, 64, 3, 1, 64, 64), (320, 320, 32, 64, 3, 2, 32, 64), (160, 160, 64, 256, 1, 1, 64, 256),
               (80, 80, 128, 64, 3, 1, 384, 64), (122, 118, 64, 64, 3, 2, 64, 4096)]


@pytest.mark.parametrize("h,w,cin,cout,k,s,ldx,ldy", WGRAD_SWEEP)
def test_wgrad_workspace_switches_with_the_path_at_the_limit(h, w, cin, cout, k, s, ldx, ldy):
    lib.load()
    oh, ow = sa.conv_out_hw(h, w, k, s)
    kpad = sa.round_up32(k * k * cin)

    def ws(n, ldx_, ldy_, algo=0, dtype=sa.BF16):
        args = (PTR, ldx_, PTR, ldy_, n, h, w, cin, oh, ow, cout, k, s, dtype, algo)
        assert all(0 <= a <= INT_MAX for a in args[1:]), args
        sa.check_args("yolo_conv2d_wgrad_ws_elems", lib._protos, args)
        return lib.query("yolo_conv2d_wgrad_ws_elems", *args)

    n_under = sa.largest_under(lambda n: sa.wgrad_path(n, h, w, cin, oh, ow, cout, sa.BF16, ldx, ldy) == 2, 1, 1 << 24)
    for n in sorted({1, n_under - 1, n_under}):
        if n < 1:
            continue
        dense = ws(n, cin, cout)              # the partial-matrix workspace is a function of the dimensions alone
        if sa.wgrad_path(n, h, w, cin, oh, ow, cout, sa.BF16, cin, cout) == 2:
            assert ws(n, ldx, ldy) == dense, f"N={n}: under the limit, yet not the partial-matrix workspace"
        assert ws(n, ldx, ldy, algo=3) == cout * kpad and ws(n, ldx, ldy, algo=1) == cout * kpad
        plan_code = lib.query("yolo_conv2d_wgrad_plan", n, h, w, cin, oh, ow, cout, k, s, sa.BF16)
        assert plan_code > 0, f"N={n}: the MFMA weight gradient has no plan ({plan_code})"
    assert ws(n_under, ldx, ldy) != cout * kpad, "a switch of the path would be invisible in the workspace size at this shape"
    for n in (n_under + 1, n_under + 2, 2 * n_under):
        assert sa.wgrad_path(n, h, w, cin, oh, ow, cout, sa.BF16, ldx, ldy) == 3
        assert ws(n, ldx, ldy) == cout * kpad, f"N={n} (limit {n_under}): past the limit, yet not the one-matrix workspace"
    assert ws(2, ldx, ldy, dtype=sa.F32) == cout * kpad                # fp32: the generic / fp32 kernels, one matrix


@pytest.mark.parametrize("h,w,c", [(61, 59, 16), (160, 160, 64), (80, 80, 128), (20, 20, 512), (7, 193, 8), (320, 320, 32)])
def test_dw_plan_names_the_16bit_kernels_up_to_2_31_bytes(h, w, c):
    lib.load()
    n_under = sa.largest_under(lambda n: sa.dw16_takes(n, h, w, c, c, c), 1, 1 << 24)
    assert n_under * h * w * c * 2 < sa.WRAP31 <= (n_under + 1) * h * w * c * 2
    for field in (0, 12):
        for n in sorted({1, n_under - 1, n_under}):
            assert lib.query("yolo_dw_plan", n, h, w, c, field) in (1, 2), (n, field)
        for n in (n_under + 1, 2 * n_under):
            assert n * h * w < INT_MAX
            assert lib.query("yolo_dw_plan", n, h, w, c, field) == 0, (n, field)
    assert lib.query("yolo_dw_plan", 2, h, w, c + 4, 0) == 0               # C % 8: the generic kernels
    assert lib.query("yolo_dw_plan", 0, h, w, c, 0) == -1
    # the launch-side test sees the row strides, source and destination independently
    assert sa.dw16_takes(9, 61, 59, 16, sa.LD_FLAT[0], 16) and not sa.dw16_takes(9, 61, 59, 16, sa.LD_FLAT[1], 16)
    assert sa.dw16_takes(9, 61, 59, 16, 16, sa.LD_FLAT[0]) and not sa.dw16_takes(9, 61, 59, 16, 16, sa.LD_FLAT[1])


def test_stem_conv_eligible_is_the_documented_table():
    lib.load()
    for img_dt in (sa.F32, sa.BF16, sa.F16):
        for dtype in (sa.F32, sa.BF16, sa.F16):
            for cout in (0, 8, 16, 24, 32, 48, 64, 80, 96, 112, 128, 144, 160, 256):
                want = sa.stem_conv_eligible(img_dt, dtype, cout) and cout > 0
                assert bool(lib.query("yolo_stem_conv_eligible", img_dt, dtype, cout)) == want, (img_dt, dtype, cout)


def test_layout_pairs_lie_either_side_of_their_limit():
    n, h, w = sa.NPIX_IMG
    p = n * h * w
    for (under, over), extra in ((sa.LD_CONV, w + 1), (sa.LD_FLAT, 0)):
        assert over == under + 8 and under % 8 == 0
        assert (p + extra) * under < sa.DESC_ELEMS <= (p + extra) * over
    assert p * (sa.LD_2G - 8) < (1 << 31) <= p * sa.LD_2G and sa.LD_2G < INT_MAX
    g_u = sa.Geom(0, n, h, w, 64, h, w, 64, 3, 1, 0, sa.LD_CONV[0], 64)
    g_o = sa.Geom(0, n, h, w, 64, h, w, 64, 3, 1, 0, sa.LD_CONV[1], 64)
    assert sa.mfma_conv_eligible(g_u, sa.BF16) and sa.ring_conv_eligible(g_u, sa.BF16) and not sa.mfma_conv_eligible(g_o, sa.BF16)
    # the destination is in no guard: a small source stays on the MFMA families whatever the destination's row stride
    assert sa.mfma_conv_eligible(sa.Geom(0, n, h, w, 64, h, w, 64, 3, 1, 0, 64, sa.LD_2G), sa.BF16)
    up_u = sa.Geom(1, n, 2 * h, 2 * w, 64, h, w, 64, 3, 2, 0, 64, sa.LD_CONV[0])
    up_o = sa.Geom(1, n, 2 * h, 2 * w, 64, h, w, 64, 3, 2, 0, 64, sa.LD_CONV[1])
    assert sa.up2_conv_eligible(up_u, sa.BF16) and sa.mfma_conv_eligible(up_u, sa.BF16) and not sa.mfma_conv_eligible(up_o, sa.BF16)
    assert sa.wgrad_path(n, h, w, 16, h, w, 16, sa.BF16, sa.LD_CONV[0], 16) == 2
    assert sa.wgrad_path(n, h, w, 16, h, w, 16, sa.BF16, sa.LD_CONV[1], 16) == 3
    assert sa.wgrad_path(n, h, w, 16, h, w, 16, sa.BF16, 16, sa.LD_FLAT[0]) == 2
    assert sa.wgrad_path(n, h, w, 16, h, w, 16, sa.BF16, 16, sa.LD_FLAT[1]) == 3


# ---------------------------------------------------------------------------------------------- argument-range checker
MADE_UP = """
int toy_launch(const void* x, int ldx, long npix, int C, float scale, hipStream_t st);
size_t toy_bytes(int N, size_t each);
long toy_plan(void);
"""


def test_checker_refuses_what_ctypes_would_truncate():
    protos = sa.parse_prototypes(MADE_UP)
    assert list(protos) == ["toy_launch", "toy_bytes", "toy_plan"]
    assert protos["toy_launch"][2] == ["x", "ldx", "npix", "C", "scale", "st"]
    sa.check_args("toy_launch", protos, (PTR, INT_MAX, 1 << 40, 16, 0.5, 0))
    sa.check_args("toy_launch", protos, (PTR, -(1 << 31), -(1 << 63), 0, 1, 0))
    sa.check_args("toy_plan", protos, ())
    assert ctypes.c_int((1 << 32) + 5).value == 5                      # what the checker is for
    for args, entry, param in [((PTR, 1 << 31, 4, 16, 0.5, 0), "toy_launch", "ldx"), ((PTR, 8, 1 << 63, 16, 0.5, 0), "toy_launch", "npix"),
                               ((PTR, 8, 4, (1 << 32) + 16, 0.5, 0), "toy_launch", "C"), ((PTR, 8, 4, -(1 << 31) - 1, 0.5, 0), "toy_launch", "C"),
                               ((-8, 8, 4, 16, 0.5, 0), "toy_launch", "x"), ((PTR, 8, 4, 16, 0.5, 1 << 64), "toy_launch", "st"),
                               ((3, -1), "toy_bytes", "each"), ((1 << 31, 8), "toy_bytes", "N"), ((PTR, 8.0, 4, 16, 0.5, 0), "toy_launch", "ldx")]:
        with pytest.raises(sa.ArgumentOutOfRange) as e:
            sa.check_args(entry, protos, args)
        assert entry in str(e.value) and f"`{param}`" in str(e.value), str(e.value)
    # integers that are not `int`: numpy scalars and 0-d tensors are truncated by ctypes in the same way
    sa.check_args("toy_launch", protos, (np.int64(PTR), np.int32(8), torch.tensor(4), np.int64(16), 0.5, None))
    for bad in (np.int64(1 << 31), torch.tensor(1 << 40), np.uint64((1 << 32) + 16)):
        with pytest.raises(sa.ArgumentOutOfRange, match="toy_launch.*`C`"):
            sa.check_args("toy_launch", protos, (PTR, 8, 4, bad, 0.5, 0))
    with pytest.raises(sa.ArgumentOutOfRange, match="`ldx`"):
        sa.check_args("toy_launch", protos, (PTR, "8", 4, 16, 0.5, 0))
    with pytest.raises(sa.ArgumentOutOfRange):
        sa.check_args("toy_launch", protos, (PTR, 8, 4, 16, 0.5))       # arity
    with pytest.raises(sa.ArgumentOutOfRange):
        sa.check_args("toy_missing", protos, ())


def test_checker_wraps_the_loader(monkeypatch):
    seen = sa.install_checker(monkeypatch)
    assert lib.query("yolo_conv_kpad", 16, 16, 3, 1, 0, 0) == 160
    lib.call("yolo_conv_tune_set", *DEFAULT_TUNE)
    assert seen == ["yolo_conv_kpad", "yolo_conv_tune_set"]
    with pytest.raises(sa.ArgumentOutOfRange, match="yolo_conv_kpad.*`I`"):
        lib.query("yolo_conv_kpad", 16, 1 << 32, 3, 1, 0, 0)
    with pytest.raises(sa.ArgumentOutOfRange, match="yolo_copy_channels.*`ld_dst`"):
        lib.call("yolo_copy_channels", PTR, 8, PTR, 1 << 31, 4, 8, 0, sa.BF16, 0)
    assert seen == ["yolo_conv_kpad", "yolo_conv_tune_set"]            # a refused call never reaches the library


# ---------------------------------------------------------------------------------------------- wrap mutants
NPIX_SMALL, ROWS_BEFORE_WRAP = 24, 8


def _case_data(lay, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(NPIX_SMALL, lay.c, generator=g).to(torch.bfloat16).double().numpy()
    buf = np.full((NPIX_SMALL, lay.ld), 3.0)
    buf[:, lay.off:lay.off + lay.c] = x
    return x, buf


def _share_outside(got, ref, mass, beyond):
    """share of the elements beyond the wrap point that leave the conv family's bound (strict_compare.limit, c = 16) -- the
    WIDEST per-element bound any GPU case of these layouts is held to (the move and copy cases are bit-exact)"""
    got, ref, mass = (torch.from_numpy(np.ascontiguousarray(a)) for a in (got, ref, mass))
    lim = sc.limit(ref, got, mass, torch.bfloat16)
    out = ((got - ref).abs() > lim).numpy()
    assert beyond.any(), "no element of the scaled case lies beyond the wrap point"
    return float(out[beyond].mean())


@pytest.mark.parametrize("lay", sa.gpu_layouts(), ids=lambda l: f"{l.name}-c{l.c}")
def test_every_wrap_is_visible_at_every_gpu_layout(lay):
    """a kernel whose byte offsets wrapped at 2^31 or 2^32 bytes, or whose pixel index wrapped, on a scaled copy of the
    layout: more than half of the elements beyond the wrap point leave the bound, as values read (gather), as values
    stored (scatter) and through a 1x1 conv that reads them"""
    rowbytes = lay.ld * 2
    x, buf = _case_data(lay, lay.ld + lay.off + lay.c)
    g = torch.Generator().manual_seed(7)
    wt = (torch.randn(lay.c, lay.c, generator=g) * lay.c ** -0.5).to(torch.bfloat16).double().numpy()
    for wrap in (sa.WRAP31, sa.WRAP32):
        r = wrap % rowbytes
        assert r != 0, f"{lay}: {wrap} bytes is a whole number of pixel rows: a wrapped address would land on its own channel"
        small = sa.scaled(lay, ROWS_BEFORE_WRAP, wrap)
        got, beyond = sa.wrapped_gather(buf, lay.off, lay.c, small)
        assert _share_outside(got, x, np.abs(x), beyond) > 0.5, f"{lay}: a read wrapped at {wrap} bytes stays inside the bound"
        assert np.array_equal(got[~beyond], x[~beyond])
        held, beyond_s, whole = sa.wrapped_scatter(x, 3.0, NPIX_SMALL, lay.ld, lay.off, small)
        assert _share_outside(held, x, np.abs(x), beyond_s) > 0.5, f"{lay}: a store wrapped at {wrap} bytes stays inside the bound"
        guard = np.ones(lay.ld, bool)
        guard[lay.off:lay.off + lay.c] = False
        landed_in_guard = bool((whole[:, guard] != 3.0).any())
        landed_in_slice = bool((held[~beyond_s] != x[~beyond_s]).any())
        assert landed_in_guard or landed_in_slice, f"{lay}: the wrapped stores left no trace"
        y_ref, y_mass = x @ wt.T, np.abs(x) @ np.abs(wt).T
        assert _share_outside(got @ wt.T, y_ref, y_mass, np.broadcast_to(beyond.any(1)[:, None], y_ref.shape)) > 0.5, \
            f"{lay}: a 1x1 conv over a source wrapped at {wrap} bytes stays inside its bound"
    got, beyond = sa.pixel_wrapped_gather(buf, lay.off, lay.c, ROWS_BEFORE_WRAP)
    assert _share_outside(got, x, np.abs(x), beyond) > 0.5, f"{lay}: a wrapped pixel index stays inside the bound"


def test_a_layout_that_hides_the_wrap_is_refused():
    """2^31 bytes a whole number of rows: the wrapped read lands on the same channel of another pixel; with periodic data
    (the batch is built from three base images) it reads the very same value -- the mutant test must notice the layout"""
    lay = sa.Layout("hidden", 9, 61, 59, 16, 32768, 64)
    assert sa.WRAP31 % (lay.ld * 2) == 0
    x = np.tile(np.arange(16.0)[None, :], (NPIX_SMALL, 1))              # every pixel alike
    buf = np.full((NPIX_SMALL, lay.ld), 3.0)
    buf[:, 64:80] = x
    got, beyond = sa.wrapped_gather(buf, 64, 16, sa.scaled(lay, ROWS_BEFORE_WRAP, sa.WRAP31))
    assert beyond.any() and np.array_equal(got, x)                      # invisible: hence the r != 0 assertion above
    assert all(sa.WRAP31 % (l.ld * 2) and sa.WRAP32 % (l.ld * 2) for l in sa.gpu_layouts())
