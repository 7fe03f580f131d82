"""The 32-bit addressing contract of the fast kernels, restated from the documented rule (csrc/conv_host.h, conv_mfma.hip,
conv_ring.hip, conv_up2.hip, wgrad_path in conv_generic.hip, dw_eligible in dwconv.hip) -- NOT obtained from the library --
plus what the size tests share: the argument-range checker for lib.call / lib.query, the wrap mutants, the layouts of the
GPU cases and the device-side helpers that build a channel slice of a buffer wider than the limit.

The rule.  A buffer descriptor carries an `int` byte count and 32-bit byte offsets over 2-byte elements, so ONE descriptor
covers fewer than 2^30 elements (2^31 bytes); the descriptor of a conv source starts one row and one pixel before the
tensor, so it covers N*Hs*Ws*lds + (Ws+1)*lds elements; pixel indices are `int`, so a launch walks fewer than 2^31 pixels
(the gather kernel up to the end of its last 256-pixel tile).  What a descriptor covers is the ROW STRIDE of the buffer
(lds), not the channels of the slice.  Destinations are written through 64-bit pointers and are not part of any guard.

    MFMA conv (all five families)  16-bit dtype, lds % 8 == 0, Cd % 8 == 0, ldd % 4 == 0, Cs % 8 == 0,
                                   N*Hs*Ws*lds + (Ws+1)*lds < 2^30, N*Hg*Wg + 256 < 2^31, Cd*Kpad < 2^30
      ring, in addition            Cs % 32 == 0, Cs >= 64, Cd*Kpad*4 < 2^30
      up2 (stride-2 data gradient) even Hd, Wd, Cs % 32 == 0, Cd >= 32, N*Hs*Ws*lds < 2^30 (unshifted), N*Hd*Wd < 2^31
    weight gradient                partial-matrix design unless N*H*W*ldx + (W+1)*ldx >= 2^30 or N*OH*OW*ldy >= 2^30
                                   (`big`): then the first design (atomics into one Cout x Kpad matrix)
    depthwise, 16-bit kernels      C, ldx, ldy % 8 == 0 and N*H*W*ldx*2 < 2^31 and N*H*W*ldy*2 < 2^31, source and
                                   destination independently; the plan query sees dense rows: N*H*W*C*2 < 2^31
Everything else (element-wise, BatchNorm, pool, upsample, copy, transpose, head-group, attention, the stem's and every
conv's epilogue stores) has no guard: its index arithmetic is `long` (the audit table)."""
import ctypes
import numbers
import re

import numpy as np
import torch

F32, BF16, F16 = 0, 1, 2
ERR_ARG = 1001
DESC_ELEMS = 1 << 30          # elements of 2 bytes one descriptor can cover: desc_addressable (conv_host.h)
PIXELS = 1 << 31              # pixels_addressable
WRAP31, WRAP32 = 1 << 31, 1 << 32


def desc_addressable(elems):
    return elems < DESC_ELEMS


def pixels_addressable(npix):
    return npix < PIXELS


def conv_out_hw(h, w, k, s):
    pad = k // 2
    return (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1


def round_up32(k):
    return (k + 31) // 32 * 32


def conv_supported(k, s):
    return (k == 1 and s == 1) or (k == 3 and s in (1, 2))


class Geom:
    """ConvGeom of a forward (mode 0) or of parity class `cls` of a data gradient (mode 1), as conv_geom.h states it"""

    def __init__(self, mode, n, h, w, cin, oh, ow, cout, k, s, cls=0, ldx=None, ldy=None):
        ldx, ldy = cin if ldx is None else ldx, cout if ldy is None else ldy
        self.N = n
        if mode == 0:
            self.Hs, self.Ws, self.Cs, self.lds = h, w, cin, ldx
            self.Hd, self.Wd, self.Cd, self.ldd = oh, ow, cout, ldy
            self.Hg, self.Wg, self.ntaps, self.ostep = oh, ow, k * k, 1
        else:
            self.Hs, self.Ws, self.Cs, self.lds = oh, ow, cout, ldy
            self.Hd, self.Wd, self.Cd, self.ldd = h, w, cin, ldx
            if s == 1:
                self.Hg, self.Wg, self.ntaps, self.ostep = h, w, k * k, 1
            else:
                ph, pw = cls >> 1, cls & 1
                self.Hg = (h + 1) // 2 if ph == 0 else h // 2
                self.Wg = (w + 1) // 2 if pw == 0 else w // 2
                self.ntaps, self.ostep = (1, 2, 2, 4)[cls], 2
        self.Kpad = round_up32(self.ntaps * self.Cs)


def mfma_conv_addressable(g, dtype):
    if dtype not in (BF16, F16):
        return False
    if g.lds % 8 or g.Cd % 8 or g.ldd % 4:
        return False
    if not desc_addressable(g.N * g.Hs * g.Ws * g.lds + (g.Ws + 1) * g.lds):
        return False
    return pixels_addressable(g.N * g.Hg * g.Wg + 256)


def mfma_conv_eligible(g, dtype):
    return mfma_conv_addressable(g, dtype) and g.Cs % 8 == 0 and desc_addressable(g.Cd * g.Kpad)


def ring_conv_eligible(g, dtype):
    return mfma_conv_addressable(g, dtype) and g.Cs % 32 == 0 and g.Cs >= 64 and desc_addressable(g.Cd * g.Kpad * 4)


def up2_conv_eligible(g0, dtype):
    """g0: class 0 of a 3x3 stride-2 data gradient"""
    if dtype not in (BF16, F16):
        return False
    if (g0.Hd & 1) or (g0.Wd & 1) or g0.Hs * 2 != g0.Hd or g0.Ws * 2 != g0.Wd:
        return False
    if g0.Cs % 32 or g0.Cd % 8 or g0.Cd < 32 or g0.lds % 8 or g0.ldd % 4:
        return False
    return desc_addressable(g0.N * g0.Hs * g0.Ws * g0.lds) and pixels_addressable(g0.N * g0.Hd * g0.Wd)


def conv_plan_is_fast(mode, n, h, w, cin, oh, ow, cout, k, s, cls, dtype, ldx=None, ldy=None):
    """does the launcher name an MFMA family (plan code >= 1000) for this launch?  (the gather kernel takes every eligible one)"""
    return mfma_conv_eligible(Geom(mode, n, h, w, cin, oh, ow, cout, k, s, cls, ldx, ldy), dtype)


def wgrad_big(n, h, w, oh, ow, ldx, ldy):
    return n * h * w * ldx + (w + 1) * ldx >= DESC_ELEMS or n * oh * ow * ldy >= DESC_ELEMS


def wgrad_path(n, h, w, cin, oh, ow, cout, dtype, ldx, ldy, algo=0):
    """2 = partial matrices + reduce, 3 = first design (atomics), 1 = generic / fp32 kernels (wgrad_path, conv_generic.hip)"""
    ok = dtype in (BF16, F16) and not (cin % 8 or cout % 8 or ldx % 8 or ldy % 8)
    if algo == 1 or not ok:
        return 1
    return 3 if (algo == 3 or wgrad_big(n, h, w, oh, ow, ldx, ldy) or n * oh * ow == 0) else 2


def dw16_takes(n, h, w, c, ldx, ldy):
    """the 16-bit depthwise kernels (rows / strip) take the launch; otherwise the generic k_dw3x3*"""
    if c % 8 or ldx % 8 or ldy % 8:
        return False
    if n * h * w * ldx * 2 >= WRAP31 or n * h * w * ldy * 2 >= WRAP31:
        return False
    return n * h * w > 0


def stem_conv_eligible(img_dtype, dtype, cout):
    return img_dtype == F32 and dtype in (BF16, F16) and cout % 16 == 0 and cout // 16 in (1, 2, 3, 4, 6, 8)


def largest_under(pred, lo=1, hi=1 << 31):
    """largest v in [lo, hi) with pred(v) true, pred monotone true -> false; (v, v + 1) is the pair either side of a limit"""
    assert pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return lo


# ---------------------------------------------------------------------------------------------- argument-range checker
_RANGE = {ctypes.c_int: (-(1 << 31), (1 << 31) - 1), ctypes.c_long: (-(1 << 63), (1 << 63) - 1),
          ctypes.c_size_t: (0, (1 << 64) - 1), ctypes.c_void_p: (0, (1 << 64) - 1)}


class ArgumentOutOfRange(ValueError):
    pass


def check_args(name, protos, args):
    """refuse a Python integer that does not fit the C type of its parameter (ctypes truncates it silently: c_int(2**32 + 5)
    is 5); protos = {entry: (restype, [ctypes type], [parameter name])} as src.hipops.lib.parse_header returns it"""
    if name not in protos:
        raise ArgumentOutOfRange(f"{name}: no such entry point in the header")
    _, types, names = protos[name]
    if len(args) != len(types):
        raise ArgumentOutOfRange(f"{name}: {len(args)} arguments for {len(types)} parameters")
    for a, t, pn in zip(args, types, names):
        if isinstance(a, (float, ctypes._SimpleCData, ctypes.Array)) or a is None:
            if isinstance(a, float) and t not in (ctypes.c_float, ctypes.c_double):
                raise ArgumentOutOfRange(f"{name}: parameter `{pn}` ({t.__name__}) was given the float {a}")
            continue
        try:                                   # bool, int, numpy integers, 0-d integer tensors: whatever ctypes would take as an index
            v = a.__index__() if isinstance(a, numbers.Integral) or hasattr(a, "__index__") else None
        except TypeError:
            v = None
        if v is None:
            raise ArgumentOutOfRange(f"{name}: parameter `{pn}` ({t.__name__}) was given {type(a).__name__} {a!r}")
        if t in _RANGE:
            lo, hi = _RANGE[t]
            if not lo <= v <= hi:
                raise ArgumentOutOfRange(f"{name}: parameter `{pn}` ({t.__name__}) cannot hold {v}")


def parse_prototypes(text):
    """the prototypes of a header text, by the loader's own rule (one `int|long|size_t name(args);` per line)"""
    from src.hipops import lib
    protos = {}
    for ret, name, args in re.findall(r"^(int|long|size_t)\s+(\w+)\s*\(([^)]*)\)\s*;", text, re.M):
        types, names = [], []
        for a in [s.strip() for s in args.split(",") if s.strip() and s.strip() != "void"]:
            toks = a.replace("*", " * ").split()
            names.append(toks[-1])
            types.append(ctypes.c_void_p if "*" in toks else lib._CT[[t for t in toks[:-1] if t != "const"][0]])
        protos[name] = (lib._CT[ret], types, names)
    return protos


def install_checker(monkeypatch):
    """wrap lib.call / lib.query (every op of src.hipops.ops goes through them) with check_args; -> list of checked names"""
    from src.hipops import lib
    lib.load()
    protos, seen = lib._protos, []
    call0, query0 = lib.call, lib.query

    def call(name, *args):
        check_args(name, protos, args)
        seen.append(name)
        return call0(name, *args)

    def query(name, *args):
        check_args(name, protos, args)
        seen.append(name)
        return query0(name, *args)

    monkeypatch.setattr(lib, "call", call)
    monkeypatch.setattr(lib, "query", query)
    return seen


# ---------------------------------------------------------------------------------------------- layouts of the GPU cases
class Layout:
    """A channel slice [off, off + c) of an NHWC buffer (n, h, w, ld) of 2-byte elements"""

    def __init__(self, name, n, h, w, c, ld, off):
        self.name, self.n, self.h, self.w, self.c, self.ld, self.off = name, n, h, w, c, ld, off
        assert ld % 8 == 0 and off % 8 == 0 and 0 <= off and off + c <= ld

    npix = property(lambda s: s.n * s.h * s.w)
    elems = property(lambda s: s.npix * s.ld)
    bytes = property(lambda s: s.elems * 2)
    conv_desc_elems = property(lambda s: s.elems + (s.w + 1) * s.ld)       # what a conv source descriptor covers

    def top(self):
        return Layout(self.name + "-top", self.n, self.h, self.w, self.c, self.ld, self.ld - self.c)

    def __repr__(self):
        return f"{self.name}: {self.n}x{self.h}x{self.w} pixels, ld {self.ld}, slice [{self.off}, {self.off + self.c}): " \
               f"{self.elems} elements, {self.bytes} bytes"


# nine 61 x 59 images (3599 pixels each: no multiple of 16, 64, 80 or 128, so every kernel's last tile is partial; 32391 pixels
# in all: hundreds of workgroups); the row stride carries the span across the limit.
NPIX_IMG = (9, 61, 59)
_P = 9 * 61 * 59


def _ld_pair(extra_rows_elems):
    """(largest ld % 8 == 0 with P*ld + extra*ld < 2^30, the next multiple of 8)"""
    under = largest_under(lambda ld: (_P + extra_rows_elems) * ld * 8 < DESC_ELEMS) * 8
    return under, under + 8


LD_CONV = _ld_pair(59 + 1)       # conv source / wgrad x: + (W + 1) rows of the shifted descriptor
LD_FLAT = _ld_pair(0)            # wgrad dy, up2's unshifted descriptor, the depthwise byte test
LD_2G = largest_under(lambda ld: _P * ld * 8 < (1 << 31)) * 8 + 8      # first ld % 8 with P*ld >= 2^31 ELEMENTS (2^32 bytes)


def layout(kind, c, side, where="mid"):
    """kind: 'conv' / 'flat' with side 'under' / 'over' (either side of 2^30 elements = 2^31 bytes), or '2g' (the buffer
    crosses 2^31 elements = 2^32 bytes: where an `int` element index would wrap)"""
    n, h, w = NPIX_IMG
    if kind == "2g":
        return layout_2g(n, h, w, c, where)
    ld = {"conv": LD_CONV, "flat": LD_FLAT}[kind][0 if side == "under" else 1]
    off = {"bottom": 0, "top": ld - c, "mid": (ld // 2) // 8 * 8}[where]
    return Layout(f"{kind}-{side}-{where}", n, h, w, c, ld, off)


# every (n, h, w, c) map that a GPU case places in a buffer past 2^31 elements (layout_2g refuses any other): the nine-image
# maps of the conv, move, BatchNorm and stem cases, the patch kernel's 122 x 118 destination, the upsample pair, and the
# attention problems (3 images of 400 = 20 x 20 and 143 = 11 x 13 tokens; qkv and o / d_o widths of both head shapes)
MAPS_2G = [(9, 61, 59, 16), (9, 61, 59, 64), (9, 122, 118, 64), (9, 31, 29, 16), (9, 62, 58, 16),
           (3, 20, 20, 256), (3, 20, 20, 128), (3, 11, 13, 192), (3, 11, 13, 96)]


def layout_2g(n, h, w, c, where):
    """slice of the narrowest buffer (ld % 8 == 0) of this map that holds at least 2^31 elements"""
    assert (n, h, w, c) in MAPS_2G, f"{(n, h, w, c)} is not listed in MAPS_2G: the wrap-mutant test would not see its row stride"
    ld = largest_under(lambda m: n * h * w * m * 8 < (1 << 31)) * 8 + 8
    off = {"bottom": 0, "top": ld - c, "mid": (ld // 2) // 8 * 8}[where]
    lay = Layout(f"2g-{where}", n, h, w, c, ld, off)
    assert lay.elems >= (1 << 31) and ld < (1 << 31)
    return lay


def gpu_layouts():
    """every (row stride, offset, channels) the GPU cases use -- they build theirs with layout() and layout_2g() only: the
    wrap-mutant test runs over all of them"""
    out = []
    for c in (16, 64):
        for where in ("bottom", "top", "mid"):
            for kind in ("conv", "flat"):
                for side in ("under", "over"):
                    out.append(layout(kind, c, side, where))
    for n, h, w, c in MAPS_2G:
        for where in ("bottom", "top", "mid"):
            out.append(layout_2g(n, h, w, c, where))
    return out


# ---------------------------------------------------------------------------------------------- wrap mutants (CPU, float64)
def scaled(lay, rows_before_wrap, wrap):
    """A scaled-down copy of a layout for the mutant test: same ld, offset and channels, `npix` pixels, and a wrap point of
    q' * rowbytes + r bytes, r = wrap % rowbytes the residue of the real wrap point (2^31 or 2^32 bytes) in a pixel row:
    a wrapped byte offset lands on the same channel of a pixel q' rows back as it would in the full-size buffer."""
    rowbytes = lay.ld * 2
    return rows_before_wrap * rowbytes + wrap % rowbytes


def wrapped_gather(buf, lay_off, c, wrap_bytes):
    """buf: float64 (npix, ld) whole buffer.  What a kernel would READ as the slice if its byte offsets were reduced modulo
    wrap_bytes -> (npix, c), and the mask of elements whose offset lies beyond the wrap point"""
    npix, ld = buf.shape
    p = np.arange(npix, dtype=np.int64)[:, None]
    ch = np.arange(c, dtype=np.int64)[None, :]
    byte = (p * ld + lay_off + ch) * 2
    beyond = byte >= wrap_bytes
    elem = (byte % wrap_bytes) // 2
    return buf.reshape(-1)[elem], beyond


def wrapped_scatter(vals, fill, npix, ld, lay_off, wrap_bytes):
    """What the slice HOLDS after a kernel stored `vals` (npix, c) through byte offsets reduced modulo wrap_bytes into a
    buffer filled with `fill` -> (slice as read back correctly, mask beyond the wrap point, whole buffer)"""
    c = vals.shape[1]
    p = np.arange(npix, dtype=np.int64)[:, None]
    ch = np.arange(c, dtype=np.int64)[None, :]
    byte = (p * ld + lay_off + ch) * 2
    beyond = byte >= wrap_bytes
    buf = np.full(npix * ld, fill, dtype=np.float64)
    buf[(byte % wrap_bytes) // 2] = vals
    return buf.reshape(npix, ld)[:, lay_off:lay_off + c], beyond, buf.reshape(npix, ld)


def pixel_wrapped_gather(buf, lay_off, c, wrap_pix):
    """the same with the PIXEL index reduced modulo wrap_pix (an `int` pixel counter that wrapped)"""
    npix, ld = buf.shape
    p = np.arange(npix, dtype=np.int64)
    beyond = np.broadcast_to((p >= wrap_pix)[:, None], (npix, c))
    return buf[p % wrap_pix][:, lay_off:lay_off + c], beyond


# ---------------------------------------------------------------------------------------------- device-side helpers
def wide_buffer(lay, dtype, fill, device="cuda"):
    """-> (buffer as logical (n, ld, h, w) NHWC tensor filled with `fill`, its channel-slice view)"""
    buf = torch.empty((lay.n, lay.h, lay.w, lay.ld), dtype=dtype, device=device).permute(0, 3, 1, 2)
    buf.fill_(fill)
    return buf, buf[:, lay.off:lay.off + lay.c]


def put(lay, t, fill, device="cuda"):
    """(n, c, h, w) CPU tensor -> slice of a filled wide buffer on the device"""
    assert tuple(t.shape) == (lay.n, lay.c, lay.h, lay.w), (tuple(t.shape), lay)
    buf, view = wide_buffer(lay, t.dtype, fill, device)
    view.copy_(t.to(device))
    return buf, view


def assert_guard_channels(buf, lay, fill, what, also=()):
    """on the device, image by image: every channel of the buffer outside the slice (and outside the further slices
    `also` = [(offset, channels), ...]) still holds `fill`"""
    f = torch.tensor(fill, dtype=buf.dtype, device=buf.device)      # the fill as the buffer's type rounds it
    used = sorted([(lay.off, lay.c)] + list(also))
    gaps, at = [], 0
    for off, c in used:
        gaps.append((at, off))
        at = off + c
    gaps.append((at, lay.ld))
    for i in range(lay.n):
        for lo, hi in gaps:
            if hi > lo:
                bad = int((buf[i, lo:hi] != f).sum())
                assert bad == 0, f"{what}: {bad} guard elements of image {i}, channels [{lo}, {hi}), no longer hold {fill}"
