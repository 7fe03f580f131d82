"""Strict per-pixel comparator for the on-device input pipeline (csrc/image_prep.hip): resize + flip, mosaic, brightness,
contrast, saturation, hue, normalise.  float64 references of each stage taken from the SAME uint8 levels the device stage
saw, a derived error bound per element, and -- because every stage but the last ends in a quantiser -- a SET of allowed
uint8 levels per element instead of a distance.  Shared by tests/test_strict_image_cpu.py (the proof of the comparator, no
GPU) and tests/test_gpu_image.py (the kernels).  strict_compare.py gives ulp() and StrictMismatch.

Allowed levels.  A stage computes v~ = v + d, |d| <= e, from exact inputs and stores q(v~); q is monotone, so the stored level
lies in {q(v) : v in [x - e, x + e]} = the integers from q(x - e) to q(x + e).  An element is AMBIGUOUS when that set has more
than one level.  A reference may return several alternatives (x_a, e_a) for an element (the two floors of a gray that sits on
an integer, the two ends of the contrast mean's interval): the allowed levels are the hull of the alternatives' sets (the
alternatives differ by less than one level, so the hull is their union).  A case whose ambiguous share exceeds CAP_RESIZE = 2 %
(resize) or CAP_COLOUR = 1 % (a colour op) fails as "cannot tell" (CannotTell): that is a condition on the inputs, met by the
reference alone on every case (the CPU module asserts it), not a measurement.

u = 2^-24, gamma_n = n u / (1 - n u) (Higham (3.8)).  The file is compiled without contraction: every fp32 operation rounds
once.  The float64 evaluation's own error (2^-53 per operation) is added as gamma64 terms; it never decides anything.

Resize (resize_ref).  taps(): positions, tri() and the window exactly as taps_of / resize_pixel form them, in fp32 (numpy
float32 performs the same IEEE operations in the same order), so the unnormalised weights wy_j, wx_k ARE the kernel's.
Wy, Wx = their exact sums.  x = sum_jk wy_j wx_k p_jk / (Wy Wx), accumulated in float64.  Every term is >= 0, so the mass
sum |w p| / (Wy Wx) is x itself.  Roundings met by one term in the kernel: the product wx p and the row sum (nx), wsum_x
(nx - 1), wsum_y (ny - 1), tri / wsum_y, wy * r, / wsum_x (3), the sum over rows (ny - 1), acc + 0.5f (1, at x + 0.5):
    e = gamma_{2 nx + 2 ny + 1} (x + 0.5),      nx, ny the taps of THAT pixel
The separable fp32 oracle (weights normalised first: n per axis; two dot products: nx + ny; + 0.5) has the same count.
q(v) = clamp(floor(v + 0.5), 0, 255).
    Exact pixels (e = 0: one level, ties included, outside any cap).  An axis is dyadic when its weights are multiples of
    2^-a (a <= 10) and either Wsum is a power of two or the window is a single tap (then w / w = 1 and (w p) / w = p are exact
    quotients).  With both axes dyadic every intermediate of the kernel is a multiple of 2^-(ax + ay) below 2^9 ny nx, exact in
    fp32 when ax + ay + 8 + ceil(log2 nx) + ceil(log2 ny) <= 24; so is every intermediate of the separable oracle.  This
    holds for identity scale everywhere, for 2x down from an even size in the INTERIOR (weights 1/4 3/4 3/4 1/4, sum 2; the
    first and last output index lose a tap and normalise by 1.75, which is not exact: those pixels take the set), and for
    the whole of 1 x 9 -> 16 and 9 x 1 -> 16 (9 / 16 is dyadic, two taps w and 1 - w; one tap at the ends).

Gray.  g = c0 R + c1 G + c2 B with the fp32 constants, exact in float64 (24 + 8 bits per product); three products and two
additions, the first product meets three roundings: e_g = gamma_3 g.  floor(g) is the pair floor(g - e_g), floor(g + e_g).

Blend (brightness b = 0, contrast b = mean, saturation b = floor(gray)).  ratio is the fp32 value of the record; om = 1 - ratio
exactly.  The kernel rounds a ratio, om, b om and the sum: e = gamma_2 (|a ratio| + |b om|) + |b| e_om (1 + gamma_2).  e_om
covers both ways of forming 1 - ratio in fp32: the kernel's 1.f - ratio (one rounding, 1/2 ulp32(om)) and the oracle's and
torchvision's float32(1.0 - f) from the double f the ratio was rounded from (|f - ratio| <= 1/2 ulp32(ratio), then one
rounding): e_om = 1/2 ulp32(ratio) + 1/2 ulp32(om).  q(v) = floor(clamp(v, 0, 255)).  Saturation: one alternative per floor
of the gray.  Contrast: the blend is monotone in b; one alternative at each end of the mean's interval.

Gray mean (gray_mean_ref).  mean of floor(gray) in float64, once with every ambiguous gray floored down and once up.
k_gray_mean: gx = min(64, ceil(hw / 256)) blocks of 4 waves per image; a thread sums T = ceil(hw / (256 gx)) values serially
(T - 1 additions), the wave reduction adds 6 levels, one division by hw, and the 4 gx partials go through float atomics in
any order (4 gx - 1 additions; the first lands on the zeroed cell): e_m = gamma_{T + 4 gx + 5} mean.  (Sums of floored grays
below 2^24 are in fact exact in fp32; the count is kept as the kernel's depth.)

Hue (hue_ref).  hue_shift transcribed in float64 from the fp32-rounded r (1/255.f); the equality branches are decided on
those values and are exact.  First-order propagation, values in [0, 1] unless stated: cr, s = cr / maxc (2u s); rc gc bc (3u
each); hr <= 7u, hg <= 12u, hb <= 16u (sums at magnitude 3 and 5); / 6 + 1 <= 5.4u; fmod exact; + f (1.5u); h - floor(h) (u):
|dh| <= 8u.  h6 = 6 h: E_F = 6 * 8u + 6u = 54u on h6 and on ff (ff = h6 - fi is exact).  p = v (1 - s): 4u v.
q = v (1 - s ff): v (s E_F + 5u).  t = v (1 - s (1 - ff)): v (s E_F + 6u).  The output channel is one of v, p, q, t by
sector; as a function of h6 it is continuous, piecewise linear with slope <= v s and periodic, so a sector decided
differently changes nothing.  Times k = 256 - 1e-3 and one more rounding:
    e = k v (s E_F + 7u) / (1 - 64u)
q(v) = floor(clamp(v, 0, 255)): a channel whose exact value is 0 has x - e < 0 and is clipped, not floored to -1.

Normalise (normalise_ref).  y = level (1/255.f) exactly, d = y - m, x = d / s with the fp32 m, s:
    e = (u |y| + u |d|) / |s| + u |x| + 1/2 ulp_T(|x| + e')        three fp32 roundings + the store's
No quantiser: |got - x| <= e (check_close).

Mutants: every reference takes mut=; MUTANTS lists them by stage.  Observed on the device: OBSERVED_GPU."""
import functools

import numpy as np
import torch

from oracle import image_prep as oip
from strict_compare import StrictMismatch, ulp  # noqa: F401

f32 = np.float32
U = 2.0 ** -24
U64 = 2.0 ** -53
CAP_RESIZE, CAP_COLOUR = 0.02, 0.01
F32, BF, HF = torch.float32, torch.bfloat16, torch.float16
STATS = {}                # stage -> [elements, ambiguous, compared with the oracle, equal to it, cases, exact-class elements]
MUTANTS = {
    "resize": ["drop_last_tap", "flip_about_w", "trunc"],
    "brightness": ["swap_operands"],
    "saturation": ["gray_unfloored", "gray_0299", "swap_operands"],
    "contrast": ["mean_unfloored", "gray_0299"],
    "hue": ["hue_swap", "k255", "hue_nowrap"],
    "normalise": ["std_perm", "bf16_trunc"],
}
OBSERVED_GPU = """MI355X, tests/test_gpu_image.py, 2026-10-19 (21 tests, 2.1 s), share ambiguous / share equal to the fp32 oracle:
resize 0.013 % / 99.9999 % (116 images, 4.2 M elements, 0.40 M of them exact class; worst case 1000x750 -> 32 0.29 %; 128 -> 64
99.992 % equal: border ties), mosaic 0.057 % / 100 %, brightness 0 / 100 %, contrast 0.001 % / 100 %, saturation 0.615 % / 99.985 %
(488 lattice elements at f = 1.0713 and 1.1871 follow 1.f - ratio, not float32(1.0 - f)), hue 0.028 % / 100 %; normalise uses 0.55
(fp32), 0.999 (bf16), 0.997 (f16) of its bound; the gray mean lies 5e-5 from the float64 mean (allowed 2.3e-3 at S = 512, 3.5e-4 at
S = 50) and differs between two runs in the last bits (float atomics) while the contrast output was bit-equal; nothing outside its set"""


class CannotTell(AssertionError):
    """more ambiguous elements than the cap allows: the case proves nothing"""


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def ulp32(v):
    return ulp(torch.as_tensor(np.asarray(v, np.float64)), F32).numpy()


def q_resize(v):
    return np.clip(np.floor(v + 0.5), 0, 255)


def q_floor(v):
    return np.floor(np.clip(v, 0, 255))


def q_trunc(v):             # the "trunc" mutant of the resize
    return np.clip(np.floor(v), 0, 255)


# ---------------------------------------------------------------------------------------------- the comparator
def allowed(x, e, q, ndim):
    x, e = np.asarray(x, np.float64), np.asarray(e, np.float64)
    if x.ndim == ndim:
        x, e = x[None], e[None]
    return q(x - e).min(0), q(x + e).max(0)


def check_levels(stage, case, got, x, e, q, cap, oracle=None, record=True):
    """got: integer levels; x, e: float64 of got's shape, or (alternatives,) + that shape.  Raises StrictMismatch on any
    element outside its allowed levels, CannotTell when more than `cap` of the elements have more than one.
    -> dict(n, ambiguous, equal)"""
    got = np.asarray(got).astype(np.float64)
    lo, hi = allowed(x, e, q, got.ndim)
    assert lo.shape == got.shape, (stage, case, lo.shape, got.shape)
    bad = (got < lo) | (got > hi)
    n = got.size
    if bad.any():
        x0, e0 = (np.asarray(x)[0], np.asarray(e)[0]) if np.asarray(x).ndim > got.ndim else (np.asarray(x), np.asarray(e))
        dist = np.where(bad, np.maximum(lo - got, got - hi), 0)
        order = np.argsort(-dist, axis=None, kind="stable")[:min(16, int(bad.sum()))]
        worst = []
        lines = [f"{stage} [{case}]: {int(bad.sum())} of {n} elements outside their allowed levels; worst (index, x, e, allowed, got):"]
        for f in order:
            ix = np.unravel_index(f, got.shape)
            worst.append((tuple(int(v) for v in ix), float(got[ix]), float(x0[ix])))
            lines.append(f"    {tuple(int(v) for v in ix)}  x={x0[ix]:.9g}  e={e0[ix]:.3g}  [{int(lo[ix])}, {int(hi[ix])}]  got {int(got[ix])}")
        err = StrictMismatch("\n".join(lines), int(bad.sum()), {}, worst)
        err.families = [stage]
        raise err
    amb = int((lo != hi).sum())
    if amb > cap * n:
        raise CannotTell(f"{stage} [{case}]: cannot tell: {amb} of {n} elements ({amb / n:.3%}) have more than one allowed level (cap {cap:.0%})")
    eq = None if oracle is None else int((np.asarray(oracle).astype(np.float64) == got).sum())
    if record:
        s = STATS.setdefault(stage, [0, 0, 0, 0, 0, 0])
        s[0], s[1], s[4] = s[0] + n, s[1] + amb, s[4] + 1
        s[5] += int((np.broadcast_to(np.asarray(e), np.asarray(x).shape).reshape((-1,) + got.shape) == 0).all(0).sum())
        if eq is not None:
            s[2], s[3] = s[2] + n, s[3] + eq
    return {"n": n, "ambiguous": amb, "equal": eq}


def check_close(stage, case, got, x, e, oracle=None, record=True):
    """no quantiser (the normalised output, the gray mean): |got - x| <= e per element -> largest share of e used"""
    got, x, e = np.asarray(got, np.float64), np.asarray(x, np.float64), np.asarray(e, np.float64)
    d = np.abs(got - x)
    bad = ~(d <= e)
    if bad.any():
        order = np.argsort(-np.where(bad, d / np.maximum(e, 1e-300), 0), axis=None, kind="stable")[:min(16, int(bad.sum()))]
        lines = [f"{stage} [{case}]: {int(bad.sum())} of {got.size} elements outside x +- e; worst (index, x, e, got):"]
        worst = []
        for f in order:
            ix = np.unravel_index(f, got.shape)
            worst.append((tuple(int(v) for v in ix), float(got[ix]), float(x[ix])))
            lines.append(f"    {tuple(int(v) for v in ix)}  x={x[ix]:.9g}  e={np.broadcast_to(e, got.shape)[ix]:.3g}  got {got[ix]:.9g}")
        err = StrictMismatch("\n".join(lines), int(bad.sum()), {}, worst)
        err.families = [stage]
        raise err
    if record:
        s = STATS.setdefault(stage, [0, 0, 0, 0, 0, 0])
        s[0], s[4] = s[0] + got.size, s[4] + 1
        if oracle is not None:
            s[2], s[3] = s[2] + got.size, s[3] + int((np.asarray(oracle, np.float64) == got).sum())
    return float((d / np.maximum(e, 1e-300)).max()) if got.size else 0.0


def report():
    lines = ["[strict_image] stage: cases, elements, exact-class, ambiguous, equal to the fp32 oracle"]
    for k, s in STATS.items():
        eq = f"{s[3] / s[2]:.4%}" if s[2] else "-"
        lines.append(f"[strict_image]   {k:12s} {s[4]:4d} {s[0]:10d} {s[5]:10d}  {s[1] / max(s[0], 1):.4%}  {eq}")
    return "\n".join(lines)


def failing(fn):
    """-> the stages of the StrictMismatch fn() raises ([] when it passes); CannotTell is not a failure of an element"""
    try:
        fn()
    except StrictMismatch as e:
        return list(e.families)
    return []


# ---------------------------------------------------------------------------------------------- resize
def taps(in_size, out_size, mut=None):
    """taps_of + tri for every output index of one axis, in fp32 -> lo (out,), n (out,), w (out, nmax) float32, unnormalised, 0
    beyond n"""
    scale = f32(in_size) / f32(out_size)
    support = scale if scale >= 1 else f32(1)
    inv = f32(1) / scale if scale >= 1 else f32(1)
    center = scale * (np.arange(out_size, dtype=np.float32) + f32(0.5))
    lo = np.maximum(0, (center - support + f32(0.5)).astype(np.int64))
    n = np.minimum(in_size, (center + support + f32(0.5)).astype(np.int64)) - lo
    j = np.arange(int(n.max()))
    pos = np.abs(((j[None, :] + lo[:, None]).astype(np.float32) - center[:, None] + f32(0.5)) * inv)
    assert pos.dtype == np.float32
    w = np.where(pos < 1, f32(1) - pos, f32(0)).astype(np.float32)
    w[j[None, :] >= n[:, None]] = 0
    if mut == "drop_last_tap":                                # the window that reaches the last row / column loses that tap
        edge = np.nonzero((lo + n == in_size) & (n > 1))[0]
        w[edge, n[edge] - 1] = 0
    return lo, n, w


def _dyadic_bits(lo, n, w):
    """per output index: a such that the axis is dyadic (see the module docstring), -1 otherwise"""
    w64 = w.astype(np.float64)
    ws = w64.sum(1)
    a = np.full(len(lo), -1)
    for bits in range(10, -1, -1):
        ok = (np.floor(w64 * 2.0 ** bits) == w64 * 2.0 ** bits).all(1)
        a = np.where(ok, bits, a)
    m, _ = np.frexp(ws)
    single = (w64 > 0).sum(1) <= 1
    return np.where((a >= 0) & ((m == 0.5) | single), a, -1)


def _source(img, flip, mut=None):
    img = np.asarray(img)
    if not flip:
        return img
    if mut == "flip_about_w":                                 # column sx reads W - sx (clamped into the row), not W - 1 - sx
        w = img.shape[1]
        return img[:, np.minimum(w - np.arange(w), w - 1)]
    return img[:, ::-1]


def resize_ref(img, out_h, out_w, flip=False, mut=None):
    """uint8 (H, W, 3) -> (x, e) float64 (out_h, out_w, 3): the value before floor(. + 0.5) and its bound (0 on exact pixels)"""
    src = _source(img, flip, mut).astype(np.float64)
    h, w, _ = src.shape
    ax = []
    for size, out in ((h, out_h), (w, out_w)):
        lo, n, wt = taps(size, out, mut)
        m = np.zeros((out, size + wt.shape[1]))
        rows = np.repeat(np.arange(out), wt.shape[1])
        cols = (lo[:, None] + np.arange(wt.shape[1])[None, :]).reshape(-1)
        w64 = wt.astype(np.float64)
        m[rows, cols] = (w64 / w64.sum(1, keepdims=True)).reshape(-1)
        ax.append((m[:, :size], n, _dyadic_bits(lo, n, wt)))
    (my, ny, ay), (mx, nx, bx) = ax
    x = np.einsum("oh,hwc,pw->opc", my, src, mx, optimize=True)
    k = 2 * nx[None, :] + 2 * ny[:, None] + 1
    e = gamma(k) * (x + 0.5).transpose(2, 0, 1) + (nx[None, :] * ny[:, None] + 4) * U64 * 256.0
    exact = (ay[:, None] >= 0) & (bx[None, :] >= 0) & \
        (ay[:, None] + bx[None, :] + 8 + np.ceil(np.log2(nx))[None, :] + np.ceil(np.log2(ny))[:, None] <= 24)
    e = np.where(exact[None], 0.0, e).transpose(1, 2, 0)
    return x, e


def resize_levels(img, out_h, out_w, flip=False, mut=None):
    """what a kernel with defect `mut` stores (mut None: the reference's own levels)"""
    x, _ = resize_ref(img, out_h, out_w, flip, mut)
    return (q_trunc if mut == "trunc" else q_resize)(x)


def resize_kernel_order(img, out_h, out_w, flip=False, mut=None):
    """fp32 stand-in in resize_pixel's own order: 2-D, rows outer, serial weight sums, (wy * r) / wsum_x per row"""
    src = _source(img, flip, mut)
    h, w, _ = src.shape
    ly, ny, wy = taps(h, out_h, mut)
    lx, nx, wx = taps(w, out_w, mut)
    sy, sx = np.zeros(out_h, np.float32), np.zeros(out_w, np.float32)
    for j in range(wy.shape[1]):
        sy = sy + wy[:, j]
    for j in range(wx.shape[1]):
        sx = sx + wx[:, j]
    acc = np.zeros((out_h, out_w, 3), np.float32)
    for jy in range(wy.shape[1]):
        wyj = wy[:, jy] / sy
        rows = np.minimum(ly + jy, h - 1)
        r = np.zeros((out_h, out_w, 3), np.float32)
        for jx in range(wx.shape[1]):
            p = src[rows[:, None], np.minimum(lx + jx, w - 1)[None, :]].astype(np.float32)
            r = r + wx[:, jx][None, :, None] * p
        acc = acc + wyj[:, None, None] * r / sx[None, :, None]
    assert acc.dtype == np.float32
    return np.clip(np.floor(acc if mut == "trunc" else acc + f32(0.5)), 0, 255)


def resize_oracle(img, out_h, out_w, flip=False):
    """the separable fp32 oracle (oracle/image_prep.py's weights, rows then columns) for a rectangular output"""
    x = np.ascontiguousarray(_source(img, flip)).astype(np.float32)
    h, w, c = x.shape
    wy, wx = oip.aa_weights(h, out_h), oip.aa_weights(w, out_w)
    tmp = np.empty((h, out_w, c), np.float32)
    for ox, (lo, ww) in enumerate(wx):
        tmp[:, ox] = np.tensordot(x[:, lo:lo + len(ww)], ww, axes=([1], [0]))
    out = np.empty((out_h, out_w, c), np.float32)
    for oy, (lo, ww) in enumerate(wy):
        out[oy] = np.tensordot(tmp[lo:lo + len(ww)], ww, axes=([0], [0]))
    return np.clip(np.floor(out + f32(0.5)), 0, 255)


# ---------------------------------------------------------------------------------------------- colour ops
def gray_ref(lv, mut=None):
    """levels (..., 3) -> (g, e_g) before the floor"""
    lv = np.asarray(lv, np.float64)
    c0 = float(f32(0.299)) if mut == "gray_0299" else float(f32(0.2989))
    g = c0 * lv[..., 0] + float(f32(0.587)) * lv[..., 1] + float(f32(0.114)) * lv[..., 2]
    return g, gamma(3) * g + 3 * U64 * 256.0


def gray_floors(lv, mut=None, floor=True):
    g, e = gray_ref(lv, mut)
    return (np.floor(g - e), np.floor(g + e)) if floor else (g, g)


def blend_ref(a, b, ratio, swap=None):
    """a ratio + b (1 - ratio); ratio: the fp32 factor of the record.  swap: channel whose operands are exchanged (mutant)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    r = float(f32(ratio))
    om = 1.0 - r
    ra, rb = np.full(a.shape, r), np.full(a.shape, om)
    if swap is not None:
        ra[..., swap], rb[..., swap] = om, r
    t1, t2 = a * ra, b * rb
    e_om = 0.5 * float(ulp32(r)) + 0.5 * float(ulp32(om))
    e = gamma(2) * (np.abs(t1) + np.abs(t2)) + np.abs(b) * e_om * (1 + gamma(2)) + 4 * U64 * 512.0
    return t1 + t2, e


def brightness_ref(lv, ratio, mut=None):
    return blend_ref(lv, np.zeros_like(np.asarray(lv, np.float64)), ratio, 1 if mut == "swap_operands" else None)


def saturation_ref(lv, ratio, mut=None):
    """-> (x, e) of shape (2,) + lv.shape: one alternative per floor of the gray"""
    lo, hi = gray_floors(lv, mut, floor=mut != "gray_unfloored")
    outs = [blend_ref(lv, g[..., None], ratio, 1 if mut == "swap_operands" else None) for g in (lo, hi)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def gray_mean_ref(lv, mut=None):
    """levels (H, W, 3) of one image -> (lowest, highest value the device's fp32 mean may take, the float64 mean)"""
    lo, hi = gray_floors(lv, mut, floor=mut != "mean_unfloored")
    hw = lo.size
    gx = min(64, -(-hw // 256))
    t = -(-hw // (256 * gx))
    m_lo, m_hi = lo.sum() / hw, hi.sum() / hw
    e = gamma(t + 4 * gx + 5) * m_hi + 2 * U64 * 256.0
    return m_lo - e, m_hi + e, 0.5 * (m_lo + m_hi)


def contrast_ref(lv, ratio, mut=None, mean=None):
    """-> (x, e) of shape (2,) + lv.shape: the blend at both ends of the mean's interval (mean: that interval, if given)"""
    m_lo, m_hi, _ = gray_mean_ref(lv, mut) if mean is None else mean
    outs = [blend_ref(lv, np.full(np.shape(lv), m), ratio, 1 if mut == "swap_operands" else None) for m in (m_lo, m_hi)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


HUE_K = float(f32(255) + f32(1) - f32(1e-3))


def _hue_core(rgb, f, mut=None):
    """hue_shift in rgb's own dtype (float64: the reference; float32: a stand-in) -> (ro k, go k, bo k stacked, v, s)"""
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    eqc = maxc == minc
    cr = maxc - minc
    s = cr / np.where(eqc, 1.0, maxc)
    crd = np.where(eqc, 1.0, cr)
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    hr = np.where(maxc == r, bc - gc, 0.0)
    hg = np.where((maxc == g) & (maxc != r), 2.0 + rc - bc, 0.0)
    hb = np.where((maxc != g) & (maxc != r), 4.0 + gc - rc, 0.0)
    h = np.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0) + float(f32(f))
    neg = h < 0
    h = np.where(neg, h, h - np.floor(h)) if mut == "hue_nowrap" else h - np.floor(h)
    h6 = h * 6.0
    fi = np.floor(h6)
    ff = h6 - fi
    i = fi.astype(np.int64) % 6
    if mut == "hue_nowrap":                                   # C's % keeps the sign: a negative sector takes the default branch
        i = np.where(neg, 5, i)
    v = maxc
    p = np.clip(v * (1 - s), 0, 1)
    q = np.clip(v * (1 - s * ff), 0, 1)
    t = np.clip(v * (1 - s * (1 - ff)), 0, 1)
    ro = [v, p, q, p, t, v] if mut == "hue_swap" else [v, q, p, p, t, v]
    k = 255.0 if mut == "k255" else HUE_K
    x = np.stack([np.choose(i, ro), np.choose(i, [t, v, v, q, p, p]), np.choose(i, [p, p, t, v, v, q])], -1) * k
    assert x.dtype == rgb.dtype
    return x, v, s


def hue_ref(lv, f, mut=None):
    """levels (..., 3), f the fp32 factor -> (x, e): ro k, go k, bo k before the floor"""
    c255 = f32(1) / f32(255)
    x, v, s = _hue_core((np.asarray(lv).astype(np.float32) * c255).astype(np.float64), f, mut)
    e = HUE_K * v * (s * 54 * U + 7 * U) / (1 - 64 * U) + 40 * U64 * 256.0
    return x, np.broadcast_to(e[..., None], x.shape).copy()


def op_f32(op, lv, factor, mut=None):
    """fp32 stand-in of one colour op with defect `mut` (mut None: the oracle's arithmetic); factor: the double"""
    a = np.asarray(lv).astype(np.float32)
    if op == 3:
        return np.floor(_hue_core(a * (f32(1) / f32(255)), factor, mut)[0]).astype(np.float32)
    c0 = f32(0.299) if mut == "gray_0299" else f32(0.2989)
    g = c0 * a[..., 0] + f32(0.587) * a[..., 1] + f32(0.114) * a[..., 2]
    if op == 0:
        b = np.zeros_like(a)
    elif op == 1:
        b = np.full_like(a, f32((g if mut == "mean_unfloored" else np.floor(g)).mean(dtype=np.float64)))
    else:
        b = np.broadcast_to((g if mut == "gray_unfloored" else np.floor(g))[..., None], a.shape)
    ra, rb = np.full(a.shape, f32(factor)), np.full(a.shape, f32(1.0 - factor))
    if mut == "swap_operands":
        ra[..., 1], rb[..., 1] = rb[..., 1].copy(), ra[..., 1].copy()
    return np.floor(np.clip(a * ra + b * rb, 0, 255)).astype(np.float32)


def normalise_ref(lv, mean, std, dtype):
    """levels (..., 3) -> (x, e) of the stored (level / 255 - mean) / std in `dtype`"""
    c255 = float(f32(1) / f32(255))
    m, s = np.asarray(mean, np.float32).astype(np.float64), np.asarray(std, np.float32).astype(np.float64)
    y = np.asarray(lv, np.float64) * c255
    d = y - m
    x = d / s
    e1 = (U * np.abs(y) + U * np.abs(d)) / np.abs(s) + U * np.abs(x) + 4 * U64 * 16.0
    return x, e1 + 0.5 * ulp(torch.as_tensor(np.abs(x) + e1), dtype).numpy()


def normalise_f32(lv, mean, std, dtype, mut=None):
    """fp32 stand-in of the final store -> float64 array of the values of `dtype`"""
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    if mut == "std_perm":
        s = np.roll(s, 1)
    v = torch.from_numpy(((np.asarray(lv).astype(np.float32) * (f32(1) / f32(255)) - m) / s).astype(np.float32))
    if mut == "bf16_trunc":
        v = (v.view(torch.int32) & -65536).view(torch.float32)
    return v.to(dtype).to(torch.float64).numpy()


# stage name -> (reference, quantiser); the levels a kernel with defect `mut` stores
REFS = {"brightness": brightness_ref, "contrast": contrast_ref, "saturation": saturation_ref, "hue": hue_ref}
OPS = ("brightness", "contrast", "saturation", "hue")


def op_levels(op, lv, factor, mut=None):
    x, _ = REFS[OPS[op]](lv, factor, mut)
    return q_floor(x[0] if x.ndim > np.ndim(lv) else x)


def op_oracle(op, lv, factor):
    """the fp32 oracle's stage; factor: the DOUBLE the record's fp32 ratio was rounded from"""
    x = np.asarray(lv).astype(np.float32)
    if op == 0:
        return oip._blend(x, f32(0), factor)
    if op == 1:
        return oip._blend(x, f32(oip._gray(x).mean(dtype=np.float64)), factor)
    if op == 2:
        return oip._blend(x, oip._gray(x)[..., None], factor)
    return oip._hue(x, factor)


def check_op(op, case, lv_in, factor, got, oracle=True, record=True, mean=None, cap=CAP_COLOUR):
    """one colour op from its exact input levels (H, W, 3) -> the comparator's dict"""
    x, e = REFS[OPS[op]](lv_in, factor, **({"mean": mean} if op == 1 and mean is not None else {}))
    return check_levels(OPS[op], case, got, x, e, q_floor, cap, op_oracle(op, lv_in, factor) if oracle else None, record)


def pipeline(img, size, flip=False, order=(), factors=(1.0, 1.0, 1.0, 0.0), mean=oip.MEAN, std=oip.STD, dtype=F32, mut=None):
    """the whole transform in fp32 (the resize in the kernel's order, op_f32, normalise_f32) with defect `mut` in its stage
    -> float64 (3, size, size)"""
    lv = resize_kernel_order(img, size, size, flip, mut)
    for op in order:
        lv = op_f32(op, lv, factors[op], mut)
    return normalise_f32(lv, mean, std, dtype, mut).transpose(2, 0, 1)


# ---------------------------------------------------------------------------------------------- inputs and cases
RESIZE_CASES = [(333, 500, 64), (17, 301, 64), (1000, 750, 32), (37, 23, 264), (1, 9, 16), (9, 1, 16), (128, 128, 64), (64, 64, 64)]
EXACT_CASES = [(128, 128, 64), (64, 64, 64), (1, 9, 16), (9, 1, 16)]
BLEND_FACTORS = (0.8137, 0.9329, 1.0713, 1.1871)
HUE_FACTORS = (-0.3137, -0.0871, 0.0, 0.0613, 0.4127)
ORDERS = [(0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2), (2, 0, 3, 1), (0, 2, 1, 3), (3, 0, 1, 2), (1, 0, 2, 3), (2, 3, 0, 1)]
CHAIN_FACTORS = (0.8137, 1.1871, 0.9329, -0.0871)             # indexed by op


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def impulses(h, w):
    """one 255 pixel on black: the four corners, the middle of the last row and of the last column"""
    out = []
    for y, x in dict.fromkeys([(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h - 1, w // 2), (h // 2, w - 1)]):
        im = np.zeros((h, w, 3), np.uint8)
        im[y, x] = 255
        out.append(im)
    return out


@functools.lru_cache(maxsize=None)
def resize_case(h, w, s):
    """-> (images, records): two noise images back to back (the second at an odd offset when h w is odd), then the impulses;
    records = (image index, flip), each image without and with flip"""
    images = [noise(h, w, 100 + h), noise(h, w, 200 + w)] + impulses(h, w)
    return images, [(i, fl) for i in range(len(images)) for fl in (False, True)]


@functools.lru_cache(maxsize=None)
def resize_case_ref(h, w, s):
    images, recs = resize_case(h, w, s)
    return [resize_ref(images[i], s, s, fl) for i, fl in recs]


@functools.lru_cache(maxsize=None)
def resize_case_oracle(h, w, s):
    images, recs = resize_case(h, w, s)
    return [resize_oracle(images[i], s, s, fl) for i, fl in recs]


def lattice_levels():
    """the 64 levels: 0-3, 126-129, 252-255 and 52 spread over the rest"""
    rng = np.random.default_rng(64)
    rest = np.array([v for v in range(4, 252) if not 126 <= v <= 129])
    return np.sort(np.concatenate([[0, 1, 2, 3, 126, 127, 128, 129, 252, 253, 254, 255], rng.choice(rest, 52, replace=False)]))


@functools.lru_cache(maxsize=None)
def lattice():
    """uint8 (512, 512, 3): every triple of the 64 levels"""
    lv = lattice_levels().astype(np.uint8)
    r, g, b = np.meshgrid(lv, lv, lv, indexing="ij")
    return np.ascontiguousarray(np.stack([r, g, b], -1).reshape(512, 512, 3))


def small_image():
    return noise(50, 50, 50)                                  # hw = 2500: gx = 10, the grid-stride tail


def chain_image():
    return noise(64, 64, 64)


def smooth_images(seed, sizes):
    """the images of tests/test_gpu_input_pipeline.py and tests/test_gpu_mosaic.py (smooth content + noise)"""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in sizes:
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([127 + 100 * np.sin(xx / (7.0 + c) + yy / 13.0) for c in range(3)], -1)
        out.append(np.clip(base + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8))
    return out


# mosaic: sources (H, W) and two records; tile k = (source, flip, tw, th, x0, y0) as tests/mosaic_ref.py takes them
MOSAIC_S = 64
MOSAIC_SOURCES = [(37, 23), (17, 301), (48, 40), (64, 64)]
MOSAIC_RECORDS = [
    # non-square tiles; tile 0 flipped and starting left of and above the canvas (clipped by its quadrant); quadrant 3 empty
    {"cx": 29, "cy": 35, "tiles": [(0, True, 41, 50, -12, -15), (1, False, 35, 9, 29, 26), (2, False, 23, 29, 6, 35), None]},
    # tile 1 wider than its quadrant, tile 3 the 64 x 64 image itself (identity scale) clipped on both axes
    {"cx": 40, "cy": 22, "tiles": [(3, False, 32, 20, 8, 2), (2, True, 30, 17, 40, 5), (0, False, 19, 42, 21, 22), (3, False, 64, 64, 40, 22)]},
]


@functools.lru_cache(maxsize=None)
def mosaic_sources():
    return [noise(h, w, 300 + i) for i, (h, w) in enumerate(MOSAIC_SOURCES)]


def mosaic_ref_canvas(images, record, size, fill):
    """-> (x, e) float64 (size, size, 3) of one mosaic output before the resize's quantiser: a fill pixel is the fill level with
    e = 0, a tile pixel the resize reference of its tile at (th, tw); tests/mosaic_ref.py says which pixel is which tile's"""
    import mosaic_ref
    x, e = np.full((size, size, 3), float(fill)), np.zeros((size, size, 3))
    for k, t in enumerate(record["tiles"]):
        if t is None:
            continue
        one = {"cx": record["cx"], "cy": record["cy"], "tiles": [t if j == k else None for j in range(4)]}
        ys, xs = np.nonzero(~mosaic_ref.mosaic_canvas(images, one, size, fill)[1])
        src, flip, tw, th, x0, y0 = t
        tx, te = resize_ref(images[src], th, tw, flip)
        x[ys, xs], e[ys, xs] = tx[ys - y0, xs - x0], te[ys - y0, xs - x0]
    return x, e
