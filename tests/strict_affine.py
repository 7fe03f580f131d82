"""Strict per-pixel comparator for the affine warp of the on-device input pipeline (csrc/image_prep.hip::k_affine): a float64
restatement taken from the SAME uint8 canvas the kernel read and the same six fp32 values of its record, a derived bound per
element and, because the warp ends in the resize's quantiser q(v) = clamp(floor(v + 0.5), 0, 255), a SET of allowed uint8
levels per element (strict_image.check_levels; u = 2^-24, gamma_n, CAP_RESIZE = 2 % and CannotTell are that module's).  Shared
by tests/test_affine_cpu.py (the proof of the comparator, no GPU) and tests/test_gpu_affine.py (the kernel).

The surface.  With the canvas extended by the fill level on all sides, F(u, v) is the bilinear interpolant between the pixel
centres: continuous, piecewise bilinear on the unit cells [i, i + 1] x [j, j + 1], constant = fill outside [-1, S] x [-1, S].
The kernel's range test, its floor and its border rule are one way of evaluating F (a pixel whose u is put into the
neighbouring cell by a rounding, or to the fill side of the range test, is still a value of F at the rounded u), so all that
separates the kernel from x = F(u, v) is the rounding of u, v and of the blend.

Coordinates.  The kernel forms u = ((a00 px + a01 py) + b0) - 0.5f with px = ox + 0.5f, py = oy + 0.5f (exact for ox < 2^23), one
rounding per operation.  The reference forms the same five intermediates t1, t2, s1, s2, u in float64 from the fp32 record
(products of a 24-bit and an 11-bit number are exact; each float64 sum adds 2^-53 relative, carried as a U64 term).  Each fp32
rounding is half an ulp32 at the magnitude of the value rounded, which differs from the float64 one by the error so far:
    d1 = h(t1) + h(t2), d2 = d1 + h(|s1| + d1), d3 = d2 + h(|s2| + d2), du = d3 + h(|u| + d3),   h(x) = ulp32(x) / 2
fx = u - floor(u) is exact for u >= 0 and rounds once, by at most 2^-24, for u in [-1, 0): du += 2^-24.  v likewise.
A coordinate is EXACT (du = 0) when all five float64 intermediates are representable in fp32: then no fp32 operation rounds.

Propagation.  Moving from (u, v) to the kernel's (u~, v~), first along u, then along v, stays inside the cells that
[u - du, u + du] x [v - dv, v + dv] touches (at most two per axis: du < 1/2 is asserted).  Inside a cell dF/du lies between
the two horizontal neighbour differences of its corners and dF/dv between the two vertical ones, so
    |F(u~, v~) - F(u, v)| <= du Dh + dv Dv,     Dh, Dv = the largest horizontal / vertical neighbour difference among the
corners of the touched cells, per channel, border cells having fill as the neighbour.

Blend.  top = p00 + fx (p01 - p00): the difference of two levels is exact, the product and the sum round (2 roundings at <=
255); bot alike; acc = top + fy (bot - top): three more; acc + 0.5f: one.  acc is a convex combination of top and bot, so their
errors enter once: e_blend = gamma_6 * 256.
    e = du Dh + dv Dv + e_blend        (+ the float64 evaluation's own 2^-53 terms)

Exact elements (e = 0: one level, ties included, outside any cap).  (a) Dh = Dv = 0: all corners of the touched cells are one
level p, and p + fx 0 = p, p + fy 0 = p, floor(p + 0.5) = p in any rounding -- this is every pixel whose four taps lie outside
(fill, exactly) and every flat patch.  (b) u and v exact with fx, fy multiples of 2^-7: top, bot are multiples of 2^-7 and acc
of 2^-14, all below 2^9, exact in 24 bits.  (b) holds for the identity, integer shifts, mirrors and quarter turns about the
centre (fx = fy = 0: the pixel is the tap itself) and half-pixel shifts (fx = 1/2).

Mutants (affine_ref.MUTANTS, each planted in affine_ref.warp_f32): integer-centre coordinates, a transposed matrix, nearest
neighbour, a replicated border, truncation.  Observed on the device: OBSERVED_GPU."""
import functools

import numpy as np

import affine_ref
import strict_image as si
from strict_image import CAP_RESIZE, U, U64, CannotTell, StrictMismatch, failing, gamma, q_resize, ulp32  # noqa: F401

f32 = np.float32
FILL = 114
OBSERVED_GPU = """MI355X, tests/test_gpu_affine.py, 2026-10-20 (12 tests, 3.5 s of which the captured training run 2.8 s), share ambiguous / share
equal to the fp32 restatement: general records 0.062 % / 100 % (36 cases: nine records x S = 96, 33 x plain and mosaic canvases, 556 470
elements, 236 120 of them exact class -- fill and flat patches; worst case S = 33 translate_hi 0.98 %), exact-class records 0 / 100 % (18
cases, 278 235 elements, all equal to the numpy index arithmetic); the sampled path mosaic + warp + four colour ops (S = 64, 8 outputs)
99.997 % of all elements exact, none more than 1 level off (the contract allows 97 % / 6); nothing outside its set"""


def _h(x):
    return 0.5 * ulp32(np.array(x, np.float64))


def _representable(x):
    with np.errstate(over="ignore"):
        return x.astype(np.float32).astype(np.float64) == x


def coord_ref(a0, a1, b, S):
    """one row of the record -> (u float64 (S, S), du, exact bool)"""
    a0, a1, b = float(f32(a0)), float(f32(a1)), float(f32(b))
    px, py = (np.arange(S) + 0.5)[None, :], (np.arange(S) + 0.5)[:, None]
    t1, t2 = np.broadcast_to(a0 * px, (S, S)), np.broadcast_to(a1 * py, (S, S))
    s1 = t1 + t2
    s2 = s1 + b
    u = s2 - 0.5
    d = _h(t1) + _h(t2)
    d = d + _h(np.abs(s1) + d)
    d = d + _h(np.abs(s2) + d)
    d = d + _h(np.abs(u) + d)
    d = d + U + 8 * U64 * (np.abs(t1) + np.abs(t2) + abs(b) + 0.5)
    exact = _representable(t1) & _representable(t2) & _representable(s1) & _representable(s2) & _representable(u)
    return u, np.where(exact, 0.0, d), exact


def _dyadic7(f):
    return np.floor(f * 128.0) == f * 128.0


def affine_ref_levels(canvas, rec, fill=FILL):
    """canvas: levels (S, S, 3) as the kernel read them; rec: the six fp32 values -> (x, e) float64 (S, S, 3): the value before
    floor(. + 0.5) and its bound (0 on exact elements)"""
    canvas = np.asarray(canvas, np.float64)
    S = canvas.shape[0]
    P = np.full((S + 4, S + 4, 3), float(fill))                 # P[y + 2, x + 2] = pixel (x, y); index range -2 .. S + 1
    P[2:S + 2, 2:S + 2] = canvas
    u, du, eu = coord_ref(rec[0], rec[1], rec[2], S)
    v, dv, ev = coord_ref(rec[3], rec[4], rec[5], S)
    assert du.max() < 0.5 and dv.max() < 0.5, "the record is too large for this canvas: a coordinate is uncertain by half a pixel"
    lim = lambda t: np.clip(t, -2.0, S + 1.0)                   # F is constant (fill) beyond: the outermost cells are flat
    cell = lambda t: np.clip(np.floor(lim(t)), -2, S).astype(np.int64)

    def corners(cx, cy):
        return P[cy + 2, cx + 2], P[cy + 2, cx + 3], P[cy + 3, cx + 2], P[cy + 3, cx + 3]
    cx, cy = cell(u), cell(v)
    fx, fy = (lim(u) - cx)[..., None], (lim(v) - cy)[..., None]
    p00, p01, p10, p11 = corners(cx, cy)
    top, bot = p00 + fx * (p01 - p00), p10 + fx * (p11 - p10)
    x = top + fy * (bot - top)
    dh, dvv = np.zeros_like(x), np.zeros_like(x)
    for gx in (cell(u - du), cell(u + du)):
        for gy in (cell(v - dv), cell(v + dv)):
            q00, q01, q10, q11 = corners(gx, gy)
            dh = np.maximum(dh, np.maximum(np.abs(q01 - q00), np.abs(q11 - q10)))
            dvv = np.maximum(dvv, np.maximum(np.abs(q10 - q00), np.abs(q11 - q01)))
    e = du[..., None] * dh + dv[..., None] * dvv + gamma(6) * 256.0 + 8 * U64 * 512.0
    flat = (dh == 0) & (dvv == 0)
    dyadic = (eu & ev & _dyadic7(fx[..., 0]) & _dyadic7(fy[..., 0]))[..., None]
    return x, np.where(flat | dyadic, 0.0, e)


def check_warp(case, got, canvas, rec, fill=FILL, cap=CAP_RESIZE, record=True, stage="affine"):
    """got: levels (S, S, 3) -> the comparator's dict; the oracle is the fp32 restatement in the kernel's order"""
    x, e = affine_ref_levels(canvas, rec, fill)
    return si.check_levels(stage, case, got, x, e, q_resize, cap, affine_ref.warp_f32(canvas, rec, fill), record)


# ---------------------------------------------------------------------------------------------- inputs and cases
SIZES = (96, 33)
# general records, as draws (angle, gain, shear x, shear y, tx, ty)
GENERAL = {
    "rot10": (10.0, 1.0, 0.0, 0.0, 0.5, 0.5),
    "rot137": (137.0, 1.0, 0.0, 0.0, 0.5, 0.5),
    "gain0.5": (0.0, 0.5, 0.0, 0.0, 0.5, 0.5),
    # off the centre: centred, the inverse scale 2/3 puts fx and fy on 1/6, 1/2, 5/6 and 7.6 % of all elements of ANY canvas on an
    # exact tie k + 1/2, where an inexact u leaves two levels; the same gain with a generic offset has no such lattice
    "gain1.5": (0.0, 1.5, 0.0, 0.0, 0.53, 0.47),
    "shear8": (0.0, 1.0, 8.0, 8.0, 0.5, 0.5),
    "translate_lo": (0.0, 1.0, 0.0, 0.0, 0.4, 0.4),
    "translate_hi": (0.0, 1.0, 0.0, 0.0, 0.6, 0.6),
    "combined": (-23.0, 0.8, 5.0, -7.0, 0.57, 0.44),
    "pushed_out": (0.0, 1.0, 0.0, 0.0, 2.25, 0.5),            # the whole canvas lands right of the output: all fill
}


def exact_matrices(S):
    """forward 2 x 3 matrices whose every pixel is in the exact class, with the numpy index arithmetic that states the result:
    name -> (matrix, function canvas (S, S, 3) -> levels (S, S, 3))"""
    def shift(c, dx, dy, fill=FILL):
        out = np.full_like(c, fill)
        ys, xs = np.mgrid[0:S, 0:S]
        sy, sx = ys - dy, xs - dx
        ok = (sy >= 0) & (sy < S) & (sx >= 0) & (sx < S)
        out[ys[ok], xs[ok]] = c[sy[ok], sx[ok]]
        return out

    def half(c, fill=FILL):                                     # output x shows the mean of canvas x - 1 and x, ties up
        p = np.concatenate([np.full((S, 1, 3), fill, c.dtype), c], 1).astype(np.int64)
        return ((p[:, :-1] + p[:, 1:] + 1) // 2).astype(c.dtype)
    return {
        "identity": ([[1, 0, 0], [0, 1, 0]], lambda c: c),
        "shift+7-5": ([[1, 0, 7], [0, 1, -5]], lambda c: shift(c, 7, -5)),
        "turn90": ([[0, -1, S], [1, 0, 0]], lambda c: np.rot90(c, -1)),       # (x, y) -> (S - y, x)
        "turn180": ([[-1, 0, S], [0, -1, S]], lambda c: c[::-1, ::-1]),
        "turn270": ([[0, 1, 0], [-1, 0, S]], lambda c: np.rot90(c, 1)),       # (x, y) -> (y, S - x)
        "half_pixel": ([[1, 0, 0.5], [0, 1, 0]], half),
        "mirror_x": ([[-1, 0, S], [0, 1, 0]], lambda c: c[:, ::-1]),
    }


@functools.lru_cache(maxsize=None)
def canvas(S, kind):
    """a uint8 canvas (S, S, 3) for the CPU proof: 'noise' (every neighbour difference large) or 'smooth' (photograph-like)"""
    if kind == "noise":
        return si.noise(S, S, 700 + S)
    return si.smooth_images(40 + S, [(S, S)])[0]


@functools.lru_cache(maxsize=None)
def general_record(name, S):
    return affine_ref.inverse_record(affine_ref.forward_matrix(GENERAL[name], S))
