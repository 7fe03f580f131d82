"""Numpy restatement of the affine warp's contract (test infrastructure; src/data/transforms.py, csrc/image_prep.hip::k_affine).

Coordinates are continuous: pixel i covers [i, i + 1), its centre is i + 0.5 (not OpenCV's integer centres), so pixels and boxes
share one system.  A record is the six fp32 values (a00, a01, b0, a10, a11, b1) of the INVERSE map, canvas <- output.  Output
pixel (ox, oy) samples the canvas at u = a00 (ox + 0.5) + a01 (oy + 0.5) + b0 - 0.5, v likewise: bilinear between the four
pixel centres around (u, v), a tap outside the canvas being the fill level, floor(x + 0.5), clip.  `warp_f32` does that in
the kernel's own fp32 operation order; `mut=` plants one defect.  The colour ops and the normalisation behind the warp are
oracle/image_prep.py's (`mosaic_ref.finish`)."""
import math

import numpy as np
import torch

import mosaic_ref

f32 = np.float32
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
MUTANTS = ["integer_centre", "transposed", "nearest", "replicate", "trunc"]


def forward_matrix(draw, S):
    """The forward matrix of a draw (angle, gain, shear x, shear y, tx, ty), composed step by step from what each step does to
    the three points (0, 0), (1, 0), (0, 1) -- independent of src/data/transforms.py::affine_matrix's matrix products."""
    angle, gain, shx, shy, tx, ty = (float(v) for v in draw)
    a, kx, ky = math.radians(angle), math.tan(math.radians(shx)), math.tan(math.radians(shy))

    def step(x, y):
        x, y = x - S / 2, y - S / 2                                                          # C
        x, y = gain * (x * math.cos(a) - y * math.sin(a)), gain * (x * math.sin(a) + y * math.cos(a))    # R
        x, y = x + kx * y, ky * x + y                                                        # Sh
        return x + tx * S, y + ty * S                                                        # T
    o, ex, ey = step(0.0, 0.0), step(1.0, 0.0), step(0.0, 1.0)
    return np.array([[ex[0] - o[0], ey[0] - o[0], o[0]], [ex[1] - o[1], ey[1] - o[1], o[1]]])


def inverse_record(m):
    """Forward 2 x 3 -> the six fp32 values of the inverse, by numpy's solver on the 3 x 3 form."""
    inv = np.linalg.inv(np.vstack([np.asarray(m, np.float64), [0.0, 0.0, 1.0]]))
    return tuple(float(v) for v in inv[:2].astype(np.float32).reshape(-1))


def coords_f32(rec, S, mut=None):
    """u, v (S, S) float32 in the kernel's order: ((a00 px + a01 py) + b0) - 0.5f with px = ox + 0.5f, py = oy + 0.5f"""
    a00, a01, b0, a10, a11, b1 = (f32(v) for v in rec)
    if mut == "transposed":
        a01, a10 = a10, a01
    half = f32(0.0) if mut == "integer_centre" else f32(0.5)
    px = (np.arange(S, dtype=np.float32) + half)[None, :]
    py = (np.arange(S, dtype=np.float32) + half)[:, None]
    u = ((a00 * px + a01 * py) + b0) - half
    v = ((a10 * px + a11 * py) + b1) - half
    assert u.dtype == np.float32 and v.dtype == np.float32
    return u, v


def warp_f32(canvas, rec, fill=114, mut=None):
    """canvas: levels (S, S, 3); rec: the six fp32 values -> float32 levels (S, S, 3), k_affine's operations in its order"""
    canvas = np.asarray(canvas).astype(np.float32)
    S = canvas.shape[0]
    u, v = coords_f32(rec, S, mut)
    inside = (u >= f32(-1)) & (u < f32(S)) & (v >= f32(-1)) & (v < f32(S))
    us, vs = np.where(inside, u, f32(0)), np.where(inside, v, f32(0))
    xf, yf = np.floor(us), np.floor(vs)
    fx, fy = (us - xf)[..., None], (vs - yf)[..., None]
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    if mut == "nearest":
        fx, fy = np.where(fx >= f32(0.5), f32(1), f32(0)), np.where(fy >= f32(0.5), f32(1), f32(0))

    def tap(y, x):
        ok = (x >= 0) & (x < S) & (y >= 0) & (y < S)
        p = canvas[np.clip(y, 0, S - 1), np.clip(x, 0, S - 1)]
        return p if mut == "replicate" else np.where(ok[..., None], p, f32(fill))
    p00, p01, p10, p11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    top, bot = p00 + fx * (p01 - p00), p10 + fx * (p11 - p10)
    acc = np.where(inside[..., None], top + fy * (bot - top), f32(fill))
    assert acc.dtype == np.float32
    return np.clip(np.floor(acc if mut == "trunc" else acc + f32(0.5)), 0, 255)


def outside(rec, S):
    """bool (S, S): all four taps of the pixel lie outside the canvas, decided in float64 with a margin of 2^-10 pixel on
    either side left undecided (False) -- those pixels are `fill` exactly whatever the kernel's fp32 u, v round to"""
    a00, a01, b0, a10, a11, b1 = (float(f32(v)) for v in rec)
    px, py = (np.arange(S) + 0.5)[None, :], (np.arange(S) + 0.5)[:, None]
    u, v = a00 * px + a01 * py + b0 - 0.5, a10 * px + a11 * py + b1 - 0.5
    m = 2.0 ** -10
    return (u < -1 - m) | (u > S + m) | (v < -1 - m) | (v > S + m)


def affine_boxes(m, boxes5, S, min_box=2.0, min_visible=0.1, max_aspect=100.0, max_boxes=128):
    """The box rule, float32, one box at a time: corners through the forward matrix, hull, clip to [0, S]; keep on clipped
    w', h' >= min_box, w'h' / (w h |det| + 1e-9) >= min_visible and max(w'/h', h'/w') < max_aspect; order kept; over max_boxes
    the largest clipped areas stay (ties: the earlier box).  -> float32 (M, 5)"""
    m = np.asarray(m, np.float64).astype(np.float32)
    det = f32(abs(f32(f32(m[0, 0] * m[1, 1]) - f32(m[0, 1] * m[1, 0]))))
    rows, areas = [], []
    for x, y, w, h, lab in np.asarray(boxes5, np.float32).reshape(-1, 5):
        xs, ys = [], []
        for cx, cy in ((x, y), (f32(x + w), y), (x, f32(y + h)), (f32(x + w), f32(y + h))):
            xs.append(f32(f32(f32(m[0, 0] * cx) + f32(m[0, 1] * cy)) + m[0, 2]))
            ys.append(f32(f32(f32(m[1, 0] * cx) + f32(m[1, 1] * cy)) + m[1, 2]))
        x1, x2 = min(max(min(xs), f32(0)), f32(S)), min(max(max(xs), f32(0)), f32(S))
        y1, y2 = min(max(min(ys), f32(0)), f32(S)), min(max(max(ys), f32(0)), f32(S))
        cw, ch = f32(x2 - x1), f32(y2 - y1)
        if not (cw >= min_box and ch >= min_box and cw > 0 and ch > 0):
            continue
        if f32(cw * ch) / f32(f32(f32(w * h) * det) + f32(1e-9)) >= min_visible and max(f32(cw / ch), f32(ch / cw)) < max_aspect:
            rows.append([x1, y1, cw, ch, lab])
            areas.append(f32(cw * ch))
    if len(rows) > max_boxes:
        order = sorted(range(len(rows)), key=lambda j: -float(areas[j]))[:max_boxes]       # sorted() is stable
        rows = [rows[j] for j in sorted(order)]
    return torch.from_numpy(np.asarray(rows, np.float32).reshape(-1, 5))


def image_prep_affine(src_u8, recs, tiles, affine, size, fill, jitter, dtype, mean, std):
    """CPU stand-in of ops.image_prep_affine (same arguments): the canvas of the plain resize (tiles None) or of the mosaic,
    warped by warp_f32, then the colour ops and the normalisation."""
    by_off = {int(r[0]): j for j, r in enumerate(recs)}
    images = [src_u8[off:off + h * w * 3].reshape(h, w, 3).numpy() for off, h, w, _, _, _ in recs]
    outs = []
    for i, (off, h, w, flip, order, fac) in enumerate(recs):
        if tiles is None:
            rec = mosaic_ref.plain_record(i, flip, size)
        else:
            cx, cy, quad = tiles[i]
            rec = {"cx": cx, "cy": cy, "tiles": [(by_off[int(t[0])], t[3], t[4], t[5], t[6], t[7]) if t is not None else None
                                                 for t in quad]}
        canvas = mosaic_ref.mosaic_canvas(images, rec, size, fill)[0]
        outs.append(mosaic_ref.finish(warp_f32(canvas, affine[i], fill), tuple(order) if jitter else (), fac, mean, std))
    return torch.stack(outs).to(dtype)

