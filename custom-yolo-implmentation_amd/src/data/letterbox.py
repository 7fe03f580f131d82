"""Letterbox geometry of `Model.predict` (host side, pure Python; no reference counterpart: the reference's
`Model.inference`, src/model/model_builder.py:115-139, stretches a picture to 640 x 640).

A picture of H x W pixels goes onto a square canvas of S x S: resized by one gain r = min(S / H, S / W) to the INTEGER size
(nh, nw), centred, the bars filled with the level `FILL`.  Because the resize goes to an integer size, the exact inverse of
what the resize kernel did is the per-axis ratio (W / nw, H / nh), not the common gain r: a detection at canvas x maps back to
(x - left) * (W / nw).  `csrc/image_prep.hip::k_letterbox` places the picture by this record and
`csrc/decode_nms.hip::k_rows_to_source` maps the rows back by it."""
import math

import numpy as np

FILL = 114


def letterbox_geometry(H, W, S, scaleup=True):
    """-> (nw, nh, left, top, sx, sy), computed in Python floats (double):
        r    = min(S / H, S / W);  if not scaleup: r = min(r, 1.0)
        nw   = min(S, max(1, floor(W * r + 0.5)));   nh likewise from H
        left = (S - nw) // 2;                        top = (S - nh) // 2
        sx   = float32(W / nw);                      sy = float32(H / nh)     (the double quotient, rounded once)
    H = W = S gives (S, S, 0, 0, 1.0, 1.0)."""
    H, W, S = int(H), int(W), int(S)
    if H < 1 or W < 1 or S < 1:
        raise ValueError(f"letterbox_geometry: a picture and a canvas have at least one pixel, got H={H} W={W} S={S}")
    r = min(S / H, S / W)
    if not scaleup:
        r = min(r, 1.0)
    nw = min(S, max(1, math.floor(W * r + 0.5)))
    nh = min(S, max(1, math.floor(H * r + 0.5)))
    left, top = (S - nw) // 2, (S - nh) // 2
    return nw, nh, left, top, float(np.float32(W / nw)), float(np.float32(H / nh))


def letterbox_records(sizes, S, scaleup=True, slots=None):
    """The records of `ops.letterbox` for pictures of `sizes` [(H, W)] packed back to back (uint8 HWC):
    [(off, H, W, nw, nh, left, top, sx, sy)], padded with blank slots (nw = nh = 0: all fill, nothing read) up to `slots`;
    -> (records, bytes used)."""
    recs, off = [], 0
    for h, w in sizes:
        recs.append((off, int(h), int(w)) + letterbox_geometry(h, w, S, scaleup))
        off += int(h) * int(w) * 3
    for _ in range(len(recs), slots if slots is not None else 0):
        recs.append((0, 0, 0, 0, 0, 0, 0, 1.0, 1.0))
    return recs, off
