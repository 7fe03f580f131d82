"""Numpy restatement of the mosaic contract (test infrastructure; src/data/transforms.py, csrc/image_prep.hip::k_mosaic).

A geometry record is {"cx", "cy", "tiles": four (source index, flip, tw, th, x0, y0), or None for no tile}: tile k is image `source`, optionally
mirrored, resized to (th, tw) with the separable antialiased bilinear filter of oracle/image_prep.py (`aa_weights` per axis,
rows then columns, floor(x + 0.5), clip), placed with its pixel (0, 0) at canvas (x0, y0).  Canvas pixel (ox, oy) belongs to
quadrant (ox >= cx) + 2 (oy >= cy); inside that quadrant's tile rectangle it shows the tile, elsewhere the fill level.  The
colour ops and the normalisation are oracle/image_prep.py's, applied to the finished canvas."""
import numpy as np
import torch

from oracle import image_prep as oip


def plain_record(i, flip, S):
    """The record that describes the plain resize of image i: the centre in the bottom-right corner, tile 0 = the canvas."""
    return {"cx": S, "cy": S, "tiles": [(i, flip, S, S, 0, 0)]}


def resize_tile(img_u8_hwc, flip, th, tw):
    """uint8 (H, W, 3) -> float32 levels (th, tw, 3)."""
    x = np.asarray(img_u8_hwc).astype(np.float32)
    if flip:
        x = np.ascontiguousarray(x[:, ::-1])
    h, w, c = x.shape
    wy, wx = oip.aa_weights(h, th), oip.aa_weights(w, tw)
    tmp = np.empty((h, tw, c), np.float32)
    for ox, (lo, ww) in enumerate(wx):
        tmp[:, ox] = np.tensordot(x[:, lo:lo + len(ww)], ww, axes=([1], [0]))
    out = np.empty((th, tw, c), np.float32)
    for oy, (lo, ww) in enumerate(wy):
        out[oy] = np.tensordot(tmp[lo:lo + len(ww)], ww, axes=([0], [0]))
    return np.clip(np.floor(out + np.float32(0.5)), 0, 255)


def mosaic_canvas(images, record, S, fill=114):
    """-> (canvas float32 levels (S, S, 3), bool (S, S): the pixel is fill)."""
    canvas = np.full((S, S, 3), np.float32(fill), np.float32)
    is_fill = np.ones((S, S), bool)
    cx, cy = record["cx"], record["cy"]
    for k, t in enumerate(record["tiles"]):
        if t is None:
            continue
        src, flip, tw, th, x0, y0 = t
        qx = (cx, S) if k & 1 else (0, cx)
        qy = (cy, S) if k & 2 else (0, cy)
        ax, bx = max(x0, qx[0], 0), min(x0 + tw, qx[1], S)
        ay, by = max(y0, qy[0], 0), min(y0 + th, qy[1], S)
        if bx <= ax or by <= ay:
            continue
        tile = resize_tile(np.asarray(images[src]), flip, th, tw)
        canvas[ay:by, ax:bx] = tile[ay - y0:by - y0, ax - x0:bx - x0]
        is_fill[ay:by, ax:bx] = False
    return canvas, is_fill


def finish(canvas, order=(), factors=(1.0, 1.0, 1.0, 0.0), mean=oip.MEAN, std=oip.STD):
    """oracle.image_prep.transform_image from the resized uint8 levels on: colour ops in `order`, /255, normalise."""
    x = canvas
    for op in order:
        f = factors[op]
        if op == 0:
            x = oip._blend(x, np.float32(0), f)
        elif op == 1:
            x = oip._blend(x, np.float32(oip._gray(x).mean(dtype=np.float64)), f)
        elif op == 2:
            x = oip._blend(x, oip._gray(x)[..., None], f)
        elif op == 3:
            x = oip._hue(x, f)
    x = x * np.float32(1 / 255)
    x = (x - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    return torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))


def mosaic_image(images, record, S, fill=114, order=(), factors=(1.0, 1.0, 1.0, 0.0), mean=oip.MEAN, std=oip.STD):
    """One output image: float32 (3, S, S), normalised."""
    return finish(mosaic_canvas(images, record, S, fill)[0], order, factors, mean, std)


def fill_value(fill=114, mean=oip.MEAN, std=oip.STD):
    """The normalised value of an untouched fill pixel, per channel (float32, as `finish` computes it)."""
    return finish(np.full((1, 1, 3), np.float32(fill), np.float32), mean=mean, std=std).reshape(3)


def mosaic_boxes(record, targets, sizes, S, min_box=2.0, min_visible=0.1, max_boxes=128):
    """The box rule, float32: per tile flip, scale by (tw / W, th / H), translate by (x0, y0), clip the corners to the tile's
    visible rectangle (tile & quadrant & canvas); keep on clipped w, h >= min_box and clipped / scaled area >= min_visible;
    tile order, source order; over max_boxes the largest clipped areas stay (ties: the earlier box), order kept.
    -> float32 (M, 5): x, y, w, h, label."""
    f = np.float32
    cx, cy = record["cx"], record["cy"]
    rows, areas = [], []
    for k, (src, flip, tw, th, x0, y0) in enumerate(record["tiles"]):
        H, W = sizes[src]
        qx = (cx, S) if k & 1 else (0, cx)
        qy = (cy, S) if k & 2 else (0, cy)
        ax, bx = max(x0, qx[0], 0), min(x0 + tw, qx[1], S)
        ay, by = max(y0, qy[0], 0), min(y0 + th, qy[1], S)
        boxes = np.asarray(targets[src]["boxes"], f).reshape(-1, 4)
        labels = np.asarray(targets[src]["labels"], f).reshape(-1)
        if bx <= ax or by <= ay:
            continue
        sx, sy = f(tw / W), f(th / H)
        for (x, y, w, h), lab in zip(boxes, labels):
            if flip:
                x = f(W) - (x + w)
            x, w, y, h = x * sx, w * sx, y * sy, h * sy
            x1, y1 = x + f(x0), y + f(y0)
            x2, y2 = x1 + w, y1 + h
            x1, x2 = min(max(x1, f(ax)), f(bx)), min(max(x2, f(ax)), f(bx))
            y1, y2 = min(max(y1, f(ay)), f(by)), min(max(y2, f(ay)), f(by))
            cw, ch = f(x2 - x1), f(y2 - y1)
            if cw >= min_box and ch >= min_box and f(cw * ch) / f(f(w * h) + f(1e-9)) >= min_visible:
                rows.append([x1, y1, cw, ch, lab])
                areas.append(f(cw * ch))
    if len(rows) > max_boxes:
        order = sorted(range(len(rows)), key=lambda j: -float(areas[j]))[:max_boxes]       # sorted() is stable
        rows = [rows[j] for j in sorted(order)]
    return torch.from_numpy(np.asarray(rows, f).reshape(-1, 5))


def image_prep_mosaic(src_u8, recs, tiles, size, fill, jitter, dtype, mean, std):
    """CPU stand-in of ops.image_prep_mosaic (same arguments), built on the functions above."""
    by_off = {int(r[0]): j for j, r in enumerate(recs)}
    images = [src_u8[off:off + h * w * 3].reshape(h, w, 3).numpy() for off, h, w, _, _, _ in recs]
    outs = []
    for (off, h, w, flip, order, fac), (cx, cy, quad) in zip(recs, tiles):
        rec = {"cx": cx, "cy": cy, "tiles": [(by_off[int(t[0])], t[3], t[4], t[5], t[6], t[7]) if t is not None
                                             else None for t in quad]}
        outs.append(mosaic_image(images, rec, size, fill, tuple(order) if jitter else (), fac, mean, std))
    return torch.stack(outs).to(dtype)
