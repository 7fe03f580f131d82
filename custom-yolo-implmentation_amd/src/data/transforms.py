"""The reference's image transforms (src/data/transforms.py:4-24) on the DEVICE, for a whole batch at once.

    get_train_transforms()  ToImage -> RandomHorizontalFlip(0.5) -> Resize((640, 640)) -> ColorJitter(0.2, 0.2, 0.2, 0.1)
                            -> ToDtype(float32, scale=True) -> Normalize(ImageNet)
    get_val_transforms()    ToImage -> Resize -> ToDtype -> Normalize

The reference runs them per image with torchvision on DataLoader workers (PIL decode + ~40 ms of CPU per image); here
the workers only decode, and `BatchTransform` uploads the decoded uint8 images of a batch (any sizes) and runs flip +
antialiased bilinear resize + colour jitter + normalisation as a handful of launches (csrc/image_prep.hip).  The random
decisions are drawn on the host in torchvision's order (flip: one `torch.rand(1)`; jitter: `torch.randperm(4)` then one
uniform per factor), boxes follow the geometry (XYWH: x' = W - x - w for a flip, then scaling by 640/W, 640/H) and the
batch leaves in the format of src/data/collate.py: (images[N,3,S,S], [target dicts with "boxes" (Mi, 5)]).
With `mosaic=` set (opt-in, no reference counterpart), an output is composed of four resized images of its own batch around
a random centre, in the same launch sequence (`k_mosaic` in the resize launch's place), with its boxes clipped on the host.
With `affine=` set (opt-in, no reference counterpart), the finished canvas -- plain resize or mosaic -- is warped by a random
rotation, scale, shear and translation in one more launch (`k_affine`) before the colour chain, and the boxes follow.
With `mixup=` set (opt-in, no reference counterpart), the finished canvas of an output is blended with the finished, unmixed
canvas of another output of its batch in one more launch (`k_mixup`) before the colour chain, and takes that output's boxes too."""
import math

import numpy as np
import torch

from src.hipops import ops

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
MOSAIC_DEFAULTS = dict(p=1.0, gain=(0.4, 1.0), fill=114, min_box=2.0, min_visible=0.1, max_boxes=128, close_epochs=0)
AFFINE_DEFAULTS = dict(degrees=0.0, translate=0.1, scale=0.5, shear=0.0, fill=114, min_box=2.0, min_visible=0.1, max_aspect=100.0,
                       max_boxes=128, close_epochs=0)
MIXUP_DEFAULTS = dict(p=0.1, alpha=32.0, max_boxes=128, close_epochs=0)


def _uniform(lo, hi):
    return float(torch.empty(1).uniform_(lo, hi))


def keep_largest(boxes, area, max_boxes):
    """The cap of mosaic_boxes, affine_boxes and mixup_boxes: beyond `max_boxes` the rows with the largest `area` stay (ties: the
    earlier row), in their order."""
    if boxes.shape[0] > max_boxes:
        top = torch.sort(area, descending=True, stable=True).indices[:max_boxes]
        boxes = boxes[torch.sort(top).values]
    return boxes


def mosaic_geometry(draw, i, sizes, flip0, size):
    """A `sample_mosaic` draw (cx, cy, partners[3], gains[4], flips[3]) for output `i` of a batch whose images have `sizes`
    [(H, W)] -> the geometry record {"cx", "cy", "tiles": four (source index, flip, tw, th, x0, y0)}.  Tile 0 is image `i`
    with the flip `sample()` drew for it; tile k is its source resized to (th, tw) = round(gain * size / max(H, W) * (H, W)),
    at least one pixel, touching the centre with one corner."""
    cx, cy, partners, gains, flips = draw
    tiles = []
    for k, (src, flip) in enumerate(zip((i,) + tuple(partners), (flip0,) + tuple(flips))):
        h, w = sizes[src]
        b = size / max(h, w)
        tw, th = max(1, round(gains[k] * b * w)), max(1, round(gains[k] * b * h))
        tiles.append((int(src), bool(flip), tw, th, cx if k & 1 else cx - tw, cy if k & 2 else cy - th))
    return {"cx": int(cx), "cy": int(cy), "tiles": tiles}


def mosaic_boxes(record, targets, sizes, size, min_box, min_visible, max_boxes):
    """Boxes of a mosaic output, (M, 5) float32 (x, y, w, h, label): per tile the source's XYWH boxes flipped, scaled by
    (tw / W, th / H), moved by (x0, y0) and clipped to what the tile shows (its rectangle within its quadrant and the
    canvas); a box stays when its clipped sides are >= min_box and >= min_visible of its area is left.  Tile order, source
    order inside a tile; beyond max_boxes the largest clipped areas stay, in that order."""
    cx, cy = record["cx"], record["cy"]
    kept, areas = [], []
    for k, (src, flip, tw, th, x0, y0) in enumerate(record["tiles"]):
        h, w = sizes[src]
        b = targets[src]["boxes"].clone().float().reshape(-1, 4)
        lo_x, hi_x = max(x0, cx if k & 1 else 0, 0), min(x0 + tw, size if k & 1 else cx, size)
        lo_y, hi_y = max(y0, cy if k & 2 else 0, 0), min(y0 + th, size if k & 2 else cy, size)
        if b.shape[0] == 0 or hi_x <= lo_x or hi_y <= lo_y:
            continue
        if flip:
            b[:, 0] = w - (b[:, 0] + b[:, 2])
        sx, sy = tw / w, th / h
        b[:, [0, 2]] *= sx
        b[:, [1, 3]] *= sy
        full = b[:, 2] * b[:, 3]                            # w * sx * h * sy
        x1, y1 = b[:, 0] + x0, b[:, 1] + y0
        x2, y2 = x1 + b[:, 2], y1 + b[:, 3]
        x1, x2 = x1.clamp(lo_x, hi_x), x2.clamp(lo_x, hi_x)
        y1, y2 = y1.clamp(lo_y, hi_y), y2.clamp(lo_y, hi_y)
        cw, ch = x2 - x1, y2 - y1
        keep = (cw >= min_box) & (ch >= min_box) & (cw * ch / (full + 1e-9) >= min_visible)
        kept.append(torch.stack([x1, y1, cw, ch, targets[src]["labels"].float().reshape(-1)], 1)[keep])
        areas.append((cw * ch)[keep])
    if not kept:
        return torch.zeros(0, 5)
    return keep_largest(torch.cat(kept), torch.cat(areas), max_boxes)


def affine_matrix(draw, size):
    """A `sample_affine` draw (angle, gain, shear x, shear y, tx, ty; degrees) -> the forward 2 x 3 matrix canvas -> output,
    float64, M = T Sh R C in continuous pixel coordinates (pixel i covers [i, i + 1), its centre is i + 0.5): C moves the
    canvas centre (size / 2, size / 2) to the origin, R rotates by the angle and scales by the gain, Sh has tan(shear x) at
    [0, 1] and tan(shear y) at [1, 0], T translates by (tx size, ty size)."""
    angle, gain, shx, shy, tx, ty = (float(v) for v in draw)
    c = np.array([[1.0, 0.0, -size / 2], [0.0, 1.0, -size / 2], [0.0, 0.0, 1.0]])
    a = math.radians(angle)
    r = np.array([[gain * math.cos(a), -gain * math.sin(a), 0.0], [gain * math.sin(a), gain * math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    sh = np.array([[1.0, math.tan(math.radians(shx)), 0.0], [math.tan(math.radians(shy)), 1.0, 0.0], [0.0, 0.0, 1.0]])
    t = np.array([[1.0, 0.0, tx * size], [0.0, 1.0, ty * size], [0.0, 0.0, 1.0]])
    return (t @ sh @ r @ c)[:2]


def affine_record(m):
    """Forward 2 x 3 matrix -> the record k_affine takes: the six values (a00, a01, b0, a10, a11, b1) of the INVERSE map,
    formed in float64 and rounded once to fp32.  A non-finite or singular matrix is refused."""
    m = np.asarray(m, np.float64)
    if m.shape != (2, 3) or not np.isfinite(m).all():
        raise ValueError(f"affine: a forward matrix is 2 x 3 and finite, got {m.tolist()}")
    det = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    if not abs(det) > 1e-12 * max(1.0, float(np.abs(m[:, :2]).max()) ** 2):
        raise ValueError(f"affine: singular matrix (determinant {det})")
    a = np.array([[m[1, 1], -m[0, 1]], [-m[1, 0], m[0, 0]]]) / det
    b = -a @ m[:, 2]
    rec = np.array([a[0, 0], a[0, 1], b[0], a[1, 0], a[1, 1], b[1]]).astype(np.float32)
    if not np.isfinite(rec).all():
        raise ValueError(f"affine: the inverse of {m.tolist()} is not finite in fp32")
    return tuple(float(v) for v in rec)


def affine_boxes(m, boxes5, size, min_box, min_visible, max_aspect, max_boxes):
    """Boxes (M, 5) float32 (x, y, w, h, label) on the canvas -> on the warped output: the four corners through the forward
    matrix `m`, their axis-aligned hull clipped to [0, size]; a box stays when both clipped sides are >= min_box, when
    w'h' / (w h gain^2 + 1e-9) >= min_visible (gain^2 = |det| of the matrix: the area scale) and when its aspect ratio
    max(w'/h', h'/w') < max_aspect.  Order kept; beyond max_boxes the largest clipped areas stay, in that order."""
    b = boxes5.float().reshape(-1, 5)
    mt = torch.as_tensor(np.asarray(m, np.float64), dtype=torch.float32)
    if b.shape[0] == 0:
        return torch.zeros(0, 5)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]
    cx = torch.stack([x1, x2, x1, x2], 1)
    cy = torch.stack([y1, y1, y2, y2], 1)
    wx = mt[0, 0] * cx + mt[0, 1] * cy + mt[0, 2]
    wy = mt[1, 0] * cx + mt[1, 1] * cy + mt[1, 2]
    nx1, nx2 = wx.min(1).values.clamp(0, size), wx.max(1).values.clamp(0, size)
    ny1, ny2 = wy.min(1).values.clamp(0, size), wy.max(1).values.clamp(0, size)
    cw, ch = nx2 - nx1, ny2 - ny1
    gain2 = (mt[0, 0] * mt[1, 1] - mt[0, 1] * mt[1, 0]).abs()
    aspect = torch.maximum(cw / ch, ch / cw)
    keep = (cw >= min_box) & (ch >= min_box) & (cw * ch / (b[:, 2] * b[:, 3] * gain2 + 1e-9) >= min_visible) & (aspect < max_aspect)
    return keep_largest(torch.stack([nx1, ny1, cw, ch, b[:, 4]], 1)[keep], (cw * ch)[keep], max_boxes)


def mixup_boxes(own, partner, max_boxes):
    """Boxes of a mixed output, (M, 5) float32 (x, y, w, h, label): the output's own final boxes followed by the final boxes its
    partner's unmixed output carries, every one a full target; beyond max_boxes the largest areas w h stay, in that order."""
    out = torch.cat([own.float().reshape(-1, 5), partner.float().reshape(-1, 5)])
    return keep_largest(out, out[:, 2] * out[:, 3], max_boxes)


def _options(name, given, defaults, train):
    """What the mosaic, affine and mixup options share: training only, known keys, merged with their defaults."""
    if not train:
        raise ValueError(f"{name} is a training augmentation: the validation transform takes none")
    unknown = set(given) - set(defaults)
    if unknown:
        raise ValueError(f"{name}: unknown keys {sorted(unknown)}; expected {sorted(defaults)}")
    return {**defaults, **given}


def _mosaic_options(m):
    gain = tuple(float(g) for g in m["gain"])
    if not 0.0 <= m["p"] <= 1.0:
        raise ValueError(f"mosaic.p must lie in [0, 1], got {m['p']}")
    if len(gain) != 2 or not 0.0 < gain[0] <= gain[1] <= 2.0:
        raise ValueError(f"mosaic.gain must be [lo, hi] with 0 < lo <= hi <= 2, got {m['gain']}")
    if not 0 <= int(m["fill"]) <= 255 or int(m["max_boxes"]) < 1 or int(m["close_epochs"]) < 0:
        raise ValueError("mosaic: fill is a uint8 level, max_boxes >= 1 and close_epochs >= 0")
    return dict(p=float(m["p"]), gain=gain, fill=int(m["fill"]), min_box=float(m["min_box"]), min_visible=float(m["min_visible"]),
                max_boxes=int(m["max_boxes"]), close_epochs=int(m["close_epochs"]))


def _affine_options(a, mosaic):
    if not 0.0 <= a["degrees"] <= 180.0 or not 0.0 <= a["shear"] <= 89.0:
        raise ValueError(f"affine.degrees must lie in [0, 180] and affine.shear in [0, 89], got {a['degrees']}, {a['shear']}")
    if not 0.0 <= a["translate"] < 1.0 or not 0.0 <= a["scale"] < 1.0:
        raise ValueError(f"affine.translate and affine.scale must lie in [0, 1), got {a['translate']}, {a['scale']}")
    if int(a["fill"]) != a["fill"] or not 0 <= int(a["fill"]) <= 255 or int(a["max_boxes"]) < 1 or int(a["close_epochs"]) < 0:
        raise ValueError("affine: fill is a uint8 level, max_boxes >= 1 and close_epochs >= 0")
    if a["min_box"] < 0 or a["min_visible"] < 0 or not a["max_aspect"] > 1:
        raise ValueError("affine: min_box >= 0, min_visible >= 0 and max_aspect > 1")
    if mosaic is not None and mosaic["fill"] != int(a["fill"]):
        raise ValueError(f"affine.fill ({a['fill']}) and mosaic.fill ({mosaic['fill']}) are one level: the launch takes one")
    return dict(degrees=float(a["degrees"]), translate=float(a["translate"]), scale=float(a["scale"]), shear=float(a["shear"]),
                fill=int(a["fill"]), min_box=float(a["min_box"]), min_visible=float(a["min_visible"]), max_aspect=float(a["max_aspect"]),
                max_boxes=int(a["max_boxes"]), close_epochs=int(a["close_epochs"]))


def _mixup_options(x):
    if not 0.0 <= x["p"] <= 1.0:
        raise ValueError(f"mixup.p must lie in [0, 1], got {x['p']}")
    if not (x["alpha"] > 0 and math.isfinite(x["alpha"])):
        raise ValueError(f"mixup.alpha must be positive and finite, got {x['alpha']}")
    if int(x["max_boxes"]) < 1 or int(x["close_epochs"]) < 0:
        raise ValueError("mixup: max_boxes >= 1 and close_epochs >= 0")
    return dict(p=float(x["p"]), alpha=float(x["alpha"]), max_boxes=int(x["max_boxes"]), close_epochs=int(x["close_epochs"]))


class BatchTransform:
    """Callable(images, targets) -> (batch on `device`, targets).  images: decoded RGB images as uint8 (H, W, 3) arrays /
    tensors or PIL images; targets: dicts with "boxes" (M, 4) XYWH pixels and "labels" (M, 1) (the reference dataset's
    items before its transform) or None."""

    def __init__(self, train, size=640, device="cuda", dtype=torch.float32, flip_p=0.5, brightness=0.2, contrast=0.2,
                 saturation=0.2, hue=0.1, mean=MEAN, std=STD, mosaic=None, affine=None, mixup=None):
        self.train, self.size, self.device, self.dtype = train, size, torch.device(device), dtype
        self.flip_p, self.jit = flip_p, (brightness, contrast, saturation, hue)
        self.mean, self.std = mean, std
        # mosaic, affine, mixup: each None (off: the path without the key, call for call) or a dict of its *_DEFAULTS' keys; `*_on`
        # switches it per epoch (DevicePreppedLoader.set_epoch turns it off for the last `close_epochs` epochs)
        self.mosaic = None if mosaic is None else _mosaic_options(_options("mosaic", mosaic, MOSAIC_DEFAULTS, train))
        self.affine = None if affine is None else _affine_options(_options("affine", affine, AFFINE_DEFAULTS, train), self.mosaic)
        self.mixup = None if mixup is None else _mixup_options(_options("mixup", mixup, MIXUP_DEFAULTS, train))
        self.mosaic_on, self.affine_on, self.mixup_on = self.mosaic is not None, self.affine is not None, self.mixup is not None
        self._pinned = None                 # reused pinned upload buffer (one memcpy per image into it, one async H2D per batch)
        self._uploaded = None

    def sample(self):
        """One image's random decisions, drawn like torchvision draws them: (flip, order, factors)."""
        if not self.train:
            return False, (), (1.0, 1.0, 1.0, 0.0)
        flip = bool(torch.rand(1) < self.flip_p)
        order = tuple(int(i) for i in torch.randperm(4))
        b, c, s, h = self.jit
        fac = (_uniform(max(0.0, 1 - b), 1 + b), _uniform(max(0.0, 1 - c), 1 + c), _uniform(max(0.0, 1 - s), 1 + s), _uniform(-h, h))
        return flip, order, fac

    def sample_mosaic(self, n):
        """The mosaic decisions of a batch of `n` images, drawn after its `n` sample() calls (whose sequence is unchanged):
        per output None (plain) or (cx, cy, partners[3], gains[4], flips[3]) -- one `torch.rand(1) < p`, then three partner
        indices with replacement, the centre in [S//4, S - S//4], four gains in tile order, the flips of tiles 1-3."""
        if self.mosaic is None:
            raise ValueError("sample_mosaic: this transform was built without mosaic=")
        m, s = self.mosaic, self.size
        out = []
        for _ in range(n):
            if not bool(torch.rand(1) < m["p"]):
                out.append(None)
                continue
            partners = tuple(int(v) for v in torch.randint(0, n, (3,)))
            cx = int(torch.randint(s // 4, s - s // 4 + 1, (1,)))
            cy = int(torch.randint(s // 4, s - s // 4 + 1, (1,)))
            gains = tuple(_uniform(*m["gain"]) for _ in range(4))
            flips = tuple(bool(torch.rand(1) < self.flip_p) for _ in range(3))
            out.append((cx, cy, partners, gains, flips))
        return out

    def sample_affine(self, n):
        """The warp decisions of a batch of `n` images, drawn after its `n` sample() calls and after sample_mosaic(n) when the
        mosaic is on (both sequences unchanged): per output six uniform draws, also when a range is 0 -- angle, gain, shear x,
        shear y (degrees), tx, ty (fractions of the size; 0.5 keeps the centre)."""
        if self.affine is None:
            raise ValueError("sample_affine: this transform was built without affine=")
        a = self.affine
        return [(_uniform(-a["degrees"], a["degrees"]), _uniform(1 - a["scale"], 1 + a["scale"]), _uniform(-a["shear"], a["shear"]),
                 _uniform(-a["shear"], a["shear"]), _uniform(0.5 - a["translate"], 0.5 + a["translate"]),
                 _uniform(0.5 - a["translate"], 0.5 + a["translate"])) for _ in range(n)]

    def sample_mixup(self, n):
        """The mixup decisions of a batch of `n` images, drawn after its `n` sample() calls, after sample_mosaic(n) and after
        sample_affine(n) where those are on (all three sequences unchanged): nothing for n < 2 (no partner exists); else per
        output None (not mixed) or (partner, r) -- one `torch.rand(1) < p`, then d = `torch.randint(1, n, (1,))` for the partner
        (i + d) % n, another output, then r from Beta(alpha, alpha), an fp32 value in [0, 1]."""
        if self.mixup is None:
            raise ValueError("sample_mixup: this transform was built without mixup=")
        x = self.mixup
        if n < 2:
            return [None] * n
        out = []
        for i in range(n):
            if not bool(torch.rand(1) < x["p"]):
                out.append(None)
                continue
            d = int(torch.randint(1, n, (1,)))
            out.append(((i + d) % n, float(torch.distributions.Beta(x["alpha"], x["alpha"]).sample())))
        return out

    @staticmethod
    def _mix_records(mixup, n):
        """Per output None (not mixed) or (partner, r) checked: another output of the batch and an fp32 ratio in [0, 1]."""
        if len(mixup) != n:
            raise ValueError(f"mixup: {len(mixup)} records for {n} images")
        out = []
        for i, m in enumerate(mixup):
            if m is not None:
                if len(m) != 2 or int(m[0]) != m[0] or not 0 <= int(m[0]) < n or int(m[0]) == i or not 0.0 <= float(m[1]) <= 1.0:
                    raise ValueError(f"mixup record {i}: (partner, r) with another output of the batch and r in [0, 1], got {m!r}")
                m = (int(m[0]), float(np.float32(m[1])))
            out.append(m)
        return out

    def _affine_matrices(self, affine, n):
        """Per output the forward 2 x 3 matrix (float64), from draws (six values), ready matrices or None (identity)."""
        if len(affine) != n:
            raise ValueError(f"affine: {len(affine)} records for {n} images")
        out = []
        for a in affine:
            if a is None:
                out.append(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))
                continue
            a = np.asarray(a, np.float64)
            if a.shape not in ((6,), (2, 3)):
                raise ValueError(f"affine: a record is a draw of six values or a 2 x 3 forward matrix, got shape {a.shape}")
            out.append(affine_matrix(a, self.size) if a.shape == (6,) else a)
        return out

    @staticmethod
    def _as_u8(img):
        if isinstance(img, torch.Tensor):
            t = img
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(img.convert("RGB") if hasattr(img, "convert") else img)))
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("BatchTransform takes decoded RGB images as uint8 (H, W, 3)")
        return t.contiguous()

    def __call__(self, images, targets=None, params=None, mosaic=None, affine=None, mixup=None):
        """`params`: the per-image sample() decisions; `mosaic`: per output None (plain), a sample_mosaic() draw or a
        geometry record (`mosaic_geometry`'s format); `affine`: per output None (identity), a sample_affine() draw or a
        forward 2 x 3 matrix; `mixup`: per output None (not mixed) or (partner, r) -- all are drawn here when not given."""
        imgs = [self._as_u8(i) for i in images]
        recs, records, mats, inverse, mix = self._resolve(imgs, params, mosaic, affine, mixup)
        flat = self._upload(imgs, recs)
        jitter = self.train and any(len(r[4]) for r in recs)
        tiles = self._mosaic_tiles(records, recs) if records is not None else None
        fill = self.affine["fill"] if inverse is not None else self.mosaic["fill"] if tiles is not None else 0
        tail = (self.size, fill, jitter, self.dtype, self.mean, self.std)
        if mix is not None:
            batch = ops.image_prep_mixup(flat, recs, tiles, inverse, [(i, 1.0) if m is None else m for i, m in enumerate(mix)], *tail)
        elif inverse is not None:
            batch = ops.image_prep_affine(flat, recs, tiles, inverse, *tail)
        elif tiles is not None:
            batch = ops.image_prep_mosaic(flat, recs, tiles, *tail)
        else:
            batch = ops.image_prep(flat, recs, self.size, jitter, self.dtype, self.mean, self.std)
        return batch, None if targets is None else self._boxes(targets, recs, records, mats, mix)

    def _resolve(self, imgs, params, mosaic, affine, mixup):
        """The decisions of a batch, drawn where not given, in the order sample(), sample_mosaic(), sample_affine(), sample_mixup() ->
        (PrepImage records, per output None or a mosaic geometry record, forward matrices, their inverse records, mix records); each
        of the last four is None when that stage does not run (the mix also when nobody mixes: the leaf is then the one a transform
        without the key takes)."""
        n = len(imgs)
        params = params if params is not None else [self.sample() for _ in imgs]
        for name, given in (("mosaic", mosaic), ("affine", affine), ("mixup", mixup)):
            if given is not None and getattr(self, name) is None:
                raise ValueError(f"{name} records were passed to a BatchTransform built without {name}=")
        use_mosaic = self.mosaic is not None and (self.mosaic_on or mosaic is not None)
        if use_mosaic and mosaic is None:
            mosaic = self.sample_mosaic(n)
        mats = inverse = mix = None
        if self.affine is not None and (self.affine_on or affine is not None):
            mats = self._affine_matrices(affine if affine is not None else self.sample_affine(n), n)
            inverse = [affine_record(m) for m in mats]
        if self.mixup is not None and (self.mixup_on or mixup is not None):
            mix = self._mix_records(mixup if mixup is not None else self.sample_mixup(n), n)
            if all(m is None for m in mix):
                mix = None
        recs, off = [], 0
        for t, (flip, order, fac) in zip(imgs, params):
            h, w = int(t.shape[0]), int(t.shape[1])
            recs.append((off, h, w, flip, order, fac))
            off += h * w * 3
        return recs, self._mosaic_records(mosaic, recs) if use_mosaic else None, mats, inverse, mix

    def _upload(self, imgs, recs):
        """The batch's images back to back on the device: one memcpy per image into the pinned buffer, one async copy per batch."""
        if self.device.type != "cuda":
            return torch.cat([t.reshape(-1) for t in imgs])
        total = sum(t.numel() for t in imgs)
        if self._pinned is None or self._pinned.numel() < total:
            self._pinned = torch.empty(int(total * 1.25), dtype=torch.uint8).pin_memory()
        elif self._uploaded is not None:
            self._uploaded.synchronize()        # the previous batch's upload has left the buffer
        for t, r in zip(imgs, recs):
            self._pinned[r[0]:r[0] + t.numel()].copy_(t.reshape(-1))
        flat = self._pinned[:total].to(self.device, non_blocking=True)
        self._uploaded = torch.cuda.Event()
        self._uploaded.record(torch.cuda.current_stream(self.device))
        return flat

    def _boxes(self, targets, recs, records, mats, mix):
        """The targets of the outputs: the boxes follow the flip and resize or the mosaic, then the warp, then take the partner's."""
        out_t = []
        sizes = [(r[1], r[2]) for r in recs]
        for i, (tg, (_, h, w, flip, _, _)) in enumerate(zip(targets, recs)):
            new = {k: v for k, v in tg.items() if k not in ("boxes", "labels")}
            if records is not None and records[i] is not None:
                m = self.mosaic
                new["boxes"] = mosaic_boxes(records[i], targets, sizes, self.size, m["min_box"], m["min_visible"], m["max_boxes"])
            else:
                b = tg["boxes"].clone().float().reshape(-1, 4)
                if flip:
                    b[:, 0] = w - (b[:, 0] + b[:, 2])
                b[:, [0, 2]] *= self.size / w
                b[:, [1, 3]] *= self.size / h
                new["boxes"] = torch.cat([b, tg["labels"].float().reshape(-1, 1)], 1)      # dataset_loader.py:76
            if mats is not None:
                a = self.affine
                new["boxes"] = affine_boxes(mats[i], new["boxes"], self.size, a["min_box"], a["min_visible"], a["max_aspect"], a["max_boxes"])
            out_t.append(new)
        if mix is not None:                 # the partner's boxes are those of its own unmixed output: read before any is replaced
            unmixed = [t["boxes"] for t in out_t]
            for i, m in enumerate(mix):
                if m is not None:
                    out_t[i]["boxes"] = mixup_boxes(unmixed[i], unmixed[m[0]], self.mixup["max_boxes"])
        return out_t

    def _mosaic_records(self, mosaic, recs):
        """Per output None (plain) or its geometry record, from draws or ready records."""
        if len(mosaic) != len(recs):
            raise ValueError(f"mosaic: {len(mosaic)} records for {len(recs)} images")
        sizes = [(r[1], r[2]) for r in recs]
        out = []
        for i, m in enumerate(mosaic):
            if m is not None and not isinstance(m, dict):
                m = mosaic_geometry(m, i, sizes, recs[i][3], self.size)
            if m is not None:
                if len(m["tiles"]) != 4 or any(not 0 <= t[0] < len(recs) or t[2] < 1 or t[3] < 1 for t in m["tiles"]):
                    raise ValueError(f"mosaic record {i}: four tiles with a source inside the batch and a size of at least 1 x 1")
            out.append(m)
        return out

    def _mosaic_tiles(self, records, recs):
        """The tile table of ops.image_prep_mosaic; a plain output is the record that reproduces the plain resize: the centre
        in the bottom-right corner and tile 0 covering the canvas."""
        s, out = self.size, []
        for i, m in enumerate(records):
            if m is None:
                off, h, w, flip = recs[i][:4]
                out.append((s, s, [(off, h, w, flip, s, s, 0, 0), None, None, None]))
            else:
                out.append((m["cx"], m["cy"], [(recs[src][0], recs[src][1], recs[src][2], flip, tw, th, x0, y0)
                                               for src, flip, tw, th, x0, y0 in m["tiles"]]))
        return out


def get_train_transforms(size=640, device="cuda", dtype=torch.float32, mosaic=None, affine=None, mixup=None):
    return BatchTransform(True, size, device, dtype, mosaic=mosaic, affine=affine, mixup=mixup)


def get_val_transforms(size=640, device="cuda", dtype=torch.float32):
    """Batch form; `Model.inference` applies it to a single PIL image (reference :16-24)."""
    return BatchTransform(False, size, device, dtype)
