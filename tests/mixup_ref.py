"""Numpy restatement of the mixup's contract (test infrastructure; src/data/transforms.py, csrc/image_prep.hip::k_mixup).

A record is None (the output is not mixed) or (partner, r): the output's finished canvas `a` and the finished, UNMIXED canvas `b`
of output `partner` of the same batch become, per uint8 element and in fp32 with one rounding per operation,

    level = clamp(floor((r * a + (1.0f - r) * b) + 0.5f), 0, 255)

`mix_f32` does exactly that, operation by operation; the device must equal it, element for element: every operation is one
correctly rounded fp32 operation and nothing is contracted.  `mut=` plants one defect.  The canvases in front of the mix are
tests/mosaic_ref.py's and tests/affine_ref.py's, the colour ops and the normalisation behind it oracle/image_prep.py's
(`mosaic_ref.finish`)."""
import numpy as np
import torch

import affine_ref
import mosaic_ref

f32 = np.float32
RATIOS = [0.0, 1.0, 0.5, 0.25, 0.3, 0.7, 0.4719, 2.0 ** -10]
ARITHMETIC_MUTANTS = ["swap", "rint", "trunc", "fma", "lerp", "f64"]
MUTANTS = ARITHMETIC_MUTANTS + ["inplace"]


def blend_f32(a, b, r, mut=None):
    """levels a, b (any shape) and one ratio -> float32 levels, k_mixup's operations in its order"""
    a, b = np.asarray(a).astype(np.float32), np.asarray(b).astype(np.float32)
    r = f32(r)
    q = f32(1.0) - r
    assert r.dtype == np.float32 and q.dtype == np.float32
    if mut == "swap":
        r, q = q, r
    if mut == "f64":
        acc = float(r) * a.astype(np.float64) + (1.0 - float(r)) * b.astype(np.float64)
        return np.clip(np.floor(acc + 0.5), 0, 255).astype(np.float32)
    if mut == "fma":
        # r * a is exact in float64 (24 x 8 bits) and so is its sum with the fp32 product q * b: one rounding to fp32, as a fused
        # multiply-add rounds
        acc = (float(r) * a.astype(np.float64) + (q * b).astype(np.float64)).astype(np.float32)
    elif mut == "lerp":
        acc = b + r * (a - b)
    else:
        acc = r * a + q * b
    assert acc.dtype == np.float32
    if mut == "rint":
        return np.clip(np.rint(acc), 0, 255)
    return np.clip(np.floor(acc if mut == "trunc" else acc + f32(0.5)), 0, 255)


def mix_f32(canvases, recs, mut=None):
    """canvases: levels (N, ...), the finished unmixed canvases of a batch; recs: per output None or (partner, r) -> float32
    levels of the same shape.  Every partner is read unmixed (`mut="inplace"`: the outputs are mixed one after the other in one
    buffer, so a partner with a smaller index is read after it was itself mixed)."""
    canvases = np.asarray(canvases).astype(np.float32)
    if len(recs) != canvases.shape[0]:
        raise ValueError(f"{len(recs)} records for {canvases.shape[0]} canvases")
    out = canvases.copy()
    read = out if mut == "inplace" else canvases
    for i, rec in enumerate(recs):
        if rec is None or rec[0] == i:
            continue
        out[i] = blend_f32(read[i], read[rec[0]], rec[1], None if mut == "inplace" else mut)
    return out


def lattice():
    """every pair of levels once: a = k % 256, b = k // 256, k < 65 536"""
    k = np.arange(65536)
    return (k % 256).astype(np.float32), (k // 256).astype(np.float32)


def mixup_boxes(own, partner, max_boxes=128):
    """The box rule, one row at a time: own boxes, then the partner's; over max_boxes the largest areas w h (float32) stay (ties:
    the earlier box), order kept.  -> float32 (M, 5)"""
    rows = [list(r) for r in np.asarray(own, np.float32).reshape(-1, 5)] + [list(r) for r in np.asarray(partner, np.float32).reshape(-1, 5)]
    if len(rows) > max_boxes:
        order = sorted(range(len(rows)), key=lambda j: -float(f32(rows[j][2]) * f32(rows[j][3])))[:max_boxes]       # sorted() is stable
        rows = [rows[j] for j in sorted(order)]
    return torch.from_numpy(np.asarray(rows, np.float32).reshape(-1, 5))


def canvases_of(src_u8, recs, tiles, affine, size, fill):
    """The finished unmixed canvases (N, S, S, 3) float32 levels of ops.image_prep_mixup's arguments: the plain resize (tiles None)
    or the mosaic, warped by affine_ref.warp_f32 unless affine is None."""
    by_off = {int(r[0]): j for j, r in enumerate(recs)}
    images = [src_u8[off:off + h * w * 3].reshape(h, w, 3).numpy() for off, h, w, _, _, _ in recs]
    out = []
    for i, (off, h, w, flip, order, fac) in enumerate(recs):
        if tiles is None:
            rec = mosaic_ref.plain_record(i, flip, size)
        else:
            cx, cy, quad = tiles[i]
            rec = {"cx": cx, "cy": cy, "tiles": [(by_off[int(t[0])], t[3], t[4], t[5], t[6], t[7]) if t is not None else None
                                                 for t in quad]}
        canvas = mosaic_ref.mosaic_canvas(images, rec, size, fill)[0]
        out.append(canvas if affine is None else affine_ref.warp_f32(canvas, affine[i], fill))
    return np.stack(out)


def image_prep_mixup(src_u8, recs, tiles, affine, mix, size, fill, jitter, dtype, mean, std):
    """CPU stand-in of ops.image_prep_mixup (same arguments): the canvases above, mixed by mix_f32, then the colour ops of each
    OUTPUT and the normalisation."""
    if len(mix) != len(recs):
        raise ValueError(f"image_prep_mixup: {len(recs)} records need {len(recs)} mix records")
    mixed = mix_f32(canvases_of(src_u8, recs, tiles, affine, size, fill), mix)
    return torch.stack([mosaic_ref.finish(mixed[i], tuple(order) if jitter else (), fac, mean, std)
                        for i, (_, _, _, _, order, fac) in enumerate(recs)]).to(dtype)
