"""Reference of `Model.predict`'s inverse map (csrc/decode_nms.hip::k_rows_to_source), shared by tests/test_predict_cpu.py (the
proof that the comparison is sharp, no GPU) and tests/test_gpu_predict.py (the kernel).

rows_to_source_ref restates the kernel in numpy float32, operation for operation -- numpy performs the same IEEE operations in
the same order, each rounding once:
    x' = min(max((x - (float)left) * sx, 0.f), (float)W)      for x1 and x2
    y' = min(max((y - (float)top)  * sy, 0.f), (float)H)      for y1 and y2
    conf' = prob ? 1.f / (1.f + expf(-conf)) : conf;  cls unchanged;  rows at or past counts[n] untouched
so the box columns are compared bit for bit.  The score is the one column that is not: numpy's expf and the device's are two
libraries.  The GPU test holds it to SIGMOID_BOUND against the float64 sigmoid instead.

SIGMOID_BOUND.  c = fl(1 / fl(1 + e~)), e~ = expf(-x) (the negation is exact).  With u = 2^-24 (half an ulp, relative):
  * e~ = e (1 + d1), |d1| <= 2^-23: the HIP programming guide's table of single-precision device functions gives expf a
    maximum error of 1 ulp, and an ulp is at most 2^-23 of the value.  dc/de = -1 / (1 + e)^2, so this moves c by at most
    e / (1 + e)^2 * 2^-23 <= 2^-25 (e / (1 + e)^2 <= 1/4, at e = 1);
  * the add rounds once: 1 + e~ changes by a relative u, and so does c <= 1: at most 2^-24;
  * the divide rounds once: at most c u <= 2^-24.
Sum: 2^-25 + 2^-24 + 2^-24 = 1.25 * 2^-23 < 2^-22 = SIGMOID_BOUND (second-order terms are below 2^-45).  Where e~ overflows
(x < -88.7) c = 1 / inf = 0 against a sigmoid below 2^-127, and e~ = 0 gives 1 against 1 - 2^-128: both inside the bound.

Mutants (rows_to_source_ref(mut=...)): the defects a wrong inverse map would have.  Each changes at least one element of
CASES' rows -- tests/test_predict_cpu.py asserts it -- so a kernel with that defect cannot pass the bit comparison."""
import functools

import numpy as np

f32 = np.float32
SIGMOID_BOUND = 2.0 ** -22
MUTANTS = ["common_gain", "pad_kept", "pad_added", "scales_swapped", "divide", "no_clip", "clip_to_canvas", "past_count"]
S = 96
MAX_DET = 8
SOURCES = [(37, 41), (50, 200), (200, 50), (96, 96), (7, 10)]          # (H, W)
COUNTS = [8, 0, 5, 3, 8]                                              # count = 0 and count = max_det are both there
# yolo_letter_fill: a good record (the 50 x 200 picture on S = 96) and, one change each, what the record contract refuses
LETTER_OK = dict(off=0, H=50, W=200, nw=96, nh=24, left=0, top=36, sx=200 / 96, sy=50 / 24, S=96, src_bytes=3 * 50 * 200)
LETTER_BLANK = dict(H=0, W=0, nw=0, nh=0, left=0, top=0, sx=1.0, sy=1.0)
LETTER_REFUSED = [dict(off=-1), dict(off=1), dict(src_bytes=3 * 50 * 200 - 1), dict(H=1 << 30, W=1 << 30),   # outside the source buffer
                  dict(nw=97), dict(nw=-1), dict(nh=97), dict(nh=-1),                                        # outside [0, S]
                  dict(nw=0), dict(nh=0),                                                                    # exactly one of them 0
                  dict(left=1), dict(left=-1), dict(top=73), dict(top=-1),                                   # leaves the canvas
                  dict(sx=0.0), dict(sx=-1.0), dict(sx=float("inf")), dict(sx=float("nan")),                 # not finite and positive
                  dict(sy=0.0), dict(sy=-1.0), dict(sy=float("inf")), dict(sy=float("nan"))]
YOLO_ERR_ARG = 1001


def letter_fill(lib, ptr, index=0, **kw):
    """yolo_letter_fill of LETTER_OK with the changes `kw` into record `index` of the host table at `ptr` -> its status"""
    a = {**LETTER_OK, **kw}
    return lib.query("yolo_letter_fill", ptr, index, a["off"], a["H"], a["W"], a["nw"], a["nh"], a["left"], a["top"], a["sx"], a["sy"],
                     a["S"], a["src_bytes"])


def geometry(H, W, size, scaleup=True):
    """letterbox_geometry restated on its own (the CPU test holds the module's function to hand-worked cases and to this)."""
    r = min(size / H, size / W)
    if not scaleup:
        r = min(r, 1.0)
    nw, nh = min(size, max(1, int(np.floor(W * r + 0.5)))), min(size, max(1, int(np.floor(H * r + 0.5))))
    return nw, nh, (size - nw) // 2, (size - nh) // 2, float(f32(W / nw)), float(f32(H / nh))


@functools.lru_cache(maxsize=None)
def cases():
    """-> (recs [(off, H, W, nw, nh, left, top, sx, sy)], rows float32 [N][MAX_DET][6], counts int32 [N]): boxes on the canvas,
    reaching into the bars and beyond the canvas ([-12, S + 12]), logits in descending order per image, integer classes.
    Read-only: every user copies before it writes."""
    rng = np.random.default_rng(96)
    recs, off = [], 0
    for h, w in SOURCES:
        recs.append((off, h, w) + geometry(h, w, S))
        off += 3 * h * w
    n = len(SOURCES)
    rows = np.empty((n, MAX_DET, 6), np.float32)
    a = rng.uniform(-12.0, S + 12.0, (n, MAX_DET, 2, 2)).astype(np.float32)
    rows[..., 0], rows[..., 1] = a[..., 0, 0].copy(), a[..., 0, 1].copy()
    rows[..., 2], rows[..., 3] = a[..., 1, 0].copy(), a[..., 1, 1].copy()
    rows[..., :2], rows[..., 2:4] = np.minimum(rows[..., :2], rows[..., 2:4]), np.maximum(rows[..., :2], rows[..., 2:4])
    rows[..., 4] = -np.sort(-rng.uniform(-9.0, 9.0, (n, MAX_DET)).astype(np.float32), axis=1)
    rows[..., 5] = rng.integers(0, 80, (n, MAX_DET)).astype(np.float32)
    rows.setflags(write=False)
    counts = np.asarray(COUNTS, np.int32)
    counts.setflags(write=False)
    return recs, rows, counts


def rows_to_source_ref(rows, counts, recs, prob, size=S, mut=None):
    """-> float32 copy of `rows` [N][max_det][6] mapped back by `recs`, in k_rows_to_source's operations and order."""
    out = np.array(rows, np.float32)
    assert out.dtype == np.float32
    for n, (_, H, W, nw, nh, left, top, sx, sy) in enumerate(recs):
        c = int(counts[n])
        if mut == "past_count":
            c = out.shape[1]
        sx, sy = f32(sx), f32(sy)
        if mut == "common_gain":
            sx = sy = f32(max(H, W) / size)
        if mut == "scales_swapped":
            sx, sy = sy, sx
        for col, pad, s, hi, num, den in ((0, left, sx, W, nw, W), (1, top, sy, H, nh, H), (2, left, sx, W, nw, W), (3, top, sy, H, nh, H)):
            v = out[n, :c, col]
            p = f32(pad)
            v = v if mut == "pad_kept" else v + p if mut == "pad_added" else v - p
            v = v / f32(num / den) if mut == "divide" else v * s
            if mut != "no_clip":
                v = np.minimum(np.maximum(v, f32(0)), f32(size if mut == "clip_to_canvas" else hi))
            assert v.dtype == np.float32
            out[n, :c, col] = v
        if prob:
            with np.errstate(over="ignore"):
                out[n, :c, 4] = f32(1) / (f32(1) + np.exp(-out[n, :c, 4], dtype=np.float32))
    return out


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))
