"""COCO average precision restated in numpy float64, for the tests of the device kernels (yolo_ap_match, yolo_ap_curve).

The rules are COCOeval's published ones (pycocotools cocoeval.py: evaluateImg, accumulate, _summarize) for area "all", with
no crowd and no ignore regions:

  matching   per image, rows in the order given (descending score).  For IoU threshold t a row of class c takes the ground
             truth of class c not yet taken at t whose IoU is largest and >= min(thr_t, 1 - 1e-10); the scan replaces on `>=`,
             so among equal IoUs the HIGHEST index wins.  Every threshold keeps its own `taken` set.  Images without ground
             truth are not skipped: their rows are false positives.
  IoU        in double from the fp32 values: ground-truth corners cx -+ w / 2, cy -+ h / 2; iw = min(x2, X2) - max(x1, X1)
             clamped at 0, ih likewise; inter = iw * ih; a = (x2 - x1) * (y2 - y1) for either box;
             iou = inter / ((a1 + a2) - inter), no epsilon.  A NaN IoU never matches.
  records    key = (cls << 32) | (0xFFFFFFFF - ord(score)), ord = the order-preserving map of an fp32 bit pattern to uint32;
             ascending keys = class ascending, then score descending.  Rows at or past the image's count and rows whose class
             is outside [0, nc) get key = nc << 32 and tp = 0.  tp bit t = matched at threshold t.  An image with more than
             1024 ground truths sets status and contributes nothing.
  table      precision[c][t][k], 101 recall thresholds np.linspace(0, 1, 101): rows of class c in ascending key order with a
             STABLE sort (COCOeval's mergesort); tp_i, fp_i cumulative; rc_i = tp_i / npig; pr_i = tp_i / (fp_i + tp_i + eps),
             eps = np.spacing(1); envelope from the right; q_k = pr[first i with rc_i >= r_k], 0 when there is none; npig = 0
             gives -1 everywhere (class absent), a class with ground truth and no rows 101 zeros.
  means      over the entries > -1 (mAP50-95: the whole table, mAP50: the threshold equal to 0.5), 0 when there is none.

The keyword switches (`tie_highest`, `strict`, `shared_taken`, `skip_empty`, `stable`, `envelope`, `side`) exist for the
mutants of tests/test_ap_ref_cpu.py; their defaults are the rules above."""
import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
MAX_GT = 1024


def score_ord(score):
    u = np.ascontiguousarray(score, dtype=np.float32).view(np.uint32)
    return np.where((u & np.uint32(0x80000000)) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def iou_matrix(det, gt):
    """det [n][>=4] fp32 (x1, y1, x2, y2), gt [m][>=4] fp32 (cx, cy, w, h) -> float64 [n][m]"""
    d, g = np.asarray(det, dtype=np.float32).astype(np.float64), np.asarray(gt, dtype=np.float32).astype(np.float64)
    x1, y1, x2, y2 = (d[:, k][:, None] for k in range(4))
    hw, hh = g[:, 2] / 2.0, g[:, 3] / 2.0
    X1, Y1, X2, Y2 = (g[:, 0] - hw)[None], (g[:, 1] - hh)[None], (g[:, 0] + hw)[None], (g[:, 1] + hh)[None]
    a1, a2 = (x2 - x1) * (y2 - y1), (X2 - X1) * (Y2 - Y1)
    with np.errstate(invalid="ignore", divide="ignore"):
        iw = np.where(x2 < X2, x2, X2) - np.where(x1 > X1, x1, X1)
        ih = np.where(y2 < Y2, y2, Y2) - np.where(y1 > Y1, y1, Y1)
        iw, ih = np.where(iw > 0.0, iw, 0.0), np.where(ih > 0.0, ih, 0.0)
        inter = iw * ih
        return inter / ((a1 + a2) - inter)


def _classes(col):
    with np.errstate(invalid="ignore"):
        return np.asarray(col, dtype=np.float32).astype(np.int64)


def match_image(det, n, gt, thrs, nc, tie_highest=True, strict=False, shared_taken=False):
    """det fp32 [K][6] (x1, y1, x2, y2, score, cls), n valid rows, gt fp32 [m][5] -> (key int64 [K], tp uint32 [K])"""
    det = np.asarray(det, dtype=np.float32).reshape(-1, 6)
    gt = np.asarray(gt, dtype=np.float32).reshape(-1, 5)
    K, m = det.shape[0], gt.shape[0]
    n = min(max(int(n), 0), K)
    cls = _classes(det[:, 5])
    valid = (np.arange(K) < n) & (cls >= 0) & (cls < nc)
    low = (np.uint32(0xFFFFFFFF) - score_ord(det[:, 4])).astype(np.int64)
    key = np.where(valid, (np.where(valid, cls, 0) << 32) | low, np.int64(nc) << 32)
    tp = np.zeros(K, dtype=np.uint32)
    if m == 0 or n == 0:
        return key, tp
    gcls = _classes(gt[:, 4])
    iou = iou_matrix(det[:n], gt)
    taken = np.zeros((len(thrs), m), dtype=bool)
    for i in range(n):
        if not valid[i]:
            continue
        same = gcls == cls[i]
        if not same.any():
            continue
        v = iou[i]
        for t, thr in enumerate(thrs):
            lim = min(float(thr), 1 - 1e-10)
            tk = taken[0] if shared_taken else taken[t]
            with np.errstate(invalid="ignore"):
                cand = same & ~tk & ((v > lim) if strict else (v >= lim))
            if not cand.any():
                continue
            js = np.flatnonzero(cand & (v == v[cand].max()))
            tk[js[-1] if tie_highest else js[0]] = True
            tp[i] |= np.uint32(1 << t)
    return key, tp


def match_image_scan(det, n, gt, thrs, nc):
    """the same rules as a literal transcription of evaluateImg's loops (slow; cross-checks match_image)"""
    det = np.asarray(det, dtype=np.float32).reshape(-1, 6)
    gt = np.asarray(gt, dtype=np.float32).reshape(-1, 5)
    K, m = det.shape[0], gt.shape[0]
    n = min(max(int(n), 0), K)
    cls, gcls = _classes(det[:, 5]), _classes(gt[:, 4])
    ious = iou_matrix(det[:n], gt) if m and n else np.zeros((n, m))
    tp = np.zeros(K, dtype=np.uint32)
    for tind, t in enumerate(thrs):
        gtm = np.zeros(m, dtype=bool)
        for dind in range(n):
            if not 0 <= cls[dind] < nc:
                continue
            iou, match = min(float(t), 1 - 1e-10), -1
            for gind in range(m):
                if gcls[gind] != cls[dind] or gtm[gind]:
                    continue
                if not ious[dind, gind] >= iou:            # COCOeval: `if ious[dind, gind] < iou: continue`; NaN never matches
                    continue
                iou, match = ious[dind, gind], gind
            if match >= 0:
                gtm[match] = True
                tp[dind] |= np.uint32(1 << tind)
    return tp


def match_batch(det, count, gts, thrs, nc, skip_empty=False, **rules):
    """det fp32 [N][K][6], count [N], gts: N arrays [m][5] -> (key int64 [N][K], tp uint32 [N][K], gt_count int64 [nc], status)"""
    det = np.asarray(det, dtype=np.float32)
    N, K = det.shape[:2]
    key = np.full((N, K), np.int64(nc) << 32, dtype=np.int64)
    tp = np.zeros((N, K), dtype=np.uint32)
    gt_count = np.zeros(nc, dtype=np.int64)
    status = 0
    for b in range(N):
        gt = np.asarray(gts[b], dtype=np.float32).reshape(-1, 5)
        if gt.shape[0] > MAX_GT:
            status = 1
            continue
        if skip_empty and gt.shape[0] == 0:
            continue
        key[b], tp[b] = match_image(det[b], count[b], gt, thrs, nc, **rules)
        gc = _classes(gt[:, 4])
        gt_count += np.bincount(gc[(gc >= 0) & (gc < nc)], minlength=nc)
    return key, tp, gt_count, status


def sort_records(key, tp, stable=True):
    key, tp = np.asarray(key, dtype=np.int64).reshape(-1), np.asarray(tp, dtype=np.uint32).reshape(-1)
    # the unstable stand-in: equal keys in REVERSED insertion order
    order = np.argsort(key, kind="stable") if stable else np.lexsort((-np.arange(key.size), key))
    return key[order], tp[order]


def curve(key, tp, gt_count, nc, n_thr, rec_thrs=REC_THRS, stable=True, envelope=True, side="left"):
    """records in any order -> precision float64 [nc][n_thr][len(rec_thrs)]"""
    key, tp = sort_records(key, tp, stable)
    out = -np.ones((nc, n_thr, len(rec_thrs)))
    cls = key >> 32
    for c in range(nc):
        npig = int(gt_count[c])
        if npig == 0:
            continue
        seg = tp[cls == c]
        nd = seg.size
        for t in range(n_thr):
            tps = ((seg >> np.uint32(t)) & np.uint32(1)).astype(np.float64)
            tp_sum, fp_sum = np.cumsum(tps), np.cumsum(1.0 - tps)
            rc = tp_sum / npig
            pr = tp_sum / (fp_sum + tp_sum + np.spacing(1))
            if envelope:
                for i in range(nd - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
            inds = np.searchsorted(rc, rec_thrs, side=side)
            q = np.zeros(len(rec_thrs))
            for ri, pi in enumerate(inds):
                if pi < nd:
                    q[ri] = pr[pi]
            out[c, t] = q
    return out


def summarize(table, thrs):
    """-> {"mAP50", "mAP50-95", "ap_per_class"} as COCOeval._summarize: means over the entries > -1"""
    def mean(s):
        return float(np.mean(s[s > -1])) if (s > -1).any() else 0.0
    at50 = int(np.flatnonzero(np.asarray(thrs) == 0.5)[0])
    per_class = np.array([float(np.mean(table[c][table[c] > -1])) if (table[c] > -1).any() else -1.0 for c in range(table.shape[0])])
    return {"mAP50": mean(table[:, at50]), "mAP50-95": mean(table), "ap_per_class": per_class}


def evaluate(batches, nc, thrs=IOU_THRS, skip_empty=False, tie_highest=True, strict=False, shared_taken=False, stable=True,
             envelope=True, side="left"):
    """batches: [(det [N][K][6], count [N], gts)] -> (table, summary, status)"""
    keys, tps, gt_count, status = [], [], np.zeros(nc, dtype=np.int64), 0
    for det, count, gts in batches:
        k, t, g, s = match_batch(det, count, gts, thrs, nc, skip_empty=skip_empty, tie_highest=tie_highest, strict=strict,
                                 shared_taken=shared_taken)
        keys.append(k.reshape(-1))
        tps.append(t.reshape(-1))
        gt_count += g
        status |= s
    key = np.concatenate(keys) if keys else np.zeros(0, dtype=np.int64)
    tp = np.concatenate(tps) if tps else np.zeros(0, dtype=np.uint32)
    table = curve(key, tp, gt_count, nc, len(thrs), stable=stable, envelope=envelope, side=side)
    return table, summarize(table, thrs), status


# ------------------------------------------------------------------------------------------------ seeded cases
def xyxy_of(gt):
    g = np.asarray(gt, dtype=np.float32).reshape(-1, 5)
    return np.stack([g[:, 0] - g[:, 2] / 2, g[:, 1] - g[:, 3] / 2, g[:, 0] + g[:, 2] / 2, g[:, 1] + g[:, 3] / 2], 1).astype(np.float32)


def seeded_batch(seed, K, gt_counts, nc, extent=64):
    """A batch on a small integer lattice, so that IoUs are ratios of small integers: many exact ties, values exactly on a
    threshold, duplicated ground truths, rows competing for one ground truth, rows of a wrong or out-of-range class, equal
    scores.  -> (det fp32 [N][K][6] in descending score, count int32 [N], gts: N arrays fp32 [m][5])"""
    rng = np.random.default_rng(seed)
    N = len(gt_counts)
    det = np.zeros((N, K, 6), dtype=np.float32)
    count = np.zeros(N, dtype=np.int32)
    gts = []
    for b, m in enumerate(gt_counts):
        gt = np.zeros((m, 5), dtype=np.float32)
        if m:
            gt[:, 0:2] = rng.integers(4, extent - 4, (m, 2))
            gt[:, 2:4] = 2 * rng.integers(1, 5, (m, 2))                  # even sizes: integer corners
            gt[:, 4] = rng.integers(0, min(nc, 6), m)                    # few classes: crowded matching
            dup = rng.random(m) < 0.2                                    # duplicated ground truths
            gt[dup, :4] = gt[rng.integers(0, m, int(dup.sum())), :4]
            gt[rng.random(m) < 0.03, 4] = nc                             # class outside the range
            gt[rng.random(m) < 0.02, 4] = -1
        gts.append(gt)
        n = int(rng.integers(0, K + 1)) if b % 3 else K
        count[b] = n
        rows = np.zeros((K, 6), dtype=np.float32)
        if m:
            src = rng.integers(0, m, K)
            rows[:, :4] = xyxy_of(gt[src]) + rng.integers(-1, 2, (K, 4))     # jitter by -1, 0, 1: exact rational IoUs
            rows[:, 5] = gt[src, 4]
        else:
            rows[:, :2] = rng.integers(0, extent - 8, (K, 2))
            rows[:, 2:4] = rows[:, :2] + rng.integers(1, 8, (K, 2))
            rows[:, 5] = rng.integers(0, min(nc, 6), K)
        other = rng.random(K) < 0.1
        rows[other, 5] = rng.integers(0, min(nc, 6), int(other.sum()))
        rows[rng.random(K) < 0.03, 5] = nc
        rows[rng.random(K) < 0.02, 5] = -1
        score = np.round(rng.normal(0.0, 2.0, K) * 8) / 8                # logits on a coarse lattice: many equal scores
        rows[:, 4] = -np.sort(-score.astype(np.float32))
        det[b] = rows
    return det, count, gts
