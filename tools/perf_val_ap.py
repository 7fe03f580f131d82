"""What `training.val_ap` costs on the MI355X, two figures:

  (1) per validation batch of 32 images at 640 x 640, preset s, bf16, UNTRAINED weights -- the worst case: at conf = 0.001
      the cut is the logit -6.9 and every anchor of a fresh head is a candidate -- the added work (head decode, class-aware
      NMS, `DetectionAP.update_batch`) beside the validation forward of the same batch, in alternating windows;
  (2) `DetectionAP.compute()` (concatenate, stable sort, table, the one copy) for 5000 images x 300 rows with 36 000 ground
      truths in 80 classes, and the 50 `update_batch` calls of 100 images that feed it.

    python tools/perf_val_ap.py [--rounds 5] [--steps 10]

Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "custom-yolo-implmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import bench  # noqa: E402


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def stats(v):
    return dict(mean=round(statistics.mean(v), 4), stdev=round(statistics.stdev(v), 4) if len(v) > 1 else 0.0)


def per_batch(args, dev):
    from src.hipops import ops
    from src.model.model_builder import Model
    from src.training.metrics import DetectionAP
    nc = 80
    torch.manual_seed(0)
    model = Model(**bench.PRESETS[args.preset], num_classes=nc).to(dev).eval()
    img, gts = bench.synthetic_batch(args.batch, args.res, nc, 1234, dev)
    gts = [g.to(dev) for g in gts]
    ap = DetectionAP(nc)
    thr = math.log(0.001 / 0.999)
    out = {}

    def forward():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            out["p"] = model(img)

    def added():
        preds, anchors, strides = out["p"]
        y = ops.head_decode(preds, anchors, strides, nc)
        rows, count, _ = ops.nms(y, nc, thr, 0.7, None, False, False, 300)
        ap.update_batch(rows, count, gts)
        out["count"] = count

    for _ in range(3):
        forward()
        added()
    ms = {"forward": [], "nms_ap_match": []}
    for _ in range(args.rounds):
        ms["forward"].append(window(forward, args.steps))
        ms["nms_ap_match"].append(window(added, args.steps))
        ap.reset()
    anchors = sum((args.res // s) ** 2 for s in (8, 16, 32))
    return dict(batch_config=f"preset {args.preset} {args.res}x{args.res} bf16 eval, untrained, batch {args.batch}, {anchors} anchors, "
                             f"conf 0.001 nms_iou 0.7 max_det 300, {sum(int(g.shape[0]) for g in gts)} boxes",
                rows_kept_per_image=round(float(out["count"].float().mean()), 1), forward_ms=stats(ms["forward"]),
                nms_ap_match_ms=stats(ms["nms_ap_match"]))


def whole_compute(args, dev):
    from src.training.metrics import DetectionAP
    nc, n_img, per, K, n_gt = 80, 5000, 100, 300, 36000
    g = torch.Generator().manual_seed(7)
    ap = DetectionAP(nc)
    batches = []
    for b in range(n_img // per):
        m = n_gt // (n_img // per)                                          # 720 boxes per batch, spread unevenly
        owner = torch.randint(0, per, (m,), generator=g)
        sizes = torch.bincount(owner, minlength=per).tolist()
        gt = torch.cat([torch.rand(m, 2, generator=g) * 560 + 40, torch.rand(m, 2, generator=g) * 200 + 16,
                        torch.randint(0, nc, (m, 1), generator=g).float()], 1)
        targets = list(torch.split(gt, sizes))
        rows = torch.zeros(per, K, 6)
        for i, t in enumerate(targets):                                     # rows: jittered copies of the image's boxes
            src = t[torch.randint(0, max(len(t), 1), (K,), generator=g)] if len(t) else torch.zeros(K, 5)
            c = src[:, :2] + torch.randn(K, 2, generator=g) * 12
            wh = src[:, 2:4] * (1 + 0.2 * torch.randn(K, 2, generator=g)).clamp(0.3, 2.0)
            rows[i, :, :2], rows[i, :, 2:4], rows[i, :, 5] = c - wh / 2, c + wh / 2, src[:, 4]
            rows[i, :, 4] = torch.sort(torch.randn(K, generator=g), descending=True)[0]
        batches.append((rows.to(dev), torch.full((per,), K, dtype=torch.int32, device=dev), [t.to(dev) for t in targets]))

    def feed():
        ap.reset()
        for rows, count, targets in batches:
            ap.update_batch(rows, count, targets)

    feed()
    res = ap.compute()
    upd, cmp_ = [], []
    for _ in range(args.rounds):
        upd.append(window(feed, 1))
        cmp_.append(window(ap.compute, 1))
    return dict(compute_config=f"{n_img} images x {K} rows, {n_gt} boxes, {nc} classes, 10 thresholds; {len(batches)} update_batch "
                               f"calls of {per} images", update_batches_ms=stats(upd), compute_ms=stats(cmp_),
                mAP50=round(res["mAP50"], 4), mAP50_95=round(res["mAP50-95"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--preset", default="s")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=640)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_val_ap.py needs an MI355X")
    dev = torch.device("cuda", 0)
    res = per_batch(args, dev)
    res.update(whole_compute(args, dev))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
