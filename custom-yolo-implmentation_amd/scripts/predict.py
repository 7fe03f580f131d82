#!/usr/bin/env python3
"""Detect objects in pictures of any size with `Model.predict` and write COCO result records.

    python scripts/predict.py --weights W --source DIR_OR_FILE [--conf 0.25 --iou 0.45 --size 640 --batch 8 --fuse --half]
                              --out detections.json

Every picture is letterboxed on the device, the boxes come back in its own pixel coordinates and the score is a probability
(src/model/model_builder.py::Model.predict).  The output is a JSON list of
    {"file": name, "category_id": class index, "bbox": [x, y, w, h], "score": probability}
-- COCO's result format with the file name in the image id's place (no reference counterpart: the reference has no script that
runs its `Model.inference`, src/model/model_builder.py:115-139, over pictures)."""
import argparse
import json
import os
import sys

sys.path.append(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png", ".bmp", ".webp")


def coco_records(name, rows):
    """`Model.predict`'s rows of one picture ([x1, y1, x2, y2, confidence, class], any sequence of six numbers per row)
    -> COCO result records: bbox = [x, y, w, h] in pixels, rounded to two decimals as pycocotools' writers do, the score
    to five, rows in their order (descending score)."""
    out = []
    for x1, y1, x2, y2, score, cls in (tuple(float(v) for v in r) for r in rows):
        out.append({"file": name, "category_id": int(cls), "bbox": [round(x1, 2), round(y1, 2), round(x2 - x1, 2), round(y2 - y1, 2)],
                    "score": round(score, 5)})
    return out


def list_sources(source):
    """A picture, or the pictures of a directory in name order."""
    if os.path.isdir(source):
        names = sorted(n for n in os.listdir(source) if n.lower().endswith(IMAGE_SUFFIXES))
        if not names:
            raise SystemExit(f"no pictures ({', '.join(IMAGE_SUFFIXES)}) in {source}")
        return [os.path.join(source, n) for n in names]
    if not os.path.isfile(source):
        raise SystemExit(f"--source {source}: no such file or directory")
    return [source]


def main(args):
    from src.model.model_builder import Model
    from src.utils.config_loader import load_config
    cfg = load_config(args.config)["model"]
    model = Model(**cfg["config"], num_classes=cfg["num_classes"]).to("cuda")
    model.load_weights(args.weights)
    model.eval()
    if args.fuse:
        model.fuse()
    if args.half:
        model.half()
    size = args.size if args.size is not None else int(cfg.get("input_size", [Model.input_size])[0])
    paths = list_sources(args.source)
    records = []
    for lo in range(0, len(paths), args.batch):
        chunk = paths[lo:lo + args.batch]
        dets = model.predict(chunk, conf=args.conf, iou=args.iou, size=size, batch=args.batch)
        for p, d in zip(chunk, dets):
            records += coco_records(os.path.basename(p), d.tolist())
    with open(args.out, "w") as f:
        json.dump(records, f)
    print(f"{len(records)} detections in {len(paths)} pictures -> {args.out}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="Run Model.predict over a picture or a directory of pictures.")
    ap.add_argument("--weights", type=str, required=True, help="checkpoint written by training (or a bare state dict)")
    ap.add_argument("--source", type=str, required=True, help="a picture or a directory of pictures")
    ap.add_argument("--config", type=str, default="config.yaml", help="YAML configuration with the model section")
    ap.add_argument("--conf", type=float, default=0.25, help="confidence threshold, a probability in (0, 1)")
    ap.add_argument("--iou", type=float, default=0.45, help="NMS IoU threshold")
    ap.add_argument("--size", type=int, default=None, help="side of the square canvas (default: the config's input_size)")
    ap.add_argument("--batch", type=int, default=8, help="pictures per replay")
    ap.add_argument("--fuse", action="store_true", help="fold BatchNorm into the convs")
    ap.add_argument("--half", action="store_true", help="fp16 weights and activations")
    ap.add_argument("--out", type=str, required=True, help="JSON file of COCO result records")
    main(ap.parse_args())
