"""What `Model.predict` costs, in alternating windows of one process:

(a) the one-launch letterbox beside the existing two-launch route of the validation transform on 32 decoded 480 x 640 images
    -> 640 x 640 bf16, sources already on the device: `ops.letterbox` beside `ops.image_prep(jitter=0)` as called (each fills and
    uploads its pinned table), and the bare launch sequences `yolo_letterbox` beside `yolo_image_prep` on tables and buffers made
    once (the device's share);
(b) `Model.predict` on one 640 x 640 uint8 picture (preset s, fp16, fused) beside `Model.inference` on the already preprocessed
    tensor: the difference is the whole price of upload, letterbox and inverse map.

    python tools/predict_cost.py [--windows 7] [--calls 200]"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "custom-yolo-implmentation_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import PRESETS  # noqa: E402
from src.data.letterbox import FILL, letterbox_records  # noqa: E402
from src.data.transforms import MEAN, STD, get_val_transforms  # noqa: E402
from src.hipops import lib, ops  # noqa: E402
from src.model.model_builder import Model  # noqa: E402


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def alternate(fns, windows, calls):
    """-> {name: [ms per call of each window]}, the configurations taking turns window by window"""
    for fn in fns.values():                                    # every shape warm before a window is timed
        for _ in range(20):
            fn()
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            out[k].append(window(fn, calls))
    return out


def show(title, res):
    print(title)
    for k, v in res.items():
        print(f"    {k:44s} median {statistics.median(v):.4f} ms   windows {min(v):.4f} ... {max(v):.4f}", flush=True)


def main(args):
    dev = torch.device("cuda:0")
    n, h, w, s = 32, 480, 640, 640
    rng = np.random.default_rng(0)
    flat = torch.from_numpy(rng.integers(0, 256, n * h * w * 3, dtype=np.uint8)).to(dev)
    prep = [(i * h * w * 3, h, w, False, (), (1.0, 1.0, 1.0, 0.0)) for i in range(n)]
    letter, used = letterbox_records([(h, w)] * n, s)
    assert used == flat.numel()
    # the bare launch sequences: tables, staging and outputs made once
    host = torch.zeros(n * lib.query("yolo_prep_image_bytes"), dtype=torch.uint8).pin_memory()
    ops._prep_table_fill(host, prep)
    ptab, ltab = host.to(dev), ops.letter_table(letter, s, used).to(dev)
    stage = torch.empty((n, 3, s, s), dtype=torch.uint8, device=dev)
    means = torch.empty(4 * n, dtype=torch.float32, device=dev)
    out = torch.empty((n, 3, s, s), dtype=torch.bfloat16, device=dev)
    st = ops._stream(flat)
    ms = [float(v) for v in MEAN] + [float(v) for v in STD]
    res = alternate({
        "ops.image_prep(jitter=0)": lambda: ops.image_prep(flat, prep, s, False, torch.bfloat16, MEAN, STD),
        "ops.letterbox": lambda: ops.letterbox(flat, letter, s, FILL, torch.bfloat16, MEAN, STD),
        "yolo_image_prep, launches only": lambda: lib.call("yolo_image_prep", flat.data_ptr(), ptab.data_ptr(), n, s, 0, stage.data_ptr(),
                                                           means.data_ptr(), out.data_ptr(), lib.BF16, *ms, st),
        "yolo_letterbox, launch only": lambda: lib.call("yolo_letterbox", flat.data_ptr(), ltab.data_ptr(), n, s, FILL, out.data_ptr(),
                                                        lib.BF16, *ms, st),
    }, args.windows, args.calls)
    show(f"(a) {n} sources {h}x{w} -> {s}x{s} bf16, per batch", res)

    torch.manual_seed(0)
    model = Model(**PRESETS["s"], num_classes=80).to(dev).eval().fuse().half()
    pic = rng.integers(0, 256, (s, s, 3), dtype=np.uint8)
    x, _ = get_val_transforms(size=s, dtype=torch.float16)([pic])
    conf = 0.6
    thr = math.log(conf / (1 - conf))                          # inside [0, 1], where inference replays
    res = alternate({
        "Model.inference, preprocessed tensor": lambda: model.inference(x, conf_thres=thr),
        "Model.predict, uint8 picture": lambda: model.predict(pic, conf=conf),
    }, args.windows, args.calls)
    show(f"(b) one {s}x{s} picture, preset s, fp16, fused, per call "
         f"({len(model._infer_graphs.entries)} graph entries, capture {'failed: ' + model._infer_graphs.disabled if model._infer_graphs.disabled else 'ok'})", res)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    main(ap.parse_args())
