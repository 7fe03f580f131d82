"""What the mosaic costs per batch: `BatchTransform` on 32 decoded images 480x640 -> 640x640 bf16 including the pinned upload
(the figure tests/test_gpu_input_pipeline.py::test_sampled_decisions_bf16_output_and_throughput prints), plain versus
`mosaic={"p": 1, "gain": [lo, hi]}`.  Both transforms live in ONE process and are timed in alternating windows (plain,
mosaic, plain, ...), so drift of the box hits both alike.  The mosaic decisions are drawn once and reused, like the plain
ones, so the windows time the upload and the launches, not the host RNG.

    python tools/mosaic_cost.py [--batches 10] [--rounds 7] [--gain 0.4 1.0] [--plain-only] [--affine] [--mixup] [--leaf]

`--gain 1 1` keeps every tile at the plain resize's scale (same taps per pixel as the plain path, fewer pixels sampled):
with it the difference to the default gain separates the larger antialias footprints of shrunken tiles from the cost of
the quadrant test and the divergence at the quadrant edges.  `--plain-only` times the plain path alone (a checkout without
the mosaic).  `--affine` adds the warp's two batches to the alternation: `affine={"degrees": 10, "shear": 2}` behind the plain
resize and behind the mosaic, decisions drawn once (kernel rows: k_affine beside k_resize_flip / k_mosaic; it reads and writes
N * 3 * S * S bytes).  `--mixup` adds the mixup's batches: `mixup={"p": 1}`, every output mixed with a
partner drawn once, behind the plain resize and behind mosaic + warp (kernel row: k_mixup; it reads 2 and writes 1 x N * 3 * S * S
bytes).  Beside the time per batch up to the window's closing synchronise, every configuration reports the time the host spent inside
`BatchTransform.__call__` (`host_ms_per_batch_*`); `--leaf` adds, per configuration, the `src.hipops.ops` leaf alone with the batch
already on the device (`leaf_*`: table packing, allocations and launches).  Prints one JSON line.  (Kernel rows: run under `rocprofv3 --kernel-trace --stats -d DIR -- python
tools/mosaic_cost.py --rounds 2` and compare k_resize_flip with k_mosaic.)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "custom-yolo-implmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def images(seed, n, h, w):
    """smooth content + noise, as the input-pipeline tests make their sources"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 100 * np.sin(xx / (7.0 + c) + yy / 13.0) for c in range(3)], -1)
    return [torch.from_numpy(np.clip(base + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)) for _ in range(n)]


def window(call, batches):
    """-> (ms per batch up to the closing synchronise, ms per batch the host spent inside `call`: enqueueing, not the device's work)"""
    torch.cuda.synchronize()
    host = 0.0
    t0 = time.perf_counter()
    for _ in range(batches):
        t1 = time.perf_counter()
        call()
        host += time.perf_counter() - t1
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / batches, 1e3 * host / batches


def leaf_alone(call, names=("image_prep", "image_prep_mosaic", "image_prep_affine", "image_prep_mixup")):
    """`call` runs a transform once -> a callable that repeats the src.hipops.ops leaf it took with the same arguments (the batch
    already on the device): the table packing, the allocations and the launches without the transform's host work and upload"""
    from src.hipops import ops
    seen = []
    real = {n: getattr(ops, n) for n in names}
    for n in names:
        setattr(ops, n, lambda *a, _n=n: seen.append((_n, a)) or real[_n](*a))
    try:
        call()
    finally:
        for n in names:
            setattr(ops, n, real[n])
    (name, args), = seen
    return lambda: real[name](*args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--gain", type=float, nargs=2, default=[0.4, 1.0])
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--affine", action="store_true")
    ap.add_argument("--mixup", action="store_true")
    ap.add_argument("--leaf", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mosaic_cost.py needs an MI355X")
    from src.data.transforms import BatchTransform
    imgs = images(3, args.batch, 480, 640)
    plain = BatchTransform(True, size=640, device="cuda", dtype=torch.bfloat16)
    torch.manual_seed(11)
    params = [plain.sample() for _ in imgs]
    calls = {"plain": lambda: plain(imgs, params=params)}
    if not args.plain_only:
        mos = BatchTransform(True, size=640, device="cuda", dtype=torch.bfloat16, mosaic={"p": 1.0, "gain": args.gain})
        draws = mos.sample_mosaic(len(imgs))
        calls["mosaic"] = lambda: mos(imgs, params=params, mosaic=draws)
    if args.affine:
        acfg = {"degrees": 10.0, "shear": 2.0}
        aff = BatchTransform(True, size=640, device="cuda", dtype=torch.bfloat16, affine=acfg)
        warps = aff.sample_affine(len(imgs))
        calls["affine"] = lambda: aff(imgs, params=params, affine=warps)
        if not args.plain_only:
            both = BatchTransform(True, size=640, device="cuda", dtype=torch.bfloat16, mosaic={"p": 1.0, "gain": args.gain}, affine=acfg)
            calls["mosaic_affine"] = lambda: both(imgs, params=params, mosaic=draws, affine=warps)
    if args.mixup:
        acfg = {"degrees": 10.0, "shear": 2.0}
        mix = BatchTransform(True, size=640, device="cuda", dtype=torch.bfloat16, mixup={"p": 1.0})
        pairs = mix.sample_mixup(len(imgs))
        calls["mixup"] = lambda: mix(imgs, params=params, mixup=pairs)
        if not args.plain_only:
            if "mosaic_affine" not in calls:
                both = BatchTransform(True, size=640, device="cuda", dtype=torch.bfloat16, mosaic={"p": 1.0, "gain": args.gain}, affine=acfg)
                warps = both.sample_affine(len(imgs))
                calls["mosaic_affine"] = lambda: both(imgs, params=params, mosaic=draws, affine=warps)
            every = BatchTransform(True, size=640, device="cuda", dtype=torch.bfloat16, mosaic={"p": 1.0, "gain": args.gain}, affine=acfg,
                                   mixup={"p": 1.0})
            calls["mosaic_affine_mixup"] = lambda: every(imgs, params=params, mosaic=draws, affine=warps, mixup=pairs)
    if args.leaf:
        calls.update({f"leaf_{k}": leaf_alone(call) for k, call in list(calls.items())})
    for call in calls.values():
        for _ in range(args.warmup):
            call()
    times, host = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, call in calls.items():
            wall, inside = window(call, args.batches)
            times[k].append(wall)
            host[k].append(inside)
    out = dict(config=f"{args.batch} images 480x640 -> 640x640 bf16 incl. pinned upload", batches_per_window=args.batches,
               rounds=args.rounds)
    for k, t in times.items():
        m = statistics.median(t)
        out[f"ms_per_batch_{k}"] = [round(v, 3) for v in t]
        out[f"median_{k}_ms"] = round(m, 3)
        out[f"spread_{k}_percent"] = round(100 * (max(t) - min(t)) / m, 2)
        out[f"images_per_s_{k}"] = round(1e3 * args.batch / m)
        out[f"host_ms_per_batch_{k}"] = [round(v, 3) for v in host[k]]
        out[f"median_host_{k}_ms"] = round(statistics.median(host[k]), 3)
    if "mosaic" in times:
        out["gain"] = args.gain
        out["mosaic_over_plain"] = round(out["median_mosaic_ms"] / out["median_plain_ms"], 3)
    for k in ("affine", "mosaic_affine", "mixup", "mosaic_affine_mixup"):
        if k in times:
            out[f"{k}_over_plain"] = round(out[f"median_{k}_ms"] / out["median_plain_ms"], 3)
    if "mosaic_affine_mixup" in times:
        out["mosaic_affine_mixup_over_mosaic_affine"] = round(out["median_mosaic_affine_mixup_ms"] / out["median_mosaic_affine_ms"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
