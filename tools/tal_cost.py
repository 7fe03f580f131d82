"""What the task-aligned loss costs against the nearest-centre loss, two ways, both in ONE process and in alternating rounds
(old, new, old, new, ...), so drift of the box hits both alike:

  (1) the loss launch sequence alone (value + gradient), `reps` back-to-back launches captured into one hipGraph and
      replayed: N = 32, A = 8400, nc = 80, bf16, random predictions, the synthetic loader's box counts (1..20 per image);
  (2) the captured training step of the bench configuration (preset s, 640 x 640, bf16, 32 images) with each criterion.

    python tools/tal_cost.py [--rounds 7] [--reps 20] [--steps 30] [--no-step]

Prints one JSON line with mean and standard deviation per variant.  (Kernel rows, when wanted: run this under
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/tal_cost.py --rounds 2 --no-step` and look for k_tal_*.)"""
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

import torch  # noqa: E402

import bench  # noqa: E402


def anchors_of(res, dev):
    ax, ay, st = [], [], []
    for s in (8, 16, 32):
        g = res // s
        yy, xx = torch.meshgrid(torch.arange(g), torch.arange(g), indexing="ij")
        ax.append(xx.flatten() + 0.5), ay.append(yy.flatten() + 0.5), st.append(torch.full((g * g,), float(s)))
    return torch.stack([torch.cat(ax), torch.cat(ay)]).to(dev, torch.bfloat16), torch.cat(st).view(1, -1).to(dev, torch.bfloat16)


def loss_graphs(batch, res, nc, reps, dev):
    """-> {name: (graph, out)}: `reps` launches of each loss's forward + gradient on the same inputs"""
    from src.hipops import ops
    from src.model.losses import PackedTargets
    _, gts = bench.synthetic_batch(batch, res, nc, 1234, dev)
    pk = PackedTargets([g.to(dev) for g in gts], dev)
    anchors, strides = anchors_of(res, dev)
    g = torch.Generator().manual_seed(5)
    preds = torch.randn(batch, 64 + nc, anchors.shape[1], generator=g)
    preds[:, 64:] = preds[:, 64:] * 0.7 - 3.5
    preds = preds.to(dev, torch.bfloat16)

    def old():
        return ops.loss_fwd_bwd(preds, anchors, strides, *pk.as_tuple(), nc, 1.5, 1.0, True)[0]

    def new():
        return ops.loss_tal_fwd_bwd(preds, anchors, strides, *pk.as_tuple(), nc, 10, 0.5, 6.0, 7.5, 0.5, 1.5, True)[0]

    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in (("nearest", old), ("tal", new)):
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        side.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=side):
            for _ in range(reps):
                out = fn()
        graphs[name] = (gr, out)
    return graphs, pk.n_gt


def time_graph(gr, reps, replays=5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replays):
        gr.replay()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / (replays * reps)


def make_runner(preset, batch, res, nc, dev, tal):
    from src.model.losses import PackedTargets, YoloDFLQFLoss, YoloTALoss
    from src.model.model_builder import Model
    from src.training.fused_adamw import HipAdamW
    from src.training.graph_step import TrainStepRunner
    torch.manual_seed(0)
    model = Model(**bench.PRESETS[preset], num_classes=nc).to(dev).train()
    opt = HipAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    crit = YoloTALoss(num_classes=nc) if tal else YoloDFLQFLoss(num_classes=nc, lambda_box=1.5, lambda_cls=1.0)
    img, gts = bench.synthetic_batch(batch, res, nc, 1234, dev)
    runner = TrainStepRunner(model, crit, opt, "bfloat16", use_graph=True)
    runner.capture(img, PackedTargets(gts, dev))
    assert runner.graph is not None and runner.opt_in_graph, "the step was not captured with the optimizer inside"
    return runner


def window(runner, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        runner.step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def stats(v, nd):
    return dict(mean=round(statistics.mean(v), nd), stdev=round(statistics.stdev(v), nd) if len(v) > 1 else 0.0,
                rounds=[round(x, nd) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--preset", default="s")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=640)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tal_cost.py needs an MI355X")
    dev = torch.device("cuda", 0)
    graphs, n_gt = loss_graphs(args.batch, args.res, 80, args.reps, dev)
    for gr, _ in graphs.values():
        time_graph(gr, args.reps, 3)
    us = {"nearest": [], "tal": []}
    for _ in range(args.rounds):
        for name in ("nearest", "tal"):
            us[name].append(time_graph(graphs[name][0], args.reps))
    res = dict(config=f"N {args.batch} A {sum((args.res // s) ** 2 for s in (8, 16, 32))} nc 80 bf16, {n_gt} boxes; {args.reps} launches per "
                      f"replay", loss_us_nearest=stats(us["nearest"], 2), loss_us_tal=stats(us["tal"], 2),
               loss_ratio=round(statistics.mean(us["tal"]) / statistics.mean(us["nearest"]), 3),
               out_nearest=[round(float(v), 5) for v in graphs["nearest"][1]], out_tal=[round(float(v), 5) for v in graphs["tal"][1]])
    del graphs
    if not args.no_step:
        runners = {"nearest": make_runner(args.preset, args.batch, args.res, 80, dev, False),
                   "tal": make_runner(args.preset, args.batch, args.res, 80, dev, True)}
        for r in runners.values():
            for _ in range(args.warmup):
                r.step()
        ms = {"nearest": [], "tal": []}
        for _ in range(args.rounds):
            for name in ("nearest", "tal"):
                ms[name].append(window(runners[name], args.steps))
        res.update(step_config=f"preset {args.preset} {args.res}x{args.res} bf16 batch {args.batch} captured, {args.steps} steps per window",
                   step_ms_nearest=stats(ms["nearest"], 4), step_ms_tal=stats(ms["tal"], 4),
                   step_tal_minus_nearest_us=round(1e3 * (statistics.mean(ms["tal"]) - statistics.mean(ms["nearest"])), 1))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
