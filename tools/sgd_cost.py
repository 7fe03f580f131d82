"""What the optimizer choice costs per step: the bench configuration (preset s, 640x640, bf16, 32 images, captured step)
with HipSGD (Nesterov, warm-up on) versus HipAdamW.  Both steps are captured in ONE process and timed in alternating
windows (adamw, sgd, adamw, sgd, ...), so drift of the box hits both alike; the figure is the difference of the medians.
From bytes SGD moves 20 B per parameter against AdamW's 28, so it should be the cheaper step.

    python tools/sgd_cost.py [--steps 50] [--rounds 7]

Prints one JSON line.  (Kernel rows, when wanted: run this under
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/sgd_cost.py --rounds 2` and look for k_sgd / k_adamw.)"""
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


def make_runner(preset, batch, res, nc, dev, sgd):
    from src.model.losses import PackedTargets, YoloDFLQFLoss
    from src.model.model_builder import Model
    from src.training.fused_adamw import HipAdamW
    from src.training.fused_sgd import HipSGD
    from src.training.graph_step import TrainStepRunner
    torch.manual_seed(0)
    model = Model(**bench.PRESETS[preset], num_classes=nc).to(dev).train()
    if sgd:
        opt = HipSGD(model.parameters(), lr=1e-4, momentum=0.937, weight_decay=1e-4, nesterov=True, warmup_steps=1000)
    else:
        opt = HipAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    img, gts = bench.synthetic_batch(batch, res, nc, 1234, dev)
    runner = TrainStepRunner(model, YoloDFLQFLoss(num_classes=nc, lambda_box=1.5, lambda_cls=1.0), opt, "bfloat16", use_graph=True)
    runner.capture(img, PackedTargets(gts, dev))
    assert runner.graph is not None and runner.opt_in_graph, "the step was not captured with the optimizer inside"
    return runner, opt


def window(runner, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        runner.step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--preset", default="s")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--res", type=int, default=640)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sgd_cost.py needs an MI355X")
    dev = torch.device("cuda", 0)
    adamw, _ = make_runner(args.preset, args.batch, args.res, 80, dev, sgd=False)
    sgd, opt = make_runner(args.preset, args.batch, args.res, 80, dev, sgd=True)
    for r in (adamw, sgd):
        for _ in range(args.warmup):
            r.step()
    t_adamw, t_sgd = [], []
    for _ in range(args.rounds):
        t_adamw.append(window(adamw, args.steps))
        t_sgd.append(window(sgd, args.steps))
    m_adamw, m_sgd = statistics.median(t_adamw), statistics.median(t_sgd)
    elems = sum(p.numel() for g in opt.param_groups for p in g["params"] if p.requires_grad)
    print(json.dumps(dict(config=f"preset {args.preset} {args.res}x{args.res} bf16 batch {args.batch} captured",
                          steps_per_window=args.steps, rounds=args.rounds, stepped_elements=elems,
                          ms_per_step_adamw=[round(t, 4) for t in t_adamw], ms_per_step_sgd=[round(t, 4) for t in t_sgd],
                          median_adamw_ms=round(m_adamw, 4), median_sgd_ms=round(m_sgd, 4),
                          sgd_minus_adamw_us=round(1e3 * (m_sgd - m_adamw), 1),
                          sgd_minus_adamw_percent=round(100 * (m_sgd - m_adamw) / m_adamw, 3),
                          spread_adamw_percent=round(100 * (max(t_adamw) - min(t_adamw)) / m_adamw, 3),
                          sgd_steps=float(opt.state[opt.param_groups[0]["params"][0]]["step"]))), flush=True)


if __name__ == "__main__":
    main()
