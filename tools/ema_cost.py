"""What the weight EMA costs per step: the bench configuration (preset s, 640x640, bf16, 32 images, captured step) with a
ModelEMA over the optimizer (HipAdamW(ema_decay=...): the average of the parameters inside k_adamw, one k_ema_lerp launch
for the BatchNorm statistics) versus none.  Both steps are captured in ONE process and timed in alternating windows
(off, on, off, on, ...), so drift of the box hits both alike; the figure is the difference of the medians.

    python tools/ema_cost.py [--steps 50] [--rounds 7] [--decay 0.9999] [--tau 2000]

Prints one JSON line.  (Kernel rows, when wanted: run this under
`rocprofv3 --kernel-trace --stats -d DIR -- python tools/ema_cost.py --rounds 2` and compare k_adamw of the two runners;
k_ema_lerp is the added launch.)"""
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


def make_runner(preset, batch, res, nc, dev, ema_cfg):
    from src.model.losses import PackedTargets, YoloDFLQFLoss
    from src.model.model_builder import Model
    from src.training.fused_adamw import HipAdamW
    from src.training.graph_step import TrainStepRunner
    torch.manual_seed(0)
    model = Model(**bench.PRESETS[preset], num_classes=nc).to(dev).train()
    opt = HipAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    ema = None
    if ema_cfg is not None:
        from src.training.ema import ModelEMA
        ema = ModelEMA(model, opt, decay=ema_cfg[0], tau=ema_cfg[1])
    img, gts = bench.synthetic_batch(batch, res, nc, 1234, dev)
    runner = TrainStepRunner(model, YoloDFLQFLoss(num_classes=nc, lambda_box=1.5, lambda_cls=1.0), opt, "bfloat16", use_graph=True)
    runner.capture(img, PackedTargets(gts, dev))
    assert runner.graph is not None and runner.opt_in_graph, "the step was not captured with the optimizer inside"
    return runner, ema


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
    ap.add_argument("--decay", type=float, default=0.9999)
    ap.add_argument("--tau", type=float, default=2000.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_cost.py needs an MI355X")
    dev = torch.device("cuda", 0)
    off, _ = make_runner(args.preset, args.batch, args.res, 80, dev, None)
    on, ema = make_runner(args.preset, args.batch, args.res, 80, dev, (args.decay, args.tau))
    for r in (off, on):
        for _ in range(args.warmup):
            r.step()
    t_off, t_on = [], []
    for _ in range(args.rounds):
        t_off.append(window(off, args.steps))
        t_on.append(window(on, args.steps))
    m_off, m_on = statistics.median(t_off), statistics.median(t_on)
    print(json.dumps(dict(config=f"preset {args.preset} {args.res}x{args.res} bf16 batch {args.batch} captured",
                          steps_per_window=args.steps, rounds=args.rounds,
                          ms_per_step_off=[round(t, 4) for t in t_off], ms_per_step_on=[round(t, 4) for t in t_on],
                          median_off_ms=round(m_off, 4), median_on_ms=round(m_on, 4),
                          cost_us=round(1e3 * (m_on - m_off), 1), cost_percent=round(100 * (m_on - m_off) / m_off, 3),
                          spread_off_percent=round(100 * (max(t_off) - min(t_off)) / m_off, 3),
                          ema_updates=ema.updates, ema_tensors=len(ema._pairs()[0]),
                          ema_elements=sum(t.numel() for t in ema._pairs()[0]))), flush=True)


if __name__ == "__main__":
    main()
