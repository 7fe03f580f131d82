"""Run-to-run spread of the global gradient norm of ONE eager training step (nano preset, 2x3x160x160, fp32) from
identical weights on an identical batch: the batch and seeds of tests/test_gpu_grad_clip.py's model-level cases.  The
spread comes from the float-atomic BatchNorm statistics; 4x the figure printed here is the bound those tests put on the
device norm of a captured, clipped step against torch's norm on an eager twin.

    python tools/grad_norm_spread.py [--runs 8]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "custom-yolo-implmentation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

NANO = dict(csp=[False, True], depth=[1] * 6, width=[3, 16, 32, 64, 128, 256])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8)
    args = ap.parse_args()
    from src.model.losses import YoloDFLQFLoss
    from src.model.model_builder import Model
    from src.training.fused_adamw import HipAdamW
    from src.training.graph_step import TrainStepRunner
    g = torch.Generator().manual_seed(21)
    counts = [3, 5]
    img = torch.randn(len(counts), 3, 160, 160, generator=g).cuda()
    gts = [torch.cat([torch.rand(c, 2, generator=g) * 160, torch.rand(c, 2, generator=g) * 60 + 8,
                      torch.randint(0, 80, (c, 1), generator=g).float()], 1).cuda() for c in counts]
    torch.manual_seed(0)
    first = Model(**NANO, num_classes=80).cuda().train()
    state = {k: v.clone() for k, v in first.state_dict().items()}
    norms = []
    for _ in range(args.runs):
        m = Model(**NANO, num_classes=80).cuda().train()
        m.load_state_dict(state)
        opt = HipAdamW(m.parameters(), lr=1e-4, weight_decay=1e-2)
        r = TrainStepRunner(m, YoloDFLQFLoss(num_classes=80), opt, "float32", use_graph=False)
        opt.zero_grad(set_to_none=True)
        r._fwd_bwd(img, gts)
        norms.append(float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters() if p.grad is not None))))
    mean = sum(norms) / len(norms)
    pair = max(abs(x - y) for x, y in zip(norms[:-1], norms[1:])) / mean
    print("norms:", " ".join(f"{n:.10g}" for n in norms))
    print(f"relative spread: largest difference between two consecutive runs {pair:.3e}, "
          f"max - min over {len(norms)} runs {(max(norms) - min(norms)) / mean:.3e}")


if __name__ == "__main__":
    main()
