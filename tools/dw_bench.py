"""Depthwise 3x3 kernels (forward, data gradient, weight gradient + finalize) on the head / PSA shapes of preset s at 32
images: the strip and the rows variants (yolo_dw_tune_set) timed per shape in ONE process, in alternating rounds of
graph-replayed launches, beside a yardstick that moves the same bytes -- the eval BatchNorm forward (bn_act_fwd: one read,
one write) on the same tensor.  Each kernel is reported in microseconds (median over the rounds) and as a multiple of the
yardstick; the totals carry the spread (standard deviation over the rounds) of each variant.

    python tools/dw_bench.py [--rounds 7] [--launches 20]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "custom-yolo-implmentation_amd"))
import torch  # noqa: E402
from src.hipops import lib, ops  # noqa: E402

SHAPES = [(128, 80), (128, 80), (256, 40), (128, 40), (512, 20), (128, 20), (128, 20)]   # (C, H = W): the seven layers
VARIANTS = (("strip", 1), ("rows", 2))
KINDS = ("fwd", "dgrad", "wgrad")


def graph_of(fn, launches):
    """`launches` calls of fn captured into one graph (the variant is chosen at capture time, by the host launcher)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    return g


def time_us(g, launches, replays=3):
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / (replays * launches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--images", type=int, default=32)
    a = ap.parse_args()
    n = a.images
    totals = {(v, k): [0.0] * a.rounds for v, _ in VARIANTS for k in KINDS}
    total_bn = [0.0] * a.rounds
    total_ideal = 0.0
    for (c, h) in SHAPES:
        x = torch.randn(n, c, h, h, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
        dy = torch.randn_like(x)
        w9 = torch.randn(c, 9, device="cuda") * 0.2
        scale, shift = torch.rand(c, device="cuda") + 0.5, torch.randn(c, device="cuda")
        ideal = 2 * x.numel() * 2 / 6.29e6                                       # one read + one write at the measured stream rate
        fns = {"fwd": lambda: ops.dw_fwd(x, w9), "dgrad": lambda: ops.dw_dgrad(dy, w9), "wgrad": lambda: ops.dw_wgrad(x, dy)}
        graphs = {}
        for name, variant in VARIANTS:
            lib.call("yolo_dw_tune_set", variant)
            for k in KINDS:
                graphs[(name, k)] = graph_of(fns[k], a.launches)
        lib.call("yolo_dw_tune_set", 0)
        graphs["bn"] = graph_of(lambda: ops.bn_act_fwd(x, scale, shift, 1), a.launches)
        t = {key: [] for key in graphs}
        for _ in range(a.rounds):                                                # alternating: every graph once per round
            for key, g in graphs.items():
                t[key].append(time_us(g, a.launches))
        bn = statistics.median(t["bn"])
        line = f"C {c:4d} {h}x{h}: bn_act_fwd {bn:6.1f} us (ideal {ideal:5.1f})"
        for k in KINDS:
            s, r = statistics.median(t[("strip", k)]), statistics.median(t[("rows", k)])
            line += f" | {k} strip {s:6.1f} (x{s / bn:4.2f}) rows {r:6.1f} (x{r / bn:4.2f})"
        print(line, flush=True)
        for i in range(a.rounds):
            total_bn[i] += t["bn"][i]
            for name, _ in VARIANTS:
                for k in KINDS:
                    totals[(name, k)][i] += t[(name, k)][i]
        total_ideal += ideal
        plan = [lib.query("yolo_dw_plan", n, h, h, c, f) for f in range(12)]
        took = {1: "rows", 2: "strip"}
        print(f"       default: forward / data gradient {took[plan[0]]}, weight gradient {took[lib.query('yolo_dw_plan', n, h, h, c, 12)]}")
        print(f"       plan: ncol {plan[1]} x {plan[2]} blocks, {plan[4]} threads, bands {plan[5]} rows x {plan[6]} (grid {plan[7]}), "
              f"wgrad bands {plan[8]} rows x {plan[9]} (grid {plan[10]})", flush=True)
    bn = statistics.median(total_bn)
    print(f"TOTAL over the seven layers: bn_act_fwd {bn:.1f} us, ideal {total_ideal:.1f} us at 6.29 TB/s")
    for k in KINDS:
        s, r = totals[("strip", k)], totals[("rows", k)]
        ms, mr = statistics.median(s), statistics.median(r)
        print(f"TOTAL {k:5s}: strip {ms:6.1f} us (sd {statistics.pstdev(s):.2f}, x{ms / bn:4.2f} of bn) | rows {mr:6.1f} us "
              f"(sd {statistics.pstdev(r):.2f}, x{mr / bn:4.2f}) | strip - rows {ms - mr:6.1f} us = {(ms - mr) / max(statistics.pstdev(s), 1e-9):.1f} "
              f"strip sd", flush=True)


if __name__ == "__main__":
    main()
