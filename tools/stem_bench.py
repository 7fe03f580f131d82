"""The stem's three public leaves (stem_conv_fwd with statistics, stem_wgrad, stem_bn_wgrad) on 32 images of 640 x 640 in bf16 at
the stem widths of bench.py's presets (n 16, s 32, l 64, x 96), timed with device events: a warm-up, then seven windows of
--calls back-to-back calls each (a window is tens of milliseconds); one JSON line per (leaf, width) with each window's
per-call time in microseconds.

    python tools/stem_bench.py [--calls 200] [--only stem_wgrad ...] > run.jsonl
    python tools/stem_bench.py --compare parent1.jsonl parent2.jsonl parent3.jsonl --new new1.jsonl new2.jsonl new3.jsonl

To compare two builds of csrc/stem.hip, build the other library to a second path, select it with YOLO_HIP_SO_TMP and run the two in
alternating processes on one MI355X.  --compare prints, per leaf and width, the range of ALL the first build's windows (what the
machine does to identical code: the margin) and the median of the second build's per-process medians, and exits with 1 if one
lies above its range."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "custom-yolo-implmentation_amd"))

WIDTHS = (16, 32, 64, 96)
N, RES, WINDOWS, WARMUP = 32, 640, 7, 200            # a warm-up as long as a window: the first window of the trial ran 10 % slow after 20 calls


def windows(fn, calls):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(round(a.elapsed_time(b) * 1000.0 / calls, 2))
    return out


def measure(calls, only=None):
    import torch
    from src.hipops import ops
    bf16 = torch.bfloat16
    g = torch.Generator().manual_seed(0)
    img = (torch.randn(N, 3, RES, RES, generator=g) + 0.5).cuda()
    for cout in WIDTHS:
        wp = ops.stem_pack_weights((torch.randn(cout, 3, 3, 3, generator=g) * 0.2).cuda(), bf16)
        gamma, beta = torch.ones(cout, device="cuda"), torch.zeros(cout, device="cuda")
        acc = ops.bn_acc_new(cout, "cuda")
        y = ops.stem_conv_fwd(img, wp, cout, bf16, acc)
        rm, rv = torch.zeros(cout, device="cuda"), torch.ones(cout, device="cuda")
        _, mean, invstd, scale, shift = ops.bn_act_fwd_train(y, acc, gamma, beta, rm, rv, 0.03, 1e-3, 1)
        dout = ops.new_nhwc(N, cout, RES // 2, RES // 2, bf16, "cuda")
        dout.copy_(torch.randn(dout.shape, generator=g).to(bf16))
        dw = torch.empty(cout, 3, 3, 3, device="cuda")
        leaves = (("stem_conv_fwd", lambda: ops.stem_conv_fwd(img, wp, cout, bf16, acc)),
                  ("stem_wgrad", lambda: ops.stem_wgrad(img, dout, torch.float32, out=dw)),
                  ("stem_bn_wgrad", lambda: ops.stem_bn_wgrad(img, dout, y, scale, shift, mean, invstd, gamma, 1, torch.float32, out=dw)))
        for name, fn in leaves:
            if only and name not in only:
                continue
            print(json.dumps({"leaf": name, "cout": cout, "calls": calls, "us": windows(fn, calls)}), flush=True)


def read(paths):
    """-> {(leaf, cout): [the windows of one process, ...]}"""
    runs = {}
    for p in paths:
        for line in open(p):
            if line.startswith("{"):
                r = json.loads(line)
                runs.setdefault((r["leaf"], r["cout"]), []).append(r["us"])
    return runs


def compare(old_paths, new_paths):
    old, new = read(old_paths), read(new_paths)
    bad = 0
    for key in old:
        lo, hi = min(min(w) for w in old[key]), max(max(w) for w in old[key])
        mm_old = statistics.median(statistics.median(w) for w in old[key])
        mm_new = statistics.median(statistics.median(w) for w in new[key])
        bad += mm_new > hi
        print(f"{key[0]:14s} c{key[1]:<3d} first build {lo:7.2f} .. {hi:7.2f} us (median of medians {mm_old:7.2f})   "
              f"second build {mm_new:7.2f} us   {'ABOVE' if mm_new > hi else 'below' if mm_new < lo else 'inside'}")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--only", nargs="+", help="leaves to time (default: all three)")
    ap.add_argument("--compare", nargs="+", help="result files of the first build")
    ap.add_argument("--new", nargs="+", help="result files of the second build")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare, args.new))
    measure(args.calls, args.only)
