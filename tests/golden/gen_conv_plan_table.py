#!/usr/bin/env python3
"""Record which kernel yolo_conv2d_plan names for a sweep of shapes, under every tune setting the tests and tools use.

Usage (from the repo root):  python tests/golden/gen_conv_plan_table.py [path/to/libyolo_hip.so]

Writes tests/golden/conv_plan_table.json: per tune setting the SHA-256 of the plan codes in sweep order and the histogram
code -> count.  The queries are host-only (no HIP runtime call), so this runs without a GPU.  The file is a record of what
the dispatch did BEFORE a change to it: generate it from the library of the parent commit, never from the code under test
(tests/test_conv_plan_cpu.py imports the sweep from here and compares).
"""
import ctypes
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "conv_plan_table.json")
DEFAULT_SO = os.path.join(HERE, "..", "..", "custom-yolo-implmentation_amd", "src", "hipops", "libyolo_hip.so")
F32, BF16 = 0, 1

BATCHES = (1, 3, 32)
MAPS = ((7, 9), (20, 20), (23, 20), (13, 40), (40, 40), (37, 41), (80, 80), (84, 100), (160, 160), (320, 320))
CINS = (3, 16, 24, 32, 64, 72, 96, 128, 256, 512)
COUTS = (16, 24, 32, 64, 72, 128, 136, 256, 512)
KERNELS = ((1, 1), (3, 1), (3, 2))
DTYPES = (F32, BF16)
DEFAULT_TUNE = (0, -1, -1, -1, -1, 0, 0, 0)
# every code the planner can return for this sweep: the sweep must keep reaching each family
ALL_CODES = (0, 1032, 1064, 1128, 2001, 2002, 2003, 2004, 3032, 3064, 3128, 3564, 3628, 4001, 4002, 4003, 4004, 4006, 4007,
             5008, 5016)


def tune_settings():
    """(bn, tap_inner, halo, dma, ring, bm, nst, bk) of yolo_conv_tune_set, in the order of the fixture"""
    out = [DEFAULT_TUNE]
    out += [(bn, -1, 0, dma, 0, 0, 0, 0) for bn in (32, 64, 128) for dma in (0, 1)]                      # gather tiles
    out += [(bn, -1, 0, -1, 1, bm, 2, bk) for bn in (32, 64, 128) for bm in (64, 128) for bk in (32, 64)]  # ring tiles
    out += [(0, -1, v, -1, -1, 0, 0, 0) for v in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 14, 15, 16)]          # halo / rows field
    out += [(0, -1, -1, -1, 0, 0, 0, 0), (0, -1, -1, -1, 1, 0, 0, 0)]                                     # ring off / forced
    return out


def queries():
    """argument tuples of yolo_conv2d_plan, in sweep order"""
    for n in BATCHES:
        for h, w in MAPS:
            for cin in CINS:
                for cout in COUTS:
                    for k, s in KERNELS:
                        pad = k // 2
                        oh, ow = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
                        for dt in DTYPES:
                            yield (n, h, w, cin, oh, ow, cout, k, s, 0, 0, dt)
                            for cls in range(4 if s == 2 else 1):
                                yield (n, h, w, cin, oh, ow, cout, k, s, 1, cls, dt)


def open_library(path):
    so = ctypes.CDLL(path)                        # a missing library fails here, with the loader's message
    so.yolo_conv2d_plan.argtypes = [ctypes.c_int] * 12
    so.yolo_conv_tune_set.argtypes = [ctypes.c_int] * 8
    return so


def table(so):
    """{tune setting as "a,b,...": {"sha256": ..., "hist": {code: count}}}; leaves the default tune setting behind"""
    qs = list(queries())
    out = {}
    try:
        for tune in tune_settings():
            so.yolo_conv_tune_set(*tune)
            plan = so.yolo_conv2d_plan
            codes = [plan(*q) for q in qs]
            hist = {}
            for c in codes:
                hist[c] = hist.get(c, 0) + 1
            out[",".join(map(str, tune))] = {"sha256": hashlib.sha256(struct.pack(f"<{len(codes)}i", *codes)).hexdigest(),
                                             "hist": {str(c): hist[c] for c in sorted(hist)}}
    finally:
        so.yolo_conv_tune_set(*DEFAULT_TUNE)
    return out


if __name__ == "__main__":
    t = table(open_library(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_SO))
    with open(OUT, "w") as f:
        json.dump(t, f, indent=1)
        f.write("\n")
    seen = sorted({int(c) for v in t.values() for c in v["hist"]})
    print(f"{len(t)} tune settings x {sum(t[','.join(map(str, DEFAULT_TUNE))]['hist'].values())} queries, codes {seen}")
