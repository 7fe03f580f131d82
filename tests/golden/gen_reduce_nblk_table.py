#!/usr/bin/env python3
"""Record yolo_reduce_nblk(npix, C), the workgroup count of the row-strided reduction kernels, for a sweep of sizes.

Usage (from the repo root):  python tests/golden/gen_reduce_nblk_table.py [path/to/libyolo_hip.so]

Writes tests/golden/reduce_nblk_table.json: {"npix": [...], "C": [...], "nblk": [[row per npix, column per C]]}.  The
query is host-only (no HIP runtime call), so this runs without a GPU.  The file is a record of what the grid sizing did
BEFORE a change to it: generate it from the library of the parent commit, never from the code under test
(tests/test_cabi_cpu.py compares the library's answers with it).
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reduce_nblk_table.json")
DEFAULT_SO = os.path.join(HERE, "..", "..", "custom-yolo-implmentation_amd", "src", "hipops", "libyolo_hip.so")
NPIX = (1, 31, 32, 33, 429, 4096, 22000, 51200, 819200, 3276800, 10 ** 7)
CS = (3, 6, 8, 16, 24, 64, 96, 128, 264, 512, 1024, 2056)


if __name__ == "__main__":
    so = ctypes.CDLL(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_SO)   # a missing library fails here, with the loader's message
    so.yolo_reduce_nblk.argtypes = [ctypes.c_long, ctypes.c_int]
    t = {"npix": list(NPIX), "C": list(CS), "nblk": [[so.yolo_reduce_nblk(p, c) for c in CS] for p in NPIX]}
    with open(OUT, "w") as f:
        json.dump(t, f)
        f.write("\n")
    print(f"{len(NPIX)} x {len(CS)} queries, nblk {min(map(min, t['nblk']))}..{max(map(max, t['nblk']))}")
