"""The outputs of the four image_prep leaves as SHA-256 digests: every combination of (tile table, affine table, mix table)
present or absent, each through the narrowest public leaf of src.hipops.ops that takes it, at S = 20 (3 * 20^2 = 1200 bytes per
image: the 16-byte mixup kernel) and S = 33 (3267 bytes: the byte kernel), fp32 and bf16 -- 32 digests.  The sources, tiles, warps
and mix records are those of tests/test_gpu_mixup.py (imported, not copied).  Jitter is off: k_gray_mean sums with float atomics,
and a digest must not depend on their order.

    python tools/record_prep_digests.py --commit $(git rev-parse HEAD) [--out tests/golden/image_prep_routes.json]

writes the file tests/test_gpu_image.py::test_every_route_reproduces_the_recorded_digests holds later commits to.  Record it on an
MI355X from a commit whose outputs are known good (a refactor: from its parent), never from the code under test."""
import argparse
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "custom-yolo-implmentation_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = (20, 33)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "image_prep_routes.json")


def digests():
    """-> {"S20-fp32-tiles0-affine0-mix0": sha256 hex of the output's bytes, ...}"""
    import strict_image as si
    import test_gpu_mixup as gm
    from oracle import image_prep as oip
    from src.hipops import ops
    images = [si.noise(*gm.SOURCES[0], 500)] + si.smooth_images(51, gm.SOURCES[1:])            # test_gpu_mixup's `batch`
    offs = np.concatenate([[0], np.cumsum([im.size for im in images])])
    flat = torch.cat([torch.from_numpy(np.ascontiguousarray(im)).reshape(-1) for im in images]).cuda()
    recs = [(int(offs[i]), im.shape[0], im.shape[1], i == 1, (), gm.NO_JITTER) for i, im in enumerate(images)]
    out = {}
    for S, (name, dtype) in itertools.product(SIZES, DTYPES.items()):
        for has_tiles, has_affine, has_mix in itertools.product((False, True), repeat=3):
            tiles = gm._tiles(S, recs) if has_tiles else None
            affine = gm._warps(S, len(recs)) if has_affine else None
            tail = (S, gm.FILL, False, dtype, oip.MEAN, oip.STD)
            if has_mix:
                got = ops.image_prep_mixup(flat, recs, tiles, affine, gm.RECORDS["chain"], *tail)
            elif has_affine:
                got = ops.image_prep_affine(flat, recs, tiles, affine, *tail)
            elif has_tiles:
                got = ops.image_prep_mosaic(flat, recs, tiles, *tail)
            else:
                got = ops.image_prep(flat, recs, S, False, dtype, oip.MEAN, oip.STD)
            assert got.shape == (len(recs), 3, S, S) and got.dtype == dtype
            raw = got.contiguous().view(torch.uint8).cpu().numpy().tobytes()
            out[f"S{S}-{name}-tiles{int(has_tiles)}-affine{int(has_affine)}-mix{int(has_mix)}"] = hashlib.sha256(raw).hexdigest()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose build computes the digests")
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("record_prep_digests.py needs an MI355X")
    d = digests()
    assert len(d) == 32
    with open(args.out, "w") as f:
        json.dump({"commit": args.commit, "digests": d}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(d)} digests to {args.out}")


if __name__ == "__main__":
    main()
