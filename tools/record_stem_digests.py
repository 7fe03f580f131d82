"""The outputs of the stem's three fused kernels as SHA-256 digests: the cases, inputs and outputs are those of
tests/test_gpu_stem_digests.py (imported, not copied) -- 7 cases x 7 outputs = 49 digests.

    python tools/record_stem_digests.py --commit $(git rev-parse HEAD) [--out tests/golden/stem_routes.json]

writes the file tests/test_gpu_stem_digests.py holds later commits to.  Record it on an MI355X from a commit whose outputs are
known good (a refactor: from its parent), never from the code under test."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "custom-yolo-implmentation_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    import test_gpu_stem_digests as sd
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose build computes the digests")
    ap.add_argument("--out", default=sd.GOLDEN)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("record_stem_digests.py needs an MI355X")
    d = sd.digests()
    assert len(d) == len(sd.CASES) * len(sd.OUTPUTS)
    with open(args.out, "w") as f:
        json.dump({"commit": args.commit, "digests": d}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(d)} digests to {args.out}")


if __name__ == "__main__":
    main()
