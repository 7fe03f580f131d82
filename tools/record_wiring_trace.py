"""Record the launch traces of this checkout (tests/wiring_trace.py: the eleven blocks of test_block_wiring in full,
call counts and digest of the n320 training step) into tests/golden/wiring_trace.json.  CPU only.

The fixture is the EXPECTATION of tests/test_backward_plan_cpu.py, so it is recorded from the commit a change to the
host wiring starts from, never from the changed code:

    python tools/record_wiring_trace.py --commit "$(git rev-parse HEAD)" [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402,F401  (puts the repository and the package on sys.path)
import pytest  # noqa: E402
import wiring_trace as wt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit this checkout is at (stored in the fixture)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "wiring_trace.json"))
    args = ap.parse_args()
    mp = pytest.MonkeyPatch()
    doc = {"commit": args.commit, "leaves": wt.traced_leaves(),
           "blocks": {tag: wt.block_trace(mp, tag) for tag in wt.BLOCK_TAGS},
           "model_n320": wt.summary(wt.model_trace(mp))}
    with open(args.out, "w") as f:
        f.write("{\n")
        f.write(f' "commit": {json.dumps(doc["commit"])},\n "leaves": {json.dumps(doc["leaves"])},\n "blocks": {{\n')
        for i, (tag, recs) in enumerate(doc["blocks"].items()):
            f.write(f'  {json.dumps(tag)}: [\n   ' + ",\n   ".join(wt.canonical([r])[1:-1] for r in recs) + "\n  ]"
                    + ("," if i + 1 < len(doc["blocks"]) else "") + "\n")
        f.write(f' }},\n "model_n320": {json.dumps(doc["model_n320"], sort_keys=True)}\n}}\n')
    print(f"{args.out}: {sum(len(r) for r in doc['blocks'].values())} block records, "
          f"{sum(doc['model_n320']['counts'].values())} model records, sha256 {doc['model_n320']['sha256'][:16]}...")


if __name__ == "__main__":
    main()
