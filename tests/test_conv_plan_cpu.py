"""No-GPU pin of the conv dispatch table: yolo_conv2d_plan over a sweep of shapes, under every tune setting the variant tests
and the tools use, against tests/golden/conv_plan_table.json -- a record made from the library of the commit BEFORE the
dispatch was last changed (tests/golden/gen_conv_plan_table.py; never regenerated from the code under test).  The plan query
and yolo_conv_tune_set call nothing in the HIP runtime, so the cross-compiled library answers here."""
import importlib.util
import json
import os

import pytest

from src.hipops import lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_conv_plan_table", os.path.join(GOLDEN, "gen_conv_plan_table.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def tables(request):
    so = gen.open_library(lib.SO_PATH)            # needs the built library: a missing one is the loader's error, not a skip
    request.addfinalizer(lambda: so.yolo_conv_tune_set(*gen.DEFAULT_TUNE))     # the tune state is process-wide
    return gen.table(so), json.load(open(os.path.join(GOLDEN, "conv_plan_table.json")))


def test_plan_table_matches_the_recorded_one(tables):
    got, want = tables
    assert list(got) == list(want) == [",".join(map(str, t)) for t in gen.tune_settings()]
    bad = []
    for key in want:
        g, w = got[key], want[key]
        if g != w:
            diff = {c: (w["hist"].get(c, 0), g["hist"].get(c, 0)) for c in sorted(set(w["hist"]) | set(g["hist"]), key=int)
                    if w["hist"].get(c, 0) != g["hist"].get(c, 0)}
            bad.append(f"tune {key}: code -> (recorded, now) {diff or 'same histogram, other order'}")
    assert not bad, "\n".join(bad)


def test_sweep_reaches_every_plan_code(tables):
    got, want = tables
    for t in (got, want):
        assert sorted({int(c) for v in t.values() for c in v["hist"]}) == list(gen.ALL_CODES)
