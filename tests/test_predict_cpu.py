"""No-GPU checks of `Model.predict`'s host side: the letterbox geometry against hand-worked cases, the proof that the
comparison of tests/test_gpu_predict.py's inverse map is sharp (every mutant of tests/predict_ref.py changes the fixed case
list), the record guards of the C ABI that need no device, and the result formatter of scripts/predict.py."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import predict_ref as pr
from src.data.letterbox import FILL, letterbox_geometry, letterbox_records

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32

# (H, W, scaleup) -> (nw, nh, left, top, W / nw, H / nh) on S = 96, worked by hand:
#   37 x 41: r = 96 / 41, 37 r = 86.63 -> 87 rows, top = 9 // 2 = 4      50 x 200: r = 0.48, 24 rows, top = 72 // 2 = 36
#   7 x 10:  r = 9.6, 67.2 -> 67 rows, top = 29 // 2 = 14                without scaleup r = 1: 10 x 7 at (43, 44)
HAND = [
    ((37, 41, True), (96, 87, 0, 4, 41 / 96, 37 / 87)),
    ((50, 200, True), (96, 24, 0, 36, 200 / 96, 50 / 24)),
    ((200, 50, True), (24, 96, 36, 0, 50 / 24, 200 / 96)),
    ((96, 96, True), (96, 96, 0, 0, 1.0, 1.0)),
    ((1, 1, True), (96, 96, 0, 0, 1 / 96, 1 / 96)),
    ((7, 10, True), (96, 67, 0, 14, 10 / 96, 7 / 67)),
    ((7, 10, False), (10, 7, 43, 44, 1.0, 1.0)),
]


@pytest.mark.parametrize("case,want", HAND)
def test_letterbox_geometry_hand_worked(case, want):
    h, w, scaleup = case
    nw, nh, left, top, sx, sy = letterbox_geometry(h, w, 96, scaleup)
    assert (nw, nh, left, top) == want[:4]
    assert sx == float(f32(want[4])) and sy == float(f32(want[5]))            # the double quotient, rounded once
    assert (nw, nh, left, top, sx, sy) == pr.geometry(h, w, 96, scaleup)
    assert 0 <= left and 0 <= top and left + nw <= 96 and top + nh <= 96 and nw >= 1 and nh >= 1
    if scaleup:
        assert nw == 96 or nh == 96


def test_letterbox_geometry_inside_the_canvas_everywhere():
    assert FILL == 114
    assert letterbox_geometry(640, 640, 640) == (640, 640, 0, 0, 1.0, 1.0)
    rng = np.random.default_rng(5)
    for s in (20, 33, 96, 640):
        for h, w in rng.integers(1, 3000, (200, 2)):
            for scaleup in (True, False):
                nw, nh, left, top, sx, sy = letterbox_geometry(int(h), int(w), s, scaleup)
                assert 1 <= nw <= s and 1 <= nh <= s and 0 <= left and 0 <= top and left + nw <= s and top + nh <= s
                assert sx == float(f32(int(w) / nw)) and sy == float(f32(int(h) / nh))
                if scaleup or max(h, w) >= s:
                    assert nw == s or nh == s
    with pytest.raises(ValueError):
        letterbox_geometry(0, 5, 96)


def test_letterbox_records_pack_back_to_back_and_pad_with_blank_slots():
    recs, used = letterbox_records([(37, 41), (7, 10)], 96, True, slots=4)
    assert used == 3 * (37 * 41 + 7 * 10) and len(recs) == 4
    assert recs[0][:3] == (0, 37, 41) and recs[1][:3] == (3 * 37 * 41, 7, 10)
    assert recs[2] == recs[3] == (0, 0, 0, 0, 0, 0, 0, 1.0, 1.0)


def test_rows_to_source_ref_hand_worked():
    """one row on the 200 x 50 picture (24 columns at left = 36, scales 50 / 24 and 200 / 96): a box from the left bar to beyond
    the right edge of the canvas"""
    rec = (0, 200, 50) + pr.geometry(200, 50, 96)
    rows = np.array([[[30.0, 12.0, 100.0, 48.0, 0.0, 7.0], [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]]], f32)
    out = pr.rows_to_source_ref(rows, [1], [rec], True)
    sx, sy = f32(50 / 24), f32(200 / 96)
    assert out[0, 0].tolist() == [0.0, float(f32(12) * sy), 50.0, float(f32(48) * sy), 0.5, 7.0]
    assert float(f32(64 - 36) * sx) > 50.0                                    # (the clip at W did the work above)
    assert out[0, 1].tolist() == rows[0, 1].tolist()                          # past the count: untouched
    assert pr.rows_to_source_ref(rows, [1], [rec], False)[0, 0, 4] == 0.0


@pytest.mark.parametrize("prob", [False, True])
def test_every_mutant_changes_the_fixed_cases(prob):
    recs, rows, counts = pr.cases()
    assert counts.min() == 0 and counts.max() == rows.shape[1] == pr.MAX_DET
    good = pr.rows_to_source_ref(rows, counts, recs, prob)
    assert good.dtype == np.float32
    for n, c in enumerate(counts):
        assert np.array_equal(good[n, c:], rows[n, c:]) and np.array_equal(good[n, :, 5], rows[n, :, 5])
        h, w = recs[n][1:3]
        assert (good[n, :c, [0, 2]] >= 0).all() and (good[n, :c, [0, 2]] <= w).all()
        assert (good[n, :c, [1, 3]] >= 0).all() and (good[n, :c, [1, 3]] <= h).all()
        assert (np.diff(good[n, :c, 4]) <= 0).all()
    inside = (good[..., :4] > 0).all(-1) & (good[..., 2] < np.array([r[2] for r in recs])[:, None])
    assert inside.any(), "the cases need boxes that no clip touches"
    if prob:
        live = np.arange(pr.MAX_DET)[None, :] < counts[:, None]
        assert (np.abs(good[..., 4] - pr.sigmoid64(rows[..., 4]))[live] <= pr.SIGMOID_BOUND).all()
    for mut in pr.MUTANTS:
        bad = pr.rows_to_source_ref(rows, counts, recs, prob, mut=mut)
        assert not np.array_equal(bad.view(np.uint32), good.view(np.uint32)), f"mutant {mut} is invisible on the fixed cases"


def test_letter_fill_guards_without_a_device():
    """yolo_letter_fill is host code: each refusal of the record contract answers YOLO_ERR_ARG, a good record and a blank slot 0"""
    from src.hipops import lib
    n = lib.query("yolo_letter_bytes")
    assert n == 40
    buf = ctypes.create_string_buffer(2 * n)
    ptr = ctypes.addressof(buf)
    assert pr.letter_fill(lib, ptr) == 0 and pr.letter_fill(lib, ptr, index=1, **pr.LETTER_BLANK) == 0
    rec = np.frombuffer(buf.raw[:n], np.int32)
    assert rec[:8].tolist() == [0, 0, 50, 200, 96, 24, 0, 36] and np.frombuffer(buf.raw[32:40], f32).tolist() == [f32(200 / 96), f32(50 / 24)]
    for bad in pr.LETTER_REFUSED + [dict(index=-1)]:
        assert pr.letter_fill(lib, ptr, **bad) == pr.YOLO_ERR_ARG, bad


def _script():
    path = os.path.join(ROOT, "custom-yolo-implmentation_amd", "scripts", "predict.py")
    spec = importlib.util.spec_from_file_location("predict_script", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_formats_coco_result_records(tmp_path):
    mod = _script()
    rows = [[10.126, 20.5, 110.126, 60.25, 0.912345678, 17.0], [0.0, 0.0, 4.0, 3.0, 0.25, 0.0]]
    assert mod.coco_records("a.jpg", rows) == [
        {"file": "a.jpg", "category_id": 17, "bbox": [10.13, 20.5, 100.0, 39.75], "score": 0.91235},
        {"file": "a.jpg", "category_id": 0, "bbox": [0.0, 0.0, 4.0, 3.0], "score": 0.25},
    ]
    assert mod.coco_records("b.png", []) == []
    for name in ("b.PNG", "a.jpg", "notes.txt"):
        (tmp_path / name).write_bytes(b"")
    assert [os.path.basename(p) for p in mod.list_sources(str(tmp_path))] == ["a.jpg", "b.PNG"]
    assert mod.list_sources(str(tmp_path / "a.jpg")) == [str(tmp_path / "a.jpg")]
    with pytest.raises(SystemExit):
        mod.list_sources(str(tmp_path / "missing"))
