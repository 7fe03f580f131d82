"""No GPU: the proof of tests/ap_ref.py, the numpy float64 restatement of COCOeval's rules that the device kernels
(yolo_ap_match, yolo_ap_curve: tests/test_gpu_val_ap.py) are held to.  Hand-worked answers first; then mutants of the
restatement, one per rule that is easy to get wrong, each of which must change the result of at least one case."""
import numpy as np
import pytest

import ap_ref as ar

T10 = ar.IOU_THRS
FAR = (500.0, 500.0, 510.0, 510.0)         # a box that overlaps nothing
ONE = 1.0 / (0.0 + 1.0 + np.spacing(1))    # the precision of a lone TP: 1 - 2^-52, COCOeval's "1"


def gt_box(x1, y1, x2, y2, cls):
    return [(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, cls]


def image(rows, gts, K=None):
    """rows: [(x1, y1, x2, y2, score, cls)] in descending score -> (det [1][K][6], count [1], [gt [m][5]])"""
    K = K or max(len(rows), 1)
    det = np.zeros((1, K, 6), dtype=np.float32)
    if rows:
        det[0, :len(rows)] = np.asarray(rows, dtype=np.float32)
    return det, np.array([len(rows)], dtype=np.int32), [np.asarray(gts, dtype=np.float32).reshape(-1, 5)]


def flags_case(flags, n_gt, cls=0):
    """rows that are TP / FP by construction: ground truth g is the 10 x 10 box at x = 100 g; a TP row is that box, an FP
    row is FAR.  Scores descend."""
    gts = [gt_box(100 * g, 0, 100 * g + 10, 10, cls) for g in range(n_gt)]
    rows, g = [], 0
    for i, f in enumerate(flags):
        if f:
            rows.append((100 * g, 0, 100 * g + 10, 10, 10.0 - i, cls))
            g += 1
        else:
            rows.append(FAR + (10.0 - i, cls))
    return image(rows, gts)


# ------------------------------------------------------------------------------------------------ known answers
def test_one_ground_truth_one_matching_row_gives_ap_one():
    table, s, status = ar.evaluate([flags_case([1], 1)], nc=1)
    assert status == 0 and table.shape == (1, 10, 101) and (table == ONE).all()
    assert ONE == 1.0 - 2.0 ** -52
    assert s["mAP50"] == pytest.approx(1.0, rel=1e-15) and s["mAP50-95"] == pytest.approx(1.0, rel=1e-15)
    assert s["ap_per_class"].tolist() == [s["mAP50-95"]]


def test_tp_fp_tp_with_two_ground_truths():
    table, s, _ = ar.evaluate([flags_case([1, 0, 1], 2)], nc=1)
    for t in range(10):
        q = table[0, t]
        assert (q[:51] == ONE).all() and (q[51:] == 2.0 / (1.0 + 2.0 + np.spacing(1))).all()
    assert s["mAP50"] == pytest.approx((51 + 100 / 3) / 101, rel=1e-15)
    assert s["mAP50-95"] == pytest.approx((51 + 100 / 3) / 101, rel=1e-15)


def test_class_with_ground_truth_and_no_rows_gives_zero_and_a_class_without_is_excluded():
    det, count, gts = flags_case([1], 1, cls=0)
    gts[0] = np.concatenate([gts[0], np.asarray([gt_box(300, 300, 320, 320, 1)], dtype=np.float32)])
    table, s, _ = ar.evaluate([(det, count, gts)], nc=3)
    assert (table[0] == ONE).all() and (table[1] == 0.0).all() and (table[2] == -1.0).all()
    assert s["ap_per_class"][1:].tolist() == [0.0, -1.0] and s["ap_per_class"][0] == pytest.approx(1.0, rel=1e-15)
    assert s["mAP50"] == pytest.approx(0.5, rel=1e-15) and s["mAP50-95"] == pytest.approx(0.5, rel=1e-15)     # classes 0 and 1 only
    table, s, _ = ar.evaluate([image([FAR + (1.0, 0)], [])], nc=2)      # no class has ground truth: all zeros
    assert (table == -1.0).all() and s["mAP50"] == 0.0 and s["mAP50-95"] == 0.0


def test_three_ground_truths_each_tp_jumps_a_third_of_the_recall_thresholds():
    table, _, _ = ar.evaluate([flags_case([1, 0, 1, 0, 1], 3)], nc=1)
    eps = np.spacing(1)
    p1, p2, p3 = 1.0 / (0.0 + 1.0 + eps), 2.0 / (1.0 + 2.0 + eps), 3.0 / (2.0 + 3.0 + eps)
    q = table[0, 0]
    assert (q[:34] == p1).all() and (q[34:67] == p2).all() and (q[67:] == p3).all()      # 34 + 33 + 34 thresholds
    table, _, _ = ar.evaluate([flags_case([1, 0, 1], 3)], nc=1)         # recall stops at 2/3: the last 34 stay 0
    assert (table[0, 0][67:] == 0.0).all() and (table[0, 0][34:67] == p2).all()


def test_iou_exactly_on_a_threshold_matches_and_thresholds_are_independent():
    # [0,0,4,4] against [0,0,4,3]: 12 / 16 = 0.75 exactly; [0,0,10,10] against [0,0,10,5]: 50 / 100 = 0.5 exactly
    det, count, gts = image([(0, 0, 4, 4, 2.0, 0), (100, 0, 110, 10, 1.0, 0)], [gt_box(0, 0, 4, 3, 0), gt_box(100, 0, 110, 5, 0)])
    assert ar.iou_matrix(det[0, :, :4], gts[0][:, :4])[[0, 1], [0, 1]].tolist() == [0.75, 0.5]
    key, tp, gt_count, _ = ar.match_batch(det, count, gts, T10, 1)
    assert tp[0].tolist() == [0b111111, 0b1] and gt_count.tolist() == [2]      # 0.5 .. 0.75 and 0.5 alone
    assert (key[0] >> 32).tolist() == [0, 0] and key[0, 0] < key[0, 1]          # higher score sorts first


def test_key_orders_class_then_score_and_marks_ignored_rows():
    rows = [(0, 0, 1, 1, 3.5, 1), (0, 0, 1, 1, 0.0, 0), (0, 0, 1, 1, -0.0, 0), (0, 0, 1, 1, -2.0, 0), (0, 0, 1, 1, -2.5, 2),
            (0, 0, 1, 1, -3.0, -1)]
    det, count, gts = image(rows, [], K=8)
    key, tp, _, _ = ar.match_batch(det, count, gts, T10, 2)
    assert key[0, 1] < key[0, 2] < key[0, 3] < key[0, 0]                # class 0 by descending score (+0 before -0), then class 1
    assert (key[0, 4:] == 2 << 32).all() and (tp == 0).all()            # class nc, class -1, rows past the count
    assert ar.score_ord(np.float32([-np.inf, -1, -0.0, 0.0, 1, np.inf])).tolist() == sorted(
        ar.score_ord(np.float32([-np.inf, -1, -0.0, 0.0, 1, np.inf])).tolist())


def test_zero_area_pair_never_matches():
    det, count, gts = image([(5, 5, 5, 5, 1.0, 0)], [[5, 5, 0, 0, 0]])
    assert np.isnan(ar.iou_matrix(det[0, :, :4], gts[0][:, :4])[0, 0])
    _, tp, gt_count, _ = ar.match_batch(det, count, gts, T10, 1)
    assert tp.tolist() == [[0]] and gt_count.tolist() == [1]
    assert ar.match_image_scan(det[0], 1, gts[0], T10, 1).tolist() == [0]


def test_more_than_1024_ground_truths_set_status_and_contribute_nothing():
    det, count, gts = ar.seeded_batch(3, 8, [1025, 2], 4)
    key, tp, gt_count, status = ar.match_batch(det, count, gts, T10, 4)
    k1, t1, g1, s1 = ar.match_batch(det[1:], count[1:], gts[1:], T10, 4)
    assert status == 1 and s1 == 0 and (key[0] == 4 << 32).all() and (tp[0] == 0).all()
    assert np.array_equal(key[1:], k1) and np.array_equal(tp[1:], t1) and np.array_equal(gt_count, g1)


@pytest.mark.parametrize("seed", range(6))
def test_vectorised_matching_equals_the_literal_scan(seed):
    det, count, gts = ar.seeded_batch(seed, 24, [0, 1, 7, 40], 5)
    _, tp, _, _ = ar.match_batch(det, count, gts, T10, 5)
    for b in range(4):
        assert np.array_equal(tp[b], ar.match_image_scan(det[b], count[b], gts[b], T10, 5)), b
    assert tp.any()


# ------------------------------------------------------------------------------------------------ mutants
def _cases():
    c = {}
    # A ties between two different ground truths (IoU 0.5 with each half of it), B is the upper half itself: with the
    # highest index A takes the lower half [0,5,10,10] and B is left with nothing
    c["tie"] = ([image([(0, 0, 10, 10, 2.0, 0), (0, 5, 10, 10, 1.0, 0)], [gt_box(0, 0, 10, 5, 0), gt_box(0, 5, 10, 10, 0)])], 1)
    # IoU exactly 0.5
    c["on_threshold"] = ([image([(0, 0, 10, 10, 1.0, 0)], [gt_box(0, 0, 10, 5, 0)])], 1)
    # A (IoU 0.6 = 6 / 10) takes the ground truth at the low thresholds, B (the box itself) at the high ones
    c["per_threshold"] = ([image([(0, 0, 10, 6, 2.0, 0), (0, 0, 10, 10, 1.0, 0)], [gt_box(0, 0, 10, 10, 0)])], 1)
    # equal scores across two images: the TP was inserted first
    a, b = flags_case([1], 1), image([FAR + (10.0, 0)], [])
    c["equal_scores"] = ([a, b], 1)
    # [FP, TP, TP]: the precision rises towards the end, so the envelope lifts the early entries
    c["rising"] = ([flags_case([0, 1, 1], 2)], 1)
    # recall reaches exactly 1.0 = the last recall threshold
    c["full_recall"] = ([flags_case([1], 1)], 1)
    # an image without ground truth whose row outscores the TP of another image
    c["empty_image"] = ([image([FAR + (20.0, 0)], []), flags_case([1], 1)], 1)
    return c


MUTANTS = {"lowest index on an IoU tie": dict(tie_highest=False), "> instead of >= at the threshold": dict(strict=True),
           "one taken set for all thresholds": dict(shared_taken=True), "unstable sort": dict(stable=False),
           "no envelope": dict(envelope=False), "searchsorted side right": dict(side="right"),
           "images without ground truth skipped": dict(skip_empty=True)}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_every_mutant_changes_a_case(name):
    changed = []
    for tag, (batches, nc) in _cases().items():
        want = ar.evaluate(batches, nc)[0]
        got = ar.evaluate(batches, nc, **MUTANTS[name])[0]
        if not np.array_equal(want, got):
            changed.append(tag)
    assert changed, f"mutant `{name}` passes every case"
    print(f"\n[ap_ref] mutant `{name}` changes: {changed}")


def test_the_cases_have_the_answers_worked_by_hand():
    c = _cases()
    ev = lambda tag, **kw: ar.evaluate(*c[tag], **kw)
    _, tp, _, _ = ar.match_batch(*c["tie"][0][0], T10, 1)
    assert tp[0].tolist() == [0b1, 0b1111111110]                        # A at 0.5 only; B finds its own box taken there ...
    assert ev("tie")[0][0, 0].tolist() == [ONE] * 51 + [0.0] * 50       # ... so recall stops at 1/2 at threshold 0.5
    half = 1.0 / (1.0 + 1.0 + np.spacing(1))                            # from 0.55 on the rows are [FP, TP]
    assert all(ev("tie")[0][0, t].tolist() == [half] * 51 + [0.0] * 50 for t in range(1, 10))
    _, tp, _, _ = ar.match_batch(*c["per_threshold"][0][0], T10, 1)
    assert tp[0].tolist() == [0b111, 0b1111111000]                      # A at 0.5, 0.55, 0.6; B from 0.65 on
    assert ev("equal_scores")[1]["mAP50"] == pytest.approx(1.0, rel=1e-15) and ev("equal_scores", stable=False)[1]["mAP50"] < 0.51
    assert ev("rising")[0][0, 0].tolist() == [2.0 / (1.0 + 2.0 + np.spacing(1))] * 101
    assert ev("empty_image")[1]["mAP50"] == 1.0 / (1.0 + 1.0 + np.spacing(1))
    assert ev("empty_image", skip_empty=True)[1]["mAP50"] == pytest.approx(1.0, rel=1e-15)
