"""-m gpu: COCO average precision on the device.  yolo_ap_match and yolo_ap_curve are held BIT FOR BIT to
tests/ap_ref.py, the numpy float64 restatement of COCOeval's rules that tests/test_ap_ref_cpu.py proves: every compared
quantity is an integer (keys, bit sets, counts, status) or a double formed in one fixed operation order (the table), so no
tolerance applies anywhere.  Then DetectionAP over three batches against the same restatement, and train()'s validation
epoch with and without `val_ap`."""
import numpy as np
import pytest
import torch

import ap_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda"
T10 = ar.IOU_THRS


def gt_box(x1, y1, x2, y2, cls):
    return [(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, cls]


def run_match(det, count, gts, thrs, nc):
    from src.hipops import ops
    sizes = [len(g) for g in gts]
    gt = np.concatenate([np.asarray(g, dtype=np.float32).reshape(-1, 5) for g in gts] + [np.zeros((1, 5), dtype=np.float32)])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    gt_count = torch.zeros(nc, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    key, tp = ops.ap_match(torch.from_numpy(np.ascontiguousarray(det, dtype=np.float32)).to(DEV),
                           torch.from_numpy(np.asarray(count, dtype=np.int32)).to(DEV), torch.from_numpy(gt).to(DEV),
                           torch.from_numpy(off).to(DEV), torch.from_numpy(np.asarray(thrs, dtype=np.float64)).to(DEV), nc,
                           gt_count, status)
    torch.cuda.synchronize()
    return key.cpu().numpy(), tp.cpu().numpy().view(np.uint32), gt_count.cpu().numpy(), int(status.cpu()[0])


def check_match(det, count, gts, thrs, nc):
    want = ar.match_batch(det, count, gts, thrs, nc)
    got = run_match(det, count, gts, thrs, nc)
    for name, w, g in zip(("key", "tp", "gt_count"), want, got):
        assert w.dtype == g.dtype and np.array_equal(w, g), (name, np.argwhere(w != g)[:5].tolist())
    assert want[3] == got[3], ("status", want[3], got[3])
    return want


def test_ap_match_hand_cases():
    """N = 4, K = 8: an IoU tie between two different ground truths (the highest index wins, so row 1 loses its own box at
    0.5), IoU exactly 0.5 and exactly 0.75, duplicated ground truths, two rows competing for one ground truth, a row whose
    partner differs between thresholds, rows of class nc and -1, a count of 0, ground-truth classes outside the range, a
    zero-area pair (NaN), an image without ground truth."""
    nc = 3
    det = np.zeros((4, 8, 6), dtype=np.float32)
    det[0, :7] = [(0, 0, 10, 10, 5.0, 0), (0, 5, 10, 10, 4.5, 0),         # the tie, then the upper half itself
                  (100, 0, 104, 4, 4.0, 1),                               # IoU 0.75 with [100,0,104,3]
                  (200, 0, 210, 10, 3.0, 2), (200, 0, 210, 10, 3.0, 2), (200, 0, 210, 10, 2.0, 2),    # three rows, two duplicated GT
                  (0, 0, 10, 10, 1.0, 3)]                                 # class nc
    g0 = [gt_box(0, 0, 10, 5, 0), gt_box(0, 5, 10, 10, 0), gt_box(100, 0, 104, 3, 1), gt_box(200, 0, 210, 10, 2),
          gt_box(200, 0, 210, 10, 2), gt_box(0, 0, 10, 10, 3), gt_box(0, 0, 10, 10, -1)]
    # image 1: A = the left 7 columns of G0 (IoU 0.7; 0.3 with G1) before B = its right 9 columns (IoU 0.9; 60 / 90 with G1 =
    # its right 6 columns): A holds G0 up to 0.7, so B's partner is G1 up to 0.65, nobody at 0.7, G0 from 0.75 to 0.9
    det[1, :3] = [(0, 0, 7, 10, 3.0, 0), (1, 0, 10, 10, 2.0, 0), (5, 5, 5, 5, 1.0, 1)]
    g1 = [gt_box(0, 0, 10, 10, 0), gt_box(4, 0, 10, 10, 0), [5, 5, 0, 0, 1]]
    det[2, :4] = [(0, 0, 10, 10, 1.0, 0)] * 4                             # count 0: rows ignored, ground truths counted
    g2 = [gt_box(0, 0, 10, 10, 0), gt_box(0, 0, 10, 10, 2)]
    det[3, :5] = [(0, 0, 10, 10, 2.0, 0), (0, 0, 10, 10, 2.0, 1), (0, 0, 10, 10, -0.0, 1), (0, 0, 10, 10, 0.0, 1), (1, 1, 2, 2, -7.0, -1)]
    count = np.array([7, 3, 0, 5], dtype=np.int32)
    key, tp, gt_count, status = check_match(det, count, [g0, g1, g2, []], T10, nc)
    assert status == 0 and gt_count.tolist() == [5, 2, 3]
    assert tp[0, :7].tolist() == [0b1, 0b1111111110, 0b111111, 0x3FF, 0x3FF, 0, 0]
    assert tp[1, :3].tolist() == [0b11111, 0b111101111, 0] and (tp[2:] == 0).all()
    assert (key[2] == nc << 32).all() and (key[3, :4] >> 32).tolist() == [0, 1, 1, 1] and key[3, 4] == nc << 32


@pytest.mark.parametrize("K,gt_counts,thrs", [
    (8, [1], T10), (8, [0, 63], T10), (300, [64, 65, 1], T10), (300, [1024, 0, 65, 63], T10), (8, [1025, 1, 0, 64], T10),
    (300, [1025, 1024], T10), (300, [65, 7], [0.5]), (8, [63, 64, 65], [0.75, 0.5, 1.0])],
    ids=["1x8", "2x8", "3x300", "4x300-1024", "4x8-1025", "2x300-1025", "one-threshold", "three-unordered"])
def test_ap_match_equals_the_restatement_bit_for_bit(K, gt_counts, thrs):
    nc = 5
    det, count, gts = ar.seeded_batch(100 + K + len(gt_counts), K, gt_counts, nc)
    key, tp, gt_count, status = check_match(det, count, gts, thrs, nc)
    assert status == int(max(gt_counts) > 1024)
    if max(gt_counts) > 1 and status == 0:
        assert tp.any() and (key != nc << 32).any()


def test_ap_match_and_ap_curve_refuse_what_they_cannot_hold():
    from src.hipops import lib
    det, count, gts = ar.seeded_batch(1, 8, [2], 3)
    for thrs in ([], np.linspace(0.5, 0.95, 11)):
        with pytest.raises(RuntimeError, match="1001"):
            run_match(det, count, gts, thrs, 3)
    with pytest.raises(RuntimeError, match="1001"):          # D = 2^31 rows: refused before anything is launched or read
        lib.call("yolo_ap_curve", 0, 0, 1 << 31, 0, 0, 3, 10, 0, 0)


def curve_records(seed, nc, n_thr):
    """records with class segments of 0, 1, 255, 256, 257 and 1000 rows, all-TP, all-FP, dense and sparse bit sets, scores on
    a coarse lattice (equal scores from different 'images'), npig of 0, 1, 3 and 1000, some ignored rows, in random
    insertion order"""
    rng = np.random.default_rng(seed)
    lens, npigs = [0, 1, 255, 256, 257, 1000], [1, 3, 1000, 0]
    keys, tps = [], []
    gt_count = np.zeros(nc, dtype=np.int64)
    for c in range(nc):
        L = lens[(c + seed) % 6]
        gt_count[c] = npigs[(c + seed // 6) % 4] if nc > 1 else npigs[seed % 3]
        score = (np.round(rng.normal(0, 2, L) * 4) / 4).astype(np.float32)
        keys.append((np.int64(c) << 32) | (np.uint32(0xFFFFFFFF) - ar.score_ord(score)).astype(np.int64))
        kind = (c + seed) % 4
        full = np.uint32((1 << n_thr) - 1)
        bits = rng.integers(0, 1 << n_thr, L).astype(np.uint32)
        tps.append([np.full(L, full, dtype=np.uint32), np.zeros(L, dtype=np.uint32), bits,
                    np.where(rng.random(L) < 0.05, bits, 0).astype(np.uint32)][kind])
    keys.append(np.full(37, np.int64(nc) << 32))
    tps.append(np.zeros(37, dtype=np.uint32))
    key, tp = np.concatenate(keys), np.concatenate(tps)
    order = rng.permutation(key.size)
    return key[order], tp[order], gt_count


@pytest.mark.parametrize("nc,n_thr,seed", [(1, 1, 0), (1, 10, 1), (1, 1, 2), (1, 10, 3), (1, 10, 4), (1, 10, 5), (3, 10, 0),
                                           (3, 1, 3), (3, 10, 8), (80, 10, 0), (80, 1, 7), (80, 10, 13)])
def test_ap_curve_equals_the_restatement_bit_for_bit(nc, n_thr, seed):
    from src.hipops import ops
    key, tp, gt_count = curve_records(seed, nc, n_thr)
    want = ar.curve(key, tp, gt_count, nc, n_thr)
    skey, stp = ar.sort_records(key, tp)
    got = ops.ap_curve(torch.from_numpy(skey).to(DEV), torch.from_numpy(stp.view(np.int32)).to(DEV),
                       torch.from_numpy(gt_count).to(DEV), torch.from_numpy(ar.REC_THRS).to(DEV), nc, n_thr)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    if nc == 80:
        assert (want == -1).any() and (want == 0).any() and (want > 0.5).any()


def test_ap_curve_without_any_row():
    from src.hipops import ops
    gt_count = np.array([0, 4], dtype=np.int64)
    got = ops.ap_curve(torch.empty(0, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV),
                       torch.from_numpy(gt_count).to(DEV), torch.from_numpy(ar.REC_THRS).to(DEV), 2, 10).cpu().numpy()
    assert (got[0] == -1).all() and (got[1] == 0).all()


def test_detection_ap_over_three_batches():
    """DetectionAP (update_batch x 3, compute: concatenate, stable sort, table, one copy) against the restatement: the table
    bit for bit, the means equal as Python floats; compute() twice gives the same; reset() starts over."""
    from src.training.metrics import DetectionAP
    nc = 80
    batches = [ar.seeded_batch(11, 300, [9, 0, 70, 3], nc), ar.seeded_batch(12, 8, [2, 5, 0], nc),
               ar.seeded_batch(13, 300, [130, 1], nc)]
    table, summary, status = ar.evaluate(batches, nc)
    assert status == 0
    ap = DetectionAP(nc)
    assert np.array_equal(ap.iou_thresholds, T10)
    for det, count, gts in batches:
        ap.update_batch(torch.from_numpy(det).to(DEV), torch.from_numpy(count).to(DEV), [torch.from_numpy(g) for g in gts])
    for _ in range(2):
        res = ap.compute()
        assert set(res) == {"mAP50", "mAP50-95", "ap_per_class", "precision"}
        assert np.array_equal(res["precision"], table), np.argwhere(res["precision"] != table)[:5].tolist()
        assert type(res["mAP50"]) is float and res["mAP50"] == summary["mAP50"] and res["mAP50-95"] == summary["mAP50-95"]
        assert np.array_equal(res["ap_per_class"], summary["ap_per_class"])
    assert 0.0 < res["mAP50-95"] < res["mAP50"] < 1.0 and (res["ap_per_class"][6:] == -1).all()
    ap.reset()
    res = ap.compute()
    assert res["mAP50"] == 0.0 and res["mAP50-95"] == 0.0 and (res["precision"] == -1).all() and (res["ap_per_class"] == -1).all()
    det, count, gts = ar.seeded_batch(14, 8, [1025, 3], nc)
    ap.update_batch(torch.from_numpy(det).to(DEV), torch.from_numpy(count).to(DEV), [torch.from_numpy(g) for g in gts])
    with pytest.raises(RuntimeError, match="1024 targets"):
        ap.compute()


TODAY = {"precision", "recall", "f1_score", "mAP", "true_positives", "false_positives", "false_negatives", "total_predictions",
         "total_ground_truths"}


def _train_one_epoch(tmp_path, monkeypatch, **kw):
    """train() on the smallest preset at 64 x 64: one training batch, two validation batches (one image without boxes)"""
    import strict_addressing as sa
    from oracle.blocks import PRESETS
    from src.model.losses import YoloDFLQFLoss
    from src.model.model_builder import Model
    from src.training import train_model as tm
    from src.training.utils_train import get_optimizer

    class Loader(list):
        sampler = None

    def batches(n, seed, counts):
        g = torch.Generator().manual_seed(seed)
        out = Loader()
        for _ in range(n):
            img = torch.randn(len(counts), 3, 64, 64, generator=g)
            tg = [{"boxes": torch.cat([torch.rand(c, 2, generator=g) * 48 + 8, torch.rand(c, 2, generator=g) * 24 + 4,
                                       torch.randint(0, 80, (c, 1), generator=g).float()], 1)} for c in counts]
            out.append((img, tg))
        return out
    torch.manual_seed(0)
    model = Model(**PRESETS["n"], num_classes=80).to(DEV)
    opt, sched = get_optimizer(model, lr=1e-4, weight_decay=1e-4, patience=3, factor=0.5)
    seen = sa.install_checker(monkeypatch)
    md = tm.train(model=model, train_loader=batches(1, 3, [2, 3]), val_loader=batches(2, 4, [3, 0]), optimizer=opt,
                  scheduler=sched, criterion=YoloDFLQFLoss(num_classes=80), initial_epoch=0, num_epochs=1, device=0,
                  num_classes=80, rank=0, checkpoint_dir=str(tmp_path), distributed_mode="ddp", precision="float32",
                  conf_threshold=0.01, captured_step=False, **kw)
    return md, seen


def test_train_validation_epoch_with_val_ap(tmp_path, monkeypatch, capsys):
    md, seen = _train_one_epoch(tmp_path, monkeypatch, val_ap={"conf": 0.001, "nms_iou": 0.7, "max_det": 300})
    assert set(md) == TODAY | {"mAP50", "mAP50-95"}
    for k in ("mAP50", "mAP50-95"):
        assert type(md[k]) is float and np.isfinite(md[k]) and 0.0 <= md[k] <= 1.0, (k, md[k])
    assert seen.count("yolo_ap_match") == 2 and seen.count("yolo_nms") == 2 and seen.count("yolo_ap_curve") == 1
    assert seen.count("yolo_head_decode") == 2                         # the decoded tensor is shared with the counters
    out = capsys.readouterr().out
    assert "COCO AP - mAP50: " in out and "mAP50-95: " in out


def test_train_without_val_ap_is_todays(tmp_path, monkeypatch, capsys):
    md, seen = _train_one_epoch(tmp_path, monkeypatch)
    assert set(md) == TODAY
    assert not any(n in seen for n in ("yolo_ap_match", "yolo_ap_curve", "yolo_nms")) and seen.count("yolo_head_decode") == 2
    assert "mAP50" not in capsys.readouterr().out
    from src.training.train_model import val_ap_settings
    assert val_ap_settings(None) is None and val_ap_settings({}) == {"conf": 0.001, "nms_iou": 0.7, "max_det": 300}
    for bad in ({"iou": 0.5}, {"conf": 0.0}, {"max_det": 0}, [0.001]):
        with pytest.raises(ValueError, match="val_ap"):
            val_ap_settings(bad)
