"""Mosaic augmentation on the CPU: the host logic of BatchTransform's mosaic (draw order, records, box rule, validation,
per-epoch switch) with the two device leaves swapped for CPU stand-ins -- `image_prep` for the oracle (emulated_ops) and
`image_prep_mosaic` for tests/mosaic_ref.py -- and the C ABI of the new entry points (host-side calls only)."""
import os

import numpy as np
import pytest
import torch

import emulated_ops
import mosaic_ref
from oracle import image_prep as oip
from src.hipops import ops as real_ops

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(autouse=True)
def _emulate(monkeypatch):
    emulated_ops.install(monkeypatch)
    monkeypatch.setattr(real_ops, "image_prep_mosaic", mosaic_ref.image_prep_mosaic, raising=False)


@pytest.fixture
def calls(monkeypatch):
    """Which of the two leaves a transform call went through."""
    seen = []
    for name in ("image_prep", "image_prep_mosaic"):
        inner = getattr(real_ops, name)
        monkeypatch.setattr(real_ops, name, lambda *a, _n=name, _f=inner: (seen.append(_n), _f(*a))[1])
    return seen


def _inputs():
    """The inputs of test_batch_transform_host_logic_and_box_geometry."""
    rng = np.random.default_rng(3)
    imgs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)) for h, w in ((40, 60), (33, 20), (64, 64))]
    tg = [{"boxes": torch.tensor([[10., 5., 20., 10.]]), "labels": torch.tensor([[3.]]), "name": "a"},
          {"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, 1), "name": "b"},
          {"boxes": torch.tensor([[0., 0., 64., 64.], [16., 8., 8., 4.]]), "labels": torch.tensor([[1.], [2.]]), "name": "c"}]
    return imgs, tg


def _by_hand_sample():
    flip = bool(torch.rand(1) < 0.5)
    order = tuple(int(i) for i in torch.randperm(4))
    return flip, order, tuple(float(torch.empty(1).uniform_(a, b)) for a, b in ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.1, 0.1)))


def test_c1_draws_follow_the_stated_order_and_leave_sample_alone(calls):
    from src.data.transforms import BatchTransform, mosaic_geometry
    imgs, tg = _inputs()
    n, S = len(imgs), 32
    tr = BatchTransform(True, size=S, device="cpu", mosaic={"p": 0.6, "gain": [0.5, 1.5]})
    torch.manual_seed(4)
    params = [tr.sample() for _ in range(n)]
    draws = tr.sample_mosaic(n)
    after = float(torch.rand(1))
    torch.manual_seed(4)
    want_p = [_by_hand_sample() for _ in range(n)]
    want_d = []
    for _ in range(n):
        if not bool(torch.rand(1) < 0.6):
            want_d.append(None)
            continue
        partners = tuple(int(v) for v in torch.randint(0, n, (3,)))
        cx = int(torch.randint(S // 4, S - S // 4 + 1, (1,)))
        cy = int(torch.randint(S // 4, S - S // 4 + 1, (1,)))
        gains = tuple(float(torch.empty(1).uniform_(0.5, 1.5)) for _ in range(4))
        flips = tuple(bool(torch.rand(1) < 0.5) for _ in range(3))
        want_d.append((cx, cy, partners, gains, flips))
    assert params == want_p and draws == want_d and after == float(torch.rand(1))
    assert any(d is None for d in draws) and any(d is not None for d in draws)      # the seed exercises both branches
    for d in draws:
        if d is not None:
            assert S // 4 <= d[0] <= S - S // 4 and S // 4 <= d[1] <= S - S // 4 and all(0.5 <= g <= 1.5 for g in d[3])
    # the geometry of a draw: tile sizes by the rounding rule, every tile with one corner on the centre, tile 0 = the image itself
    sizes = [tuple(t.shape[:2]) for t in imgs]
    i = next(j for j, d in enumerate(draws) if d is not None)
    cx, cy, partners, gains, flips = draws[i]
    rec = mosaic_geometry(draws[i], i, sizes, params[i][0], S)
    assert (rec["cx"], rec["cy"]) == (cx, cy) and [t[0] for t in rec["tiles"]] == [i, *partners]
    assert [t[1] for t in rec["tiles"]] == [params[i][0], *flips]
    for k, (src, _, tw, th, x0, y0) in enumerate(rec["tiles"]):
        h, w = sizes[src]
        assert tw == max(1, round(gains[k] * (S / max(h, w)) * w)) and th == max(1, round(gains[k] * (S / max(h, w)) * h))
        assert (x0 if k & 1 else x0 + tw) == cx and (y0 if k & 2 else y0 + th) == cy

    # a whole call draws sample() x n, then sample_mosaic(n): the same batch from the seed as from the explicit decisions
    torch.manual_seed(4)
    got, got_t = tr(imgs, tg)
    want, want_t = tr(imgs, tg, params=params, mosaic=draws)
    assert torch.equal(got, want) and all(torch.equal(a["boxes"], b["boxes"]) for a, b in zip(got_t, want_t))
    assert calls == ["image_prep_mosaic", "image_prep_mosaic"]

    # mosaic switched off: sample()'s sequence and the output are the plain transform's, and nothing else is drawn
    del calls[:]
    tr.mosaic_on = False
    torch.manual_seed(4)
    off, off_t = tr(imgs, tg)
    rng_after = float(torch.rand(1))
    torch.manual_seed(4)
    plain, plain_t = BatchTransform(True, size=S, device="cpu")(imgs, tg)
    assert rng_after == float(torch.rand(1)) and calls == ["image_prep", "image_prep"]
    assert torch.equal(off, plain) and all(torch.equal(a["boxes"], b["boxes"]) for a, b in zip(off_t, plain_t))

    # p = 0: every output is plain -- the draws say so and the batch is the plain transform's, boxes included
    tr0 = BatchTransform(True, size=S, device="cpu", mosaic={"p": 0.0})
    torch.manual_seed(4)
    assert tr0.sample_mosaic(5) == [None] * 5
    torch.manual_seed(4)
    zero, zero_t = tr0(imgs, tg)
    assert torch.equal(zero, plain) and all(torch.equal(a["boxes"], b["boxes"]) for a, b in zip(zero_t, plain_t))


def test_c2_without_mosaic_the_call_is_the_existing_path(calls):
    from src.data.transforms import BatchTransform, get_train_transforms
    imgs, tg = _inputs()
    tr = get_train_transforms(32, "cpu", mosaic=None)
    assert tr.mosaic is None and tr.mosaic_on is False
    torch.manual_seed(5)
    params = [tr.sample() for _ in imgs]
    torch.manual_seed(5)
    assert params == [_by_hand_sample() for _ in imgs]
    torch.manual_seed(5)
    batch, out = tr(imgs, tg)
    assert calls == ["image_prep"]
    assert batch.shape == (3, 3, 32, 32) and batch.dtype == torch.float32
    for i, (im, (flip, order, fac)) in enumerate(zip(imgs, params)):
        assert torch.equal(batch[i], oip.transform_image(im.numpy(), 32, flip, order, fac))
        h, w = im.shape[:2]
        ref = oip.transform_boxes(tg[i]["boxes"], w, h, 32, flip)
        assert torch.allclose(out[i]["boxes"][:, :4], ref) and torch.equal(out[i]["boxes"][:, 4:], tg[i]["labels"])
        assert out[i]["name"] == tg[i]["name"] and out[i]["boxes"].shape[1] == 5
    with pytest.raises(ValueError, match="without mosaic"):
        tr(imgs, tg, mosaic=[None] * 3)
    with pytest.raises(ValueError, match="without mosaic"):
        tr.sample_mosaic(3)
    # the reference of the CPU stand-in agrees with the oracle where both apply: a plain record is the plain transform
    for i, (im, (flip, order, fac)) in enumerate(zip(imgs, params)):
        got = mosaic_ref.mosaic_image([t.numpy() for t in imgs], mosaic_ref.plain_record(i, flip, 32), 32, 114, order, fac)
        assert torch.equal(got, oip.transform_image(im.numpy(), 32, flip, order, fac))


def _box_case():
    """Four 32 x 32 sources on a 32 canvas, centre (16, 16).  Tiles 0, 1, 3 are 16 x 16 (scale 0.5); tile 2 is 32 x 32 (scale 1)
    at (-16, 16): its quadrant shows source columns 16..31 and rows 0..15 only."""
    rng = np.random.default_rng(8)
    imgs = [torch.from_numpy(rng.integers(0, 256, (32, 32, 3)).astype(np.uint8)) for _ in range(4)]
    tg = [{"boxes": torch.tensor([[4., 4., 8., 8.]]), "labels": torch.tensor([[1.]]), "name": "i0", "image_id": torch.tensor([10])},
          {"boxes": torch.tensor([[0., 8., 8., 8.]]), "labels": torch.tensor([[2.]]), "name": "i1", "image_id": torch.tensor([11])},
          {"boxes": torch.tensor([[12., 2., 12., 8.],      # cut by the quadrant edge: x -4..8 -> 0..8, 2/3 visible
                                  [10., 2., 7., 8.],       # x -6..1 -> 0..1: narrower than min_box
                                  [0., 12., 18., 20.]]),   # x -16..2 -> 0..2, y 28..48 -> 28..32: 8 of 360 visible
           "labels": torch.tensor([[3.], [4.], [5.]]), "name": "i2", "image_id": torch.tensor([12])},
          {"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, 1), "name": "i3", "image_id": torch.tensor([13])}]
    records = [{"cx": 16, "cy": 16, "tiles": [(0, False, 16, 16, 0, 0), (1, True, 16, 16, 16, 0), (2, False, 32, 32, -16, 16),
                                              (0, False, 16, 16, 16, 16)]},       # tile 3: the partner is the image itself
               None,
               None,
               {"cx": 16, "cy": 16, "tiles": [(3, False, 16, 16, 0, 0), (3, True, 16, 16, 16, 0), (3, False, 16, 16, 0, 16),
                                              (3, False, 16, 16, 16, 16)]}]
    return imgs, tg, records


def test_c3_box_rule_by_hand():
    from src.data.transforms import BatchTransform
    imgs, tg, records = _box_case()
    sizes = [(32, 32)] * 4
    params = [(False, (), (1.0, 1.0, 1.0, 0.0)), (True, (), (1.0, 1.0, 1.0, 0.0)), (False, (), (1.0, 1.0, 1.0, 0.0)),
              (False, (), (1.0, 1.0, 1.0, 0.0))]
    tr = BatchTransform(True, size=32, device="cpu", mosaic={})
    batch, out = tr(imgs, tg, params=params, mosaic=records)
    assert batch.shape == (4, 3, 32, 32)
    want0 = torch.tensor([[2., 2., 4., 4., 1.],            # tile 0: fully inside, halved
                          [28., 4., 4., 4., 2.],           # tile 1, flipped: x = 32 - 0 - 8 = 24 -> 12 -> + 16
                          [0., 18., 8., 8., 3.],           # tile 2: cut by the quadrant edge; the two others are dropped
                          [18., 18., 4., 4., 1.]])         # tile 3: the image itself again
    assert torch.equal(out[0]["boxes"], want0) and out[0]["boxes"].dtype == torch.float32
    assert out[0]["name"] == "i0" and int(out[0]["image_id"]) == 10 and "labels" not in out[0]
    assert out[3]["boxes"].shape == (0, 5) and out[3]["name"] == "i3"               # empty targets all round
    # plain outputs inside the mosaic batch: today's box path (output 1 is flipped: x = 32 - 0 - 8)
    assert torch.equal(out[1]["boxes"], torch.tensor([[24., 8., 8., 8., 2.]]))
    assert torch.equal(out[2]["boxes"][:, :4], tg[2]["boxes"]) and torch.equal(out[2]["boxes"][:, 4:], tg[2]["labels"])
    # each dropped box falls to the rule it is meant to meet
    loose = BatchTransform(True, size=32, device="cpu", mosaic={"min_box": 1.0})(imgs, tg, params=params, mosaic=records)[1][0]["boxes"]
    assert [float(v) for v in loose[:, 4]] == [1., 2., 3., 4., 1.] and torch.equal(loose[3], torch.tensor([0., 18., 1., 8., 4.]))
    seen = BatchTransform(True, size=32, device="cpu", mosaic={"min_visible": 0.02})(imgs, tg, params=params, mosaic=records)[1][0]["boxes"]
    assert [float(v) for v in seen[:, 4]] == [1., 2., 3., 5., 1.] and torch.equal(seen[3], torch.tensor([0., 28., 2., 4., 5.]))
    # max_boxes: the largest clipped areas stay (ties: the earlier box), in their order
    two = BatchTransform(True, size=32, device="cpu", mosaic={"max_boxes": 2})(imgs, tg, params=params, mosaic=records)[1][0]["boxes"]
    assert torch.equal(two, want0[[0, 2]])
    # the restated rule gives the same
    for kw in ({}, {"min_box": 1.0}, {"min_visible": 0.02}, {"max_boxes": 2}):
        got = BatchTransform(True, size=32, device="cpu", mosaic=kw)(imgs, tg, params=params, mosaic=records)[1]
        for i in (0, 3):
            assert torch.equal(got[i]["boxes"], mosaic_ref.mosaic_boxes(records[i], tg, sizes, 32, **kw))
    # the image: quadrant by quadrant what the record says, fill where no tile reaches
    fill = mosaic_ref.fill_value()
    short = [{"cx": 16, "cy": 16, "tiles": [(0, False, 8, 8, 8, 8), (1, False, 16, 16, 16, 0), (2, False, 16, 16, 0, 16),
                                            (3, False, 16, 16, 16, 16)]}, None, None, None]
    img = tr(imgs, tg, params=params, mosaic=short)[0][0]
    assert torch.equal(img[:, :8, :16], fill.reshape(3, 1, 1).expand(3, 8, 16))
    assert torch.equal(img[:, 8:16, 8:16], oip.transform_image(imgs[0].numpy(), 8))
    assert torch.equal(img[:, 16:, 16:], oip.transform_image(imgs[3].numpy(), 16))


def test_c4_argument_validation_and_the_synthetic_path():
    from src.data.data_loader import get_data_loaders
    from src.data.transforms import BatchTransform, get_val_transforms
    for bad in ({"p": -0.1}, {"p": 1.5}, {"gain": [0.0, 1.0]}, {"gain": [1.0, 0.5]}, {"gain": [0.4, 2.5]}, {"gain": [0.4]},
                {"fill": 256}, {"max_boxes": 0}, {"close_epochs": -1}, {"scale": 2}):
        with pytest.raises(ValueError, match="mosaic"):
            BatchTransform(True, size=32, device="cpu", mosaic=bad)
    with pytest.raises(ValueError, match="training augmentation"):
        BatchTransform(False, size=32, device="cpu", mosaic={})
    assert get_val_transforms(32, "cpu").mosaic is None
    tr = BatchTransform(True, size=32, device="cpu", mosaic={})
    assert tr.mosaic == dict(p=1.0, gain=(0.4, 1.0), fill=114, min_box=2.0, min_visible=0.1, max_boxes=128, close_epochs=0)
    assert tr.mosaic_on is True
    assert BatchTransform(True, size=32, device="cpu", mosaic={"gain": [2.0, 2.0], "p": 0}).mosaic["gain"] == (2.0, 2.0)
    imgs, tg, records = _box_case()
    with pytest.raises(ValueError, match="records for 4 images"):
        tr(imgs, tg, mosaic=records[:2])
    with pytest.raises(ValueError, match="mosaic record 0"):
        tr(imgs, tg, mosaic=[{"cx": 16, "cy": 16, "tiles": [(0, False, 16, 16, 0, 0), (9, False, 16, 16, 16, 0),
                                                           (0, False, 16, 16, 0, 16), (0, False, 16, 16, 16, 16)]}, None, None, None])
    with pytest.raises(ValueError, match="decoded images"):
        get_data_loaders("/nonexistent/train", "/nonexistent/val", "", "", batch_size=2, is_test=True, device="cpu", res=32,
                         mosaic={"p": 1.0})
    tr_l, va_l = get_data_loaders("/nonexistent/train", "/nonexistent/val", "", "", batch_size=2, is_test=True, device="cpu", res=32)
    assert not hasattr(tr_l, "set_epoch")              # the synthetic path is as before


def test_c5_set_epoch_closes_the_mosaic_through_the_prefetcher(calls, tmp_path):
    import pandas as pd
    from PIL import Image
    from src.data.data_loader import DevicePrefetcher, DevicePreppedLoader, get_data_loaders
    rng = np.random.default_rng(4)
    rows = []
    os.makedirs(tmp_path / "img")
    for i, (h, w) in enumerate(((48, 64), (50, 40), (32, 32), (70, 90))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)).save(tmp_path / "img" / f"{i}.png")
        rows.append({"file_name": f"{i}.png", "bbox": [[1.0, 2.0, 10.0 + i, 12.0]] * (i + 1), "category_id": [float(i)] * (i + 1), "name": f"im{i}"})
    pd.DataFrame(rows).to_parquet(tmp_path / "train.parquet")
    pd.DataFrame(rows[:2]).to_parquet(tmp_path / "val.parquet")
    tr, va = get_data_loaders(str(tmp_path / "train.parquet"), str(tmp_path / "val.parquet"), str(tmp_path / "img"), str(tmp_path / "img"),
                              batch_size=2, is_test=True, device="cpu", res=32, mosaic={"close_epochs": 2})
    assert isinstance(tr, DevicePreppedLoader) and tr.transform.mosaic["close_epochs"] == 2 and va.transform.mosaic is None
    pf = DevicePrefetcher(tr, "cpu")
    torch.manual_seed(0)
    for epoch, on in enumerate((True, True, True, False, False)):
        pf.set_epoch(epoch, 5)
        assert tr.transform.mosaic_on is on
        del calls[:]
        for images, targets in pf:
            assert images.shape == (2, 3, 32, 32) and torch.isfinite(images).all()
            for t in targets:
                assert t["boxes"].shape[1] == 5 and t["boxes"].dtype == torch.float32 and "labels" not in t
                b = t["boxes"]
                assert (b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 0] + b[:, 2] <= 32.001).all() and (b[:, 1] + b[:, 3] <= 32.001).all()
        assert calls == (["image_prep_mosaic"] * 2 if on else ["image_prep"] * 2)
    pf.set_epoch(9, 5)                                  # resumed past the end: still off
    assert tr.transform.mosaic_on is False
    DevicePrefetcher(va, "cpu").set_epoch(0, 5)          # a loader whose transform has no mosaic: nothing to switch
    assert va.transform.mosaic_on is False


def test_c6_header_and_library_carry_the_entry_points():
    import ctypes
    from src.hipops import lib
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    block = next(b for b in text.split("/* ---- ") if b.startswith("on-device input pipeline"))
    assert "src/data/transforms.py:4-14" in block
    protos = lib.parse_header(os.path.join(ROOT, "include", "yolo_hip.h"))
    assert len(protos["yolo_mosaic_tile_bytes"][1]) == 0 and len(protos["yolo_mosaic_tile_fill"][1]) == 13
    assert protos["yolo_image_prep_mosaic"][2][:7] == ["src", "tiles_dev", "table_dev", "N", "S", "fill", "jitter"]
    assert len(protos["yolo_image_prep_mosaic"][1]) == 18
    so = ctypes.CDLL(lib.SO_PATH)
    for name in ("yolo_mosaic_tile_bytes", "yolo_mosaic_tile_fill", "yolo_image_prep_mosaic"):
        assert name in block and hasattr(so, name), name
    # the record: off (8 bytes), then H, W, flip, tw, th, x0, y0, cx, cy
    tb = lib.query("yolo_mosaic_tile_bytes")
    assert tb == 48
    host = torch.zeros(2 * 4 * tb, dtype=torch.uint8)
    assert lib.query("yolo_mosaic_tile_fill", host.data_ptr(), 1, 2, 1 << 33, 17, 301, 1, 5, 3, -2, 40, 7, 40) == 0
    rec = host[(4 + 2) * tb:(4 + 3) * tb]
    assert int(rec[:8].view(torch.int64)) == 1 << 33 and rec[8:44].view(torch.int32).tolist() == [17, 301, 1, 5, 3, -2, 40, 7, 40]
    assert int(host[:(4 + 2) * tb].sum()) == 0 and int(host[(4 + 3) * tb:].sum()) == 0
    for bad in ((1, 2, 0, 0, 301, 0, 5, 3, 0, 0, 7, 7), (1, 2, 0, 17, -1, 0, 5, 3, 0, 0, 7, 7), (1, 2, 0, 17, 301, 0, 0, 3, 0, 0, 7, 7),
                (1, 2, 0, 17, 301, 0, 5, 0, 0, 0, 7, 7), (1, 4, 0, 17, 301, 0, 5, 3, 0, 0, 7, 7), (1, -1, 0, 17, 301, 0, 5, 3, 0, 0, 7, 7)):
        assert lib.query("yolo_mosaic_tile_fill", host.data_ptr(), *bad) == 1001, bad
