"""The affine warp on the CPU: the proof of its comparator (tests/strict_affine.py: the fp32 restatement of k_affine's
operation order lies inside its own sets within the cap on every case, the exact class is exact, every mutant is rejected),
the matrix, the box rule, and the host logic of BatchTransform's affine (draw order, validation, per-epoch switch) with the
device leaves swapped for CPU stand-ins -- `image_prep` for the oracle (emulated_ops), `image_prep_mosaic` for
tests/mosaic_ref.py, `image_prep_affine` for tests/affine_ref.py -- and the C ABI of the new entry points (host-side calls)."""
import math
import os

import numpy as np
import pytest
import torch

import affine_ref as ar
import emulated_ops
import mosaic_ref
import strict_affine as sa
import strict_image as si
from src.hipops import ops as real_ops

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NO_JITTER = (1.0, 1.0, 1.0, 0.0)


@pytest.fixture(autouse=True)
def _emulate(monkeypatch):
    emulated_ops.install(monkeypatch)
    monkeypatch.setattr(real_ops, "image_prep_mosaic", mosaic_ref.image_prep_mosaic)
    monkeypatch.setattr(real_ops, "image_prep_affine", ar.image_prep_affine)


@pytest.fixture
def calls(monkeypatch):
    """Which of the three leaves a transform call went through."""
    seen = []
    for name in ("image_prep", "image_prep_mosaic", "image_prep_affine"):
        inner = getattr(real_ops, name)
        monkeypatch.setattr(real_ops, name, lambda *a, _n=name, _f=inner: (seen.append(_n), _f(*a))[1])
    return seen


# ------------------------------------------------------------------------------------------ the comparator's proof
@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("S", sa.SIZES)
def test_a1_the_fp32_restatement_lies_inside_its_own_sets_within_the_cap(S, kind):
    c = sa.canvas(S, kind)
    for name in sa.GENERAL:
        rec = sa.general_record(name, S)
        got = ar.warp_f32(c, rec)
        r = sa.check_warp(f"S={S} {kind} {name}", got, c, rec, record=False)         # raises CannotTell over the cap
        assert r["equal"] == r["n"] and r["ambiguous"] <= si.CAP_RESIZE * r["n"]
        out = ar.outside(rec, S)
        assert (got[out] == sa.FILL).all()
        x, e = sa.affine_ref_levels(c, rec)
        assert (e[out] == 0).all() and (x[out] == sa.FILL).all()                     # all four taps outside: fill, exactly
        if name == "pushed_out":
            assert out.all()
    assert not ar.outside(sa.general_record("rot10", S), S).all() and ar.outside(sa.general_record("rot10", S), S).any()


@pytest.mark.parametrize("S", sa.SIZES)
def test_a2_the_exact_class_is_one_level_and_is_the_index_arithmetic(S):
    c = sa.canvas(S, "noise")
    for name, (m, want) in sa.exact_matrices(S).items():
        rec = ar.inverse_record(m)
        x, e = sa.affine_ref_levels(c, rec)
        assert (e == 0).all(), f"{name}: {int((e != 0).sum())} elements are not in the exact class"
        assert np.array_equal(si.q_resize(x), want(c)), name
        assert np.array_equal(ar.warp_f32(c, rec), want(c)), name
    assert np.array_equal(ar.warp_f32(c, ar.IDENTITY), c)
    # a generic record has no exact pixel but the flat ones
    x, e = sa.affine_ref_levels(c, sa.general_record("gain1.5", S))
    assert (e[~ar.outside(sa.general_record("gain1.5", S), S)] > 0).mean() > 0.9


@pytest.mark.parametrize("mut", ar.MUTANTS)
def test_a3_every_mutant_is_rejected(mut):
    for S, name in ((96, "combined"), (33, "rot10")):
        c = sa.canvas(S, "noise")
        rec = sa.general_record(name, S)
        bad = ar.warp_f32(c, rec, mut=mut)
        assert si.failing(lambda: sa.check_warp(f"{mut} S={S} {name}", bad, c, rec, record=False)) == ["affine"], (mut, S, name)
    if mut in ("integer_centre", "transposed", "trunc"):
        return
    # a border mutant and a sampling mutant also show on a plain fractional shift
    c = sa.canvas(33, "noise")
    rec = sa.general_record("translate_lo", 33)
    bad = ar.warp_f32(c, rec, mut=mut)
    assert si.failing(lambda: sa.check_warp(mut, bad, c, rec, record=False)) == ["affine"]


# ------------------------------------------------------------------------------------------ the matrix
DRAWS = [(0.0, 1.0, 0.0, 0.0, 0.5, 0.5), (10.0, 1.0, 0.0, 0.0, 0.5, 0.5), (-137.0, 0.6, 0.0, 0.0, 0.41, 0.58), (0.0, 1.4, 8.0, -3.0, 0.5, 0.5),
         (33.0, 0.75, -6.0, 9.0, 0.6, 0.4), (180.0, 1.5, 0.0, 0.0, 0.5, 0.5)] + list(sa.GENERAL.values())


def test_b1_affine_matrix_against_an_independent_composition_and_its_inverse_record():
    from src.data.transforms import affine_matrix, affine_record
    for S in (96, 33, 640):
        for d in DRAWS:
            m = affine_matrix(d, S)
            assert m.shape == (2, 3) and m.dtype == np.float64
            np.testing.assert_allclose(m, ar.forward_matrix(d, S), rtol=0, atol=1e-12 * S)
            # the centre goes to (tx S, ty S); the gain is the length of a rotated unit step when nothing shears
            np.testing.assert_allclose(m @ [S / 2, S / 2, 1.0], [d[4] * S, d[5] * S], rtol=0, atol=1e-10 * S)
            if d[2] == 0 and d[3] == 0:
                assert abs(math.hypot(m[0, 0], m[1, 0]) - d[1]) < 1e-12
            rec = affine_record(m)
            assert len(rec) == 6 and all(float(np.float32(v)) == v for v in rec)
            assert rec == ar.inverse_record(m) or np.allclose(rec, ar.inverse_record(m), rtol=2 ** -22, atol=0)
            # M M^-1 = I up to the one fp32 rounding of each inverse entry
            m3 = np.vstack([m, [0, 0, 1.0]])
            i3 = np.array([[rec[0], rec[1], rec[2]], [rec[3], rec[4], rec[5]], [0, 0, 1.0]])
            assert (np.abs(m3 @ i3 - np.eye(3)) <= 2.0 ** -23 * (np.abs(m3) @ np.abs(i3))).all(), (S, d)
    assert affine_record([[1, 0, 0], [0, 1, 0]]) == ar.IDENTITY
    for bad in ([[1, 0, 0], [2, 0, 0]], [[0, 0, 1], [0, 0, 1]], [[float("nan"), 0, 0], [0, 1, 0]], [[1, 0, float("inf")], [0, 1, 0]],
                [[1, 0], [0, 1]], [[1e-30, 0, 0], [0, 1e-30, 0]]):
        with pytest.raises(ValueError, match="affine"):
            affine_record(bad)


# ------------------------------------------------------------------------------------------ the boxes
def test_b2_box_rule_on_fixed_cases():
    from src.data.transforms import affine_boxes
    S, kw = 64, dict(min_box=2.0, min_visible=0.1, max_aspect=100.0, max_boxes=128)
    t = torch.tensor
    # a box rotated a quarter turn about the centre: (x, y) -> (S - y, x)
    got = affine_boxes([[0, -1, S], [1, 0, 0]], t([[10., 20., 8., 4., 3.]]), S, **kw)
    assert torch.equal(got, t([[40., 10., 4., 8., 3.]])) and got.dtype == torch.float32
    shift = [[1, 0, -14], [0, 1, -14]]
    boxes = t([[10., 20., 8., 4., 1.],            # pushed half out on the left: x -4..4 -> 0..4
               [10., 30., 5., 10., 2.],           # x -4..1 -> 0..1: narrower than min_box (a fifth is visible: only that rule)
               [0., 0., 16.5, 16.5, 3.],          # -14..2.5 on both axes: 2.5 x 2.5 of 16.5 x 16.5 = 2.3 % visible
               [14., 20., 50., 3., 4.],           # 0..50 x 6..9, whole: aspect 16.7
               [30., 30., 10., 10., 5.]])
    assert torch.equal(affine_boxes(shift, boxes, S, **kw), t([[0., 6., 4., 4., 1.], [0., 6., 50., 3., 4.], [16., 16., 10., 10., 5.]]))
    assert [float(v) for v in affine_boxes(shift, boxes, S, **{**kw, "min_box": 1.0})[:, 4]] == [1., 2., 4., 5.]
    assert [float(v) for v in affine_boxes(shift, boxes, S, **{**kw, "min_visible": 0.02})[:, 4]] == [1., 3., 4., 5.]
    assert [float(v) for v in affine_boxes(shift, boxes, S, **{**kw, "max_aspect": 10.0})[:, 4]] == [1., 5.]
    # the visible share is taken against the box's area after the gain: a doubled box that stays inside is whole
    got = affine_boxes([[2, 0, 0], [0, 2, 0]], t([[4., 4., 10., 10., 7.], [28., 28., 10., 10., 8.]]), S, **kw)
    assert torch.equal(got, t([[8., 8., 20., 20., 7.], [56., 56., 8., 8., 8.]]))          # the second: 64 of 400 = 16 %
    assert affine_boxes([[2, 0, 0], [0, 2, 0]], t([[28., 28., 10., 10., 8.]]), S, **{**kw, "min_visible": 0.17}).shape == (0, 5)
    assert affine_boxes(shift, torch.zeros(0, 5), S, **kw).shape == (0, 5)
    # a rotated box grows to the hull of its corners
    m = ar.forward_matrix((45.0, 1.0, 0.0, 0.0, 0.5, 0.5), S)
    got = affine_boxes(m, t([[27., 27., 10., 10., 0.]]), S, **kw)
    r = 10 * math.sqrt(2)
    assert torch.allclose(got, t([[32 - r / 2, 32 - r / 2, r, r, 0.]]), rtol=0, atol=1e-4)
    # 200 boxes cut to 128: the largest clipped areas stay, in their order; ties keep the earlier box
    g = torch.Generator().manual_seed(2)
    many = torch.cat([torch.rand(200, 2, generator=g) * 40, torch.randint(3, 20, (200, 2), generator=g).float(), torch.arange(200.)[:, None]], 1)
    m = ar.forward_matrix((7.0, 1.1, 2.0, 0.0, 0.52, 0.5), S)
    full = affine_boxes(m, many, S, **{**kw, "max_boxes": 1000})
    cut = affine_boxes(m, many, S, **kw)
    assert full.shape[0] > 150 and cut.shape == (128, 5)
    order = sorted(range(full.shape[0]), key=lambda j: -float(full[j, 2] * full[j, 3]))[:128]
    assert torch.equal(cut, full[sorted(order)]) and bool((cut[1:, 4] > cut[:-1, 4]).all())
    # the restated rule gives the same on all of the above
    for mm, bb, k2 in ((shift, boxes, kw), (shift, boxes, {**kw, "min_box": 1.0}), (shift, boxes, {**kw, "max_aspect": 10.0}),
                       (shift, boxes, {**kw, "min_visible": 0.02}), (m, many, kw), (m, many, {**kw, "max_boxes": 1000}),
                       ([[0, -1, S], [1, 0, 0]], boxes, kw), (ar.forward_matrix(sa.GENERAL["combined"], S), many, kw)):
        assert torch.equal(affine_boxes(mm, bb, S, **k2), ar.affine_boxes(mm, bb, S, **k2))


# ------------------------------------------------------------------------------------------ the host logic
def _inputs():
    rng = np.random.default_rng(3)
    imgs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)) for h, w in ((40, 60), (33, 20), (64, 64))]
    tg = [{"boxes": torch.tensor([[10., 5., 20., 10.]]), "labels": torch.tensor([[3.]]), "name": "a"},
          {"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, 1), "name": "b"},
          {"boxes": torch.tensor([[0., 0., 64., 64.], [16., 8., 8., 4.]]), "labels": torch.tensor([[1.], [2.]]), "name": "c"}]
    return imgs, tg


def _u(lo, hi):
    return float(torch.empty(1).uniform_(lo, hi))


def test_c1_draws_follow_the_stated_order_and_leave_sample_and_sample_mosaic_alone(calls):
    from src.data.transforms import BatchTransform, affine_matrix, affine_record
    imgs, tg = _inputs()
    n, S = len(imgs), 32
    mcfg = {"p": 0.6, "gain": [0.5, 1.5]}
    acfg = {"degrees": 15.0, "translate": 0.2, "scale": 0.4, "shear": 3.0}
    tr = BatchTransform(True, size=S, device="cpu", mosaic=mcfg, affine=acfg)
    base = BatchTransform(True, size=S, device="cpu", mosaic=mcfg)
    torch.manual_seed(4)
    params, mdraws, adraws = [tr.sample() for _ in range(n)], tr.sample_mosaic(n), tr.sample_affine(n)
    after = float(torch.rand(1))
    torch.manual_seed(4)
    assert params == [base.sample() for _ in range(n)] and mdraws == base.sample_mosaic(n)
    want = [(_u(-15, 15), _u(0.6, 1.4), _u(-3, 3), _u(-3, 3), _u(0.3, 0.7), _u(0.3, 0.7)) for _ in range(n)]
    assert adraws == want and after == float(torch.rand(1))
    for d in adraws:
        assert -15 <= d[0] <= 15 and 0.6 <= d[1] <= 1.4 and abs(d[2]) <= 3 and abs(d[3]) <= 3 and 0.3 <= d[4] <= 0.7 and 0.3 <= d[5] <= 0.7
    # six draws per output also when every range is 0: the draws are the identity and the RNG has moved by 6 n uniforms
    tr0 = BatchTransform(True, size=S, device="cpu", affine={"degrees": 0, "translate": 0, "scale": 0, "shear": 0})
    torch.manual_seed(9)
    zero = tr0.sample_affine(n)
    after0 = float(torch.rand(1))
    torch.manual_seed(9)
    for _ in range(6 * n):
        torch.empty(1).uniform_(0, 1)
    assert after0 == float(torch.rand(1)) and zero == [(0.0, 1.0, 0.0, 0.0, 0.5, 0.5)] * n
    assert affine_record(affine_matrix(zero[0], S)) == ar.IDENTITY

    # a whole call draws sample() x n, sample_mosaic(n), sample_affine(n): the same batch from the seed as from the decisions
    torch.manual_seed(4)
    got, got_t = tr(imgs, tg)
    want_b, want_t = tr(imgs, tg, params=params, mosaic=mdraws, affine=adraws)
    assert torch.equal(got, want_b) and all(torch.equal(a["boxes"], b["boxes"]) for a, b in zip(got_t, want_t))
    assert calls == ["image_prep_affine", "image_prep_affine"]
    # ... and finished forward matrices are taken like draws
    mats = [affine_matrix(d, S) for d in adraws]
    again, again_t = tr(imgs, tg, params=params, mosaic=mdraws, affine=mats)
    assert torch.equal(again, want_b) and all(torch.equal(a["boxes"], b["boxes"]) for a, b in zip(again_t, want_t))
    # the boxes are affine_boxes of what the mosaic-only transform gives
    _, base_t = base(imgs, tg, params=params, mosaic=mdraws)
    for a, b, m in zip(want_t, base_t, mats):
        assert torch.equal(a["boxes"], ar.affine_boxes(m, b["boxes"], S)) and a["name"] == b["name"] and "labels" not in a
    # identity records: the batch is the mosaic-only transform's, bit for bit (the stand-in's warp is exact there too)
    same, same_t = tr(imgs, tg, params=params, mosaic=mdraws, affine=[None] * n)
    base_b, _ = base(imgs, tg, params=params, mosaic=mdraws)
    assert torch.equal(same, base_b)

    # affine switched off: the calls, the draws and the outputs are those of a transform built without the key
    del calls[:]
    tr.affine_on = False
    torch.manual_seed(4)
    off, off_t = tr(imgs, tg)
    rng_after = float(torch.rand(1))
    torch.manual_seed(4)
    plain, plain_t = base(imgs, tg)
    assert rng_after == float(torch.rand(1)) and calls == ["image_prep_mosaic", "image_prep_mosaic"]
    assert torch.equal(off, plain) and all(torch.equal(a["boxes"], b["boxes"]) for a, b in zip(off_t, plain_t))
    # ... and with the mosaic off as well, today's plain path
    del calls[:]
    tr.mosaic_on = False
    torch.manual_seed(4)
    off, _ = tr(imgs, tg)
    torch.manual_seed(4)
    plain, _ = BatchTransform(True, size=S, device="cpu")(imgs, tg)
    assert calls == ["image_prep", "image_prep"] and torch.equal(off, plain)
    # the warp alone, no mosaic: the plain canvas is what is warped
    del calls[:]
    only = BatchTransform(True, size=S, device="cpu", affine=acfg)
    torch.manual_seed(4)
    p2 = [only.sample() for _ in range(n)]
    a2 = only.sample_affine(n)
    torch.manual_seed(4)
    got, got_t = only(imgs, tg)
    assert calls == ["image_prep_affine"] and p2 == params
    plain_b, plain_t = BatchTransform(True, size=S, device="cpu")(imgs, tg, params=p2)
    for i in range(n):
        assert torch.equal(got_t[i]["boxes"], ar.affine_boxes(affine_matrix(a2[i], S), plain_t[i]["boxes"], S))
    assert not torch.equal(got, plain_b)


def test_c2_validation_of_keys_and_ranges_and_who_refuses_the_key():
    from src.data.data_loader import get_data_loaders
    from src.data.transforms import AFFINE_DEFAULTS, BatchTransform, get_train_transforms, get_val_transforms
    for bad in ({"degrees": -1}, {"degrees": 181}, {"translate": -0.1}, {"translate": 1.0}, {"scale": -0.1}, {"scale": 1.0}, {"shear": -1},
                {"shear": 90}, {"fill": 256}, {"fill": -1}, {"max_boxes": 0}, {"close_epochs": -1}, {"perspective": 0.001}, {"p": 1.0}):
        with pytest.raises(ValueError, match="affine"):
            BatchTransform(True, size=32, device="cpu", affine=bad)
    with pytest.raises(ValueError, match="training augmentation"):
        BatchTransform(False, size=32, device="cpu", affine={})
    with pytest.raises(ValueError, match="one level"):
        BatchTransform(True, size=32, device="cpu", mosaic={"fill": 0}, affine={})
    assert get_val_transforms(32, "cpu").affine is None and get_val_transforms(32, "cpu").affine_on is False
    tr = get_train_transforms(32, "cpu", affine={})
    assert tr.affine == dict(degrees=0.0, translate=0.1, scale=0.5, shear=0.0, fill=114, min_box=2.0, min_visible=0.1, max_aspect=100.0,
                             max_boxes=128, close_epochs=0) == AFFINE_DEFAULTS
    assert tr.affine_on is True and tr.mosaic is None
    edge = BatchTransform(True, size=32, device="cpu", affine={"degrees": 180, "shear": 89, "translate": 0.99, "scale": 0.99, "fill": 0})
    assert edge.affine["degrees"] == 180.0 and edge.affine["fill"] == 0
    plain = get_train_transforms(32, "cpu")
    assert plain.affine is None and plain.affine_on is False
    imgs, tg = _inputs()
    with pytest.raises(ValueError, match="without affine"):
        plain(imgs, tg, affine=[None] * 3)
    with pytest.raises(ValueError, match="without affine"):
        plain.sample_affine(3)
    with pytest.raises(ValueError, match="records for 3 images"):
        tr(imgs, tg, affine=[None] * 2)
    with pytest.raises(ValueError, match="six values or a 2 x 3"):
        tr(imgs, tg, affine=[None, (1.0, 2.0), None])
    with pytest.raises(ValueError, match="singular"):
        tr(imgs, tg, affine=[None, [[1, 2, 0], [2, 4, 0]], None])
    with pytest.raises(ValueError, match="decoded images"):
        get_data_loaders("/nonexistent/train", "/nonexistent/val", "", "", batch_size=2, is_test=True, device="cpu", res=32, affine={})
    tr_l, _ = get_data_loaders("/nonexistent/train", "/nonexistent/val", "", "", batch_size=2, is_test=True, device="cpu", res=32)
    assert not hasattr(tr_l, "set_epoch")              # the synthetic path is as before


def test_c3_set_epoch_closes_the_warp_beside_the_mosaic(calls, tmp_path):
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
                              batch_size=2, is_test=True, device="cpu", res=32, mosaic={"close_epochs": 3},
                              affine={"degrees": 10.0, "close_epochs": 1})
    assert isinstance(tr, DevicePreppedLoader) and tr.transform.affine["close_epochs"] == 1 and va.transform.affine is None
    pf = DevicePrefetcher(tr, "cpu")
    torch.manual_seed(0)
    for epoch, (mos, aff) in enumerate(((True, True), (True, True), (False, True), (False, True), (False, False))):
        pf.set_epoch(epoch, 5)
        assert tr.transform.mosaic_on is mos and tr.transform.affine_on is aff
        del calls[:]
        for images, targets in pf:
            assert images.shape == (2, 3, 32, 32) and torch.isfinite(images).all()
            for t in targets:
                b = t["boxes"]
                assert b.shape[1] == 5 and b.dtype == torch.float32 and "labels" not in t
                assert (b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 0] + b[:, 2] <= 32.001).all() and (b[:, 1] + b[:, 3] <= 32.001).all()
        assert calls == ["image_prep_affine" if aff else "image_prep_mosaic" if mos else "image_prep"] * 2
    pf.set_epoch(9, 5)                                  # resumed past the end: still off
    assert tr.transform.affine_on is False
    DevicePrefetcher(va, "cpu").set_epoch(0, 5)          # a loader whose transform has no warp: nothing to switch
    assert va.transform.affine_on is False


def test_c4_header_and_library_carry_the_entry_points():
    import ctypes
    from src.hipops import lib
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    block = next(b for b in text.split("/* ---- ") if b.startswith("on-device input pipeline"))
    protos = lib.parse_header(os.path.join(ROOT, "include", "yolo_hip.h"))
    assert len(protos["yolo_affine_bytes"][1]) == 0
    assert protos["yolo_affine_fill"][2] == ["table_host", "index", "a00", "a01", "b0", "a10", "a11", "b1"]
    assert protos["yolo_image_prep_affine"][2][:10] == ["src", "tiles_dev", "table_dev", "affine_dev", "N", "S", "fill", "jitter", "stage", "stage2"]
    assert len(protos["yolo_image_prep_affine"][1]) == 20
    so = ctypes.CDLL(lib.SO_PATH)
    for name in ("yolo_affine_bytes", "yolo_affine_fill", "yolo_image_prep_affine"):
        assert name in block and hasattr(so, name), name
    # the parent's two entry points are declared as they were
    assert len(protos["yolo_image_prep"][1]) == 16 and len(protos["yolo_image_prep_mosaic"][1]) == 18
    ab = lib.query("yolo_affine_bytes")
    assert ab == 24
    host = torch.zeros(3 * ab, dtype=torch.uint8)
    vals = (0.75, -0.25, 3.5, 0.125, 1.5, -40.0)
    assert lib.query("yolo_affine_fill", host.data_ptr(), 1, *vals) == 0
    assert host[ab:2 * ab].view(torch.float32).tolist() == list(vals)
    assert int(host[:ab].sum()) == 0 and int(host[2 * ab:].sum()) == 0
    for k in range(6):
        for v in (float("nan"), float("inf"), -float("inf")):
            bad = list(vals)
            bad[k] = v
            assert lib.query("yolo_affine_fill", host.data_ptr(), 0, *bad) == 1001, (k, v)
    assert lib.query("yolo_affine_fill", host.data_ptr(), -1, *vals) == 1001 and int(host[:ab].sum()) == 0
