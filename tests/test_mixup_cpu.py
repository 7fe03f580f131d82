"""The mixup on the CPU: the proof of its comparator (tests/mixup_ref.py: the fp32 restatement of k_mixup's operation order is
exact at r = 0 and r = 1 and every named mutant differs from it on the all-pairs lattice or on a mutual pair / a 3-chain), the
box rule, and the host logic of BatchTransform's mixup (draw order, validation, per-epoch switch, the leaf a batch takes) with the
device leaves swapped for CPU stand-ins -- `image_prep` for the oracle (emulated_ops), `image_prep_mosaic` for
tests/mosaic_ref.py, `image_prep_affine` for tests/affine_ref.py, `image_prep_mixup` for tests/mixup_ref.py -- and the C ABI of
the new entry points (host-side calls)."""
import os

import numpy as np
import pytest
import torch

import affine_ref as ar
import emulated_ops
import mixup_ref as mr
import mosaic_ref
from src.hipops import ops as real_ops

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REAL_MIXUP = real_ops.image_prep_mixup                 # the leaf itself, before the fixture below swaps it
LEAVES = ("image_prep", "image_prep_mosaic", "image_prep_affine", "image_prep_mixup")


@pytest.fixture(autouse=True)
def _emulate(monkeypatch):
    emulated_ops.install(monkeypatch)
    monkeypatch.setattr(real_ops, "image_prep_mosaic", mosaic_ref.image_prep_mosaic)
    monkeypatch.setattr(real_ops, "image_prep_affine", ar.image_prep_affine)
    monkeypatch.setattr(real_ops, "image_prep_mixup", mr.image_prep_mixup)


@pytest.fixture
def calls(monkeypatch):
    """Which of the four leaves a transform call went through."""
    seen = []
    for name in LEAVES:
        inner = getattr(real_ops, name)
        monkeypatch.setattr(real_ops, name, lambda *a, _n=name, _f=inner: (seen.append(_n), _f(*a))[1])
    return seen


# ------------------------------------------------------------------------------------------ A: the comparator is sharp
def test_a1_the_ends_of_the_ratio_are_exact_on_every_pair_of_levels():
    a, b = mr.lattice()
    assert a.shape == (65536,) and len(set(zip(a.tolist(), b.tolist()))) == 65536
    assert mr.RATIOS == [0.0, 1.0, 0.5, 0.25, 0.3, 0.7, 0.4719, 2.0 ** -10]
    assert np.array_equal(mr.blend_f32(a, b, 1.0), a) and np.array_equal(mr.blend_f32(a, b, 0.0), b)
    for r in mr.RATIOS:
        got = mr.blend_f32(a, b, r)
        assert got.dtype == np.float32 and np.array_equal(got, np.round(got)) and got.min() >= 0 and got.max() <= 255
        # the restatement lies within half a level (plus the fp32 roundings of three operations on values <= 255) of the real blend
        real = float(np.float32(r)) * a.astype(np.float64) + (1.0 - float(np.float32(r))) * b.astype(np.float64)
        assert np.abs(got - real).max() <= 0.5 + 3 * 255 * 2.0 ** -24
        assert np.array_equal(got[a == b], a[a == b]) or r not in (0.0, 1.0, 0.5, 0.25)      # equal levels stay at binary ratios
    # an unmixed record and a partner equal to the output's own index are copies
    c = np.stack([a.reshape(256, 256), b.reshape(256, 256)])
    assert np.array_equal(mr.mix_f32(c, [None, (1, 0.3)]), c)


@pytest.mark.parametrize("mut", mr.ARITHMETIC_MUTANTS)
def test_a2_every_arithmetic_mutant_differs_for_a_ratio_of_the_list(mut):
    a, b = mr.lattice()
    diff = {r: int((mr.blend_f32(a, b, r, mut) != mr.blend_f32(a, b, r)).sum()) for r in mr.RATIOS}
    print(f"\n[mixup_ref] {mut}: elements of 65536 that differ, per ratio: {diff}")
    assert max(diff.values()) > 0, diff
    if mut in ("swap", "rint", "trunc"):
        assert diff[0.25] > 0
    else:                                       # the single-rounding mutants show only at ratios that are no short binary fraction
        assert diff[0.3] > 0 and diff[0.7] > 0 and all(diff[r] == 0 for r in (0.0, 1.0, 0.5, 0.25, 2.0 ** -10))
    # ... and through mix_f32, as the GPU tests use it
    c = np.stack([a.reshape(256, 256), b.reshape(256, 256)])
    recs = [(1, 0.3), (0, 0.25)]
    assert not np.array_equal(mr.mix_f32(c, recs, mut), mr.mix_f32(c, recs))


def test_a3_a_partner_read_after_it_was_mixed_is_rejected_by_a_mutual_pair_and_by_a_chain():
    rng = np.random.default_rng(1)
    c = rng.integers(0, 256, (3, 16, 16, 3)).astype(np.float32)
    for recs in ([(1, 0.5), (0, 0.5), None], [(1, 0.3), (2, 0.7), (0, 0.25)]):
        good, bad = mr.mix_f32(c, recs), mr.mix_f32(c, recs, "inplace")
        assert not np.array_equal(good, bad), recs
        for i, rec in enumerate(recs):          # every output is the blend of two UNMIXED canvases
            assert np.array_equal(good[i], c[i] if rec is None else mr.blend_f32(c[i], c[rec[0]], rec[1]))
    assert np.array_equal(mr.mix_f32(c, [None, None, (0, 0.3)], "inplace"), mr.mix_f32(c, [None, None, (0, 0.3)]))     # nothing to catch
    with pytest.raises(ValueError, match="records for"):
        mr.mix_f32(c, [None])


# ------------------------------------------------------------------------------------------ B: the boxes
def test_b1_box_rule_on_fixed_cases():
    from src.data.transforms import mixup_boxes
    t = torch.tensor
    own = t([[1., 2., 10., 4., 3.], [5., 5., 2., 2., 4.]])
    par = t([[0., 0., 8., 8., 7.]])
    got = mixup_boxes(own, par, 128)
    assert torch.equal(got, t([[1., 2., 10., 4., 3.], [5., 5., 2., 2., 4.], [0., 0., 8., 8., 7.]])) and got.dtype == torch.float32
    assert torch.equal(mixup_boxes(par, own, 128), torch.cat([par, own]))                  # own first, then the partner's
    assert torch.equal(mixup_boxes(torch.zeros(0, 5), par, 128), par) and torch.equal(mixup_boxes(own, torch.zeros(0, 5), 128), own)
    assert mixup_boxes(torch.zeros(0, 5), torch.zeros(0, 5), 128).shape == (0, 5)
    # the cut keeps the largest areas in order: areas 40, 4, 64 -> two stay, the first and the third
    assert torch.equal(mixup_boxes(own, par, 2), t([[1., 2., 10., 4., 3.], [0., 0., 8., 8., 7.]]))
    assert torch.equal(mixup_boxes(own, par, 1), par)
    # 120 + 120 boxes cut to 128; ties keep the earlier box
    g = torch.Generator().manual_seed(3)
    a = torch.cat([torch.rand(120, 2, generator=g) * 40, torch.randint(3, 20, (120, 2), generator=g).float(), torch.arange(120.)[:, None]], 1)
    b = torch.cat([torch.rand(120, 2, generator=g) * 40, torch.randint(3, 20, (120, 2), generator=g).float(), 120 + torch.arange(120.)[:, None]], 1)
    cut, full = mixup_boxes(a, b, 128), torch.cat([a, b])
    order = sorted(range(240), key=lambda j: -float(full[j, 2] * full[j, 3]))[:128]
    assert cut.shape == (128, 5) and torch.equal(cut, full[sorted(order)]) and bool((cut[1:, 4] > cut[:-1, 4]).all())
    assert len(set(float(v) for v in full[:, 2] * full[:, 3])) < 240                      # there are ties in this set
    for own_, par_, k in ((own, par, 128), (own, par, 2), (a, b, 128), (b, a, 128), (a, b, 5), (a, torch.zeros(0, 5), 100)):
        assert torch.equal(mixup_boxes(own_, par_, k), mr.mixup_boxes(own_, par_, k))


def test_b2_the_shared_cap_gives_mosaic_boxes_and_affine_boxes_the_outputs_they_had():
    from src.data.transforms import affine_boxes, keep_largest, mosaic_boxes
    g = torch.Generator().manual_seed(2)
    many = torch.cat([torch.rand(200, 2, generator=g) * 40, torch.randint(3, 20, (200, 2), generator=g).float(), torch.arange(200.)[:, None]], 1)
    # the helper itself: rows of the largest areas, in their order, ties to the earlier row
    area = torch.tensor([4., 9., 9., 1., 16.])
    rows = torch.arange(5.)[:, None].repeat(1, 5)
    assert torch.equal(keep_largest(rows, area, 5), rows) and torch.equal(keep_largest(rows, area, 9), rows)
    assert torch.equal(keep_largest(rows, area, 2)[:, 0], torch.tensor([1., 4.]))
    assert torch.equal(keep_largest(rows, area, 3)[:, 0], torch.tensor([1., 2., 4.]))
    # affine_boxes: test_affine_cpu.py's case of 200 boxes under a small warp, against the restated rule
    S = 64
    m = ar.forward_matrix((7.0, 1.1, 2.0, 0.0, 0.52, 0.5), S)
    kw = dict(min_box=2.0, min_visible=0.1, max_aspect=100.0)
    for cap in (128, 50, 1000):
        assert torch.equal(affine_boxes(m, many, S, max_boxes=cap, **kw), ar.affine_boxes(m, many, S, max_boxes=cap, **kw))
    assert affine_boxes(m, many, S, max_boxes=128, **kw).shape == (128, 5)
    # mosaic_boxes: four tiles of one image with 200 boxes, against the restated rule
    sizes = [(64, 64)]
    tg = [{"boxes": many[:, :4], "labels": many[:, 4:5]}]
    rec = {"cx": 30, "cy": 34, "tiles": [(0, False, 40, 40, -10, -6), (0, True, 34, 34, 30, 0), (0, False, 30, 30, 0, 34), (0, False, 50, 50, 30, 34)]}
    for cap in (128, 50, 1000):
        got = mosaic_boxes(rec, tg, sizes, S, 2.0, 0.1, cap)
        assert torch.equal(got, mosaic_ref.mosaic_boxes(rec, tg, sizes, S, max_boxes=cap))
    assert mosaic_boxes(rec, tg, sizes, S, 2.0, 0.1, 128).shape == (128, 5) and mosaic_boxes(rec, tg, sizes, S, 2.0, 0.1, 1000).shape[0] > 128


# ------------------------------------------------------------------------------------------ C: the host logic
def _inputs():
    rng = np.random.default_rng(3)
    imgs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)) for h, w in ((40, 60), (33, 20), (64, 64))]
    tg = [{"boxes": torch.tensor([[10., 5., 20., 10.]]), "labels": torch.tensor([[3.]]), "name": "a", "image_id": 7},
          {"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, 1), "name": "b", "image_id": 8},
          {"boxes": torch.tensor([[0., 0., 64., 64.], [16., 8., 8., 4.]]), "labels": torch.tensor([[1.], [2.]]), "name": "c", "image_id": 9}]
    return imgs, tg


def _same(a, b):
    return all(torch.equal(x["boxes"], y["boxes"]) and x["name"] == y["name"] and x["image_id"] == y["image_id"] for x, y in zip(a, b))


def test_c1_draws_follow_the_stated_order_and_leave_the_three_earlier_sequences_alone(calls):
    from src.data.transforms import BatchTransform
    imgs, tg = _inputs()
    n, S = len(imgs), 32
    mcfg = {"p": 0.6, "gain": [0.5, 1.5]}
    acfg = {"degrees": 15.0, "translate": 0.2, "scale": 0.4, "shear": 3.0}
    xcfg = {"p": 0.7, "alpha": 8.0}
    tr = BatchTransform(True, size=S, device="cpu", mosaic=mcfg, affine=acfg, mixup=xcfg)
    base = BatchTransform(True, size=S, device="cpu", mosaic=mcfg, affine=acfg)
    torch.manual_seed(4)
    params, mdraws, adraws, xdraws = [tr.sample() for _ in range(n)], tr.sample_mosaic(n), tr.sample_affine(n), tr.sample_mixup(n)
    after = float(torch.rand(1))
    torch.manual_seed(4)
    assert params == [base.sample() for _ in range(n)] and mdraws == base.sample_mosaic(n) and adraws == base.sample_affine(n)
    want = []
    for i in range(n):
        if not bool(torch.rand(1) < 0.7):
            want.append(None)
            continue
        d = int(torch.randint(1, n, (1,)))
        want.append(((i + d) % n, float(torch.distributions.Beta(8.0, 8.0).sample())))
    assert xdraws == want and after == float(torch.rand(1))
    assert any(x is None for x in xdraws) and sum(x is not None for x in xdraws) >= 1, xdraws
    for i, x in enumerate(xdraws):
        if x is not None:
            assert isinstance(x[0], int) and 0 <= x[0] < n and x[0] != i and 0.0 <= x[1] <= 1.0 and float(np.float32(x[1])) == x[1]
    # p = 1: every output mixes with another output; p = 0: one rand per output and nothing else
    always = BatchTransform(True, size=S, device="cpu", mixup={"p": 1.0})
    torch.manual_seed(1)
    for _ in range(20):
        for i, x in enumerate(always.sample_mixup(5)):
            assert x is not None and x[0] != i and 0 <= x[0] < 5 and 0.25 < x[1] < 0.75         # Beta(32, 32): sd 0.06 around 0.5
    never = BatchTransform(True, size=S, device="cpu", mixup={"p": 0.0})
    torch.manual_seed(9)
    assert never.sample_mixup(4) == [None] * 4
    after0 = float(torch.rand(1))
    torch.manual_seed(9)
    for _ in range(4):
        torch.rand(1)
    assert after0 == float(torch.rand(1))
    # n < 2: no partner exists, nothing is drawn
    torch.manual_seed(9)
    state = torch.get_rng_state()
    assert always.sample_mixup(1) == [None] and always.sample_mixup(0) == [] and torch.equal(torch.get_rng_state(), state)

    # a whole call draws sample() x n, sample_mosaic(n), sample_affine(n), sample_mixup(n): the same batch from the seed as from the decisions
    torch.manual_seed(4)
    got, got_t = tr(imgs, tg)
    want_b, want_t = tr(imgs, tg, params=params, mosaic=mdraws, affine=adraws, mixup=xdraws)
    assert torch.equal(got, want_b) and _same(got_t, want_t) and calls == ["image_prep_mixup", "image_prep_mixup"]
    # boxes: own final boxes, then those of the partner's UNMIXED output; names and ids stay those of the output
    base_b, base_t = base(imgs, tg, params=params, mosaic=mdraws, affine=adraws)
    for i, x in enumerate(xdraws):
        ref = base_t[i]["boxes"] if x is None else mr.mixup_boxes(base_t[i]["boxes"], base_t[x[0]]["boxes"])
        assert torch.equal(want_t[i]["boxes"], ref) and want_t[i]["boxes"].dtype == torch.float32 and want_t[i]["boxes"].shape[1] == 5
        assert want_t[i]["name"] == tg[i]["name"] and want_t[i]["image_id"] == tg[i]["image_id"] and "labels" not in want_t[i]
        if x is None:                           # an unmixed output of a mixing batch is the base transform's, bit for bit
            assert torch.equal(want_b[i], base_b[i])
    assert any(not torch.equal(want_b[i], base_b[i]) for i, x in enumerate(xdraws) if x is not None)
    # a partner that itself mixes still gives its unmixed boxes; a chain 0 -> 1 -> 2 -> 0 and r = 1 (the image stays, the boxes join)
    chain = [(1, 1.0), (2, 0.5), (0, 0.25)]
    ch_b, ch_t = tr(imgs, tg, params=params, mosaic=mdraws, affine=adraws, mixup=chain)
    for i, (j, _) in enumerate(chain):
        assert torch.equal(ch_t[i]["boxes"], torch.cat([base_t[i]["boxes"], base_t[j]["boxes"]]))
    assert torch.equal(ch_b[0], base_b[0]) and not torch.equal(ch_b[1], base_b[1])


def test_c2_a_batch_in_which_nobody_mixes_takes_the_parents_leaf_and_a_closed_mixup_draws_nothing(calls):
    from src.data.transforms import BatchTransform
    imgs, tg = _inputs()
    S = 32
    mcfg, acfg = {"p": 0.6, "gain": [0.5, 1.5]}, {"degrees": 15.0}
    for kw, leaf in (({}, "image_prep"), ({"mosaic": mcfg}, "image_prep_mosaic"), ({"affine": acfg}, "image_prep_affine"),
                     ({"mosaic": mcfg, "affine": acfg}, "image_prep_affine")):
        tr = BatchTransform(True, size=S, device="cpu", mixup={"p": 1.0}, **kw)
        base = BatchTransform(True, size=S, device="cpu", **kw)
        # explicit records, none of which mixes
        del calls[:]
        torch.manual_seed(5)
        got, got_t = tr(imgs, tg, mixup=[None] * 3)
        after = torch.get_rng_state()
        torch.manual_seed(5)
        want, want_t = base(imgs, tg)
        assert calls == [leaf, leaf] and torch.equal(got, want) and _same(got_t, want_t) and torch.equal(torch.get_rng_state(), after)
        # sampled, every output mixes: the mixup leaf, and the other draws are where they were
        del calls[:]
        torch.manual_seed(5)
        mixed, mixed_t = tr(imgs, tg)
        assert calls == ["image_prep_mixup"] and not torch.equal(mixed, want)
        assert all(a["boxes"].shape[0] >= b["boxes"].shape[0] for a, b in zip(mixed_t, want_t))
        # p = 0: sampled, nobody mixes -> the parent's leaf
        del calls[:]
        tr0 = BatchTransform(True, size=S, device="cpu", mixup={"p": 0.0}, **kw)
        torch.manual_seed(5)
        got, got_t = tr0(imgs, tg)
        assert calls == [leaf] and torch.equal(got, want) and _same(got_t, want_t)
        # switched off: the calls, the draws and the outputs are those of a transform built without the key
        del calls[:]
        tr.mixup_on = False
        torch.manual_seed(5)
        got, got_t = tr(imgs, tg)
        assert calls == [leaf] and torch.equal(got, want) and _same(got_t, want_t) and torch.equal(torch.get_rng_state(), after)
        # ... while records passed by hand still apply
        del calls[:]
        tr(imgs, tg, mixup=[(1, 0.5), None, None])
        assert calls == ["image_prep_mixup"]
    # one image: nothing to mix with, nothing drawn, the plain leaf
    del calls[:]
    one = BatchTransform(True, size=S, device="cpu", mixup={"p": 1.0})
    torch.manual_seed(6)
    got, _ = one(imgs[:1], tg[:1])
    after = torch.get_rng_state()
    torch.manual_seed(6)
    want, _ = BatchTransform(True, size=S, device="cpu")(imgs[:1], tg[:1])
    assert calls == ["image_prep", "image_prep"] and torch.equal(got, want) and torch.equal(torch.get_rng_state(), after)


def test_c3_validation_of_keys_and_ranges_and_who_refuses_the_key():
    from src.data.data_loader import get_data_loaders
    from src.data.transforms import MIXUP_DEFAULTS, BatchTransform, get_train_transforms, get_val_transforms
    assert MIXUP_DEFAULTS == dict(p=0.1, alpha=32.0, max_boxes=128, close_epochs=0)
    for bad in ({"p": -0.1}, {"p": 1.1}, {"alpha": 0}, {"alpha": -1.0}, {"alpha": float("inf")}, {"alpha": float("nan")}, {"max_boxes": 0},
                {"close_epochs": -1}, {"beta": 1.0}, {"fill": 114}):
        with pytest.raises(ValueError, match="mixup"):
            BatchTransform(True, size=32, device="cpu", mixup=bad)
    with pytest.raises(ValueError, match="training augmentation"):
        BatchTransform(False, size=32, device="cpu", mixup={})
    assert get_val_transforms(32, "cpu").mixup is None and get_val_transforms(32, "cpu").mixup_on is False
    tr = get_train_transforms(32, "cpu", mixup={})
    assert tr.mixup == MIXUP_DEFAULTS and tr.mixup_on is True and tr.mosaic is None and tr.affine is None
    edge = BatchTransform(True, size=32, device="cpu", mixup={"p": 1, "alpha": 0.1, "max_boxes": 1, "close_epochs": 3})
    assert edge.mixup == dict(p=1.0, alpha=0.1, max_boxes=1, close_epochs=3)
    plain = get_train_transforms(32, "cpu")
    assert plain.mixup is None and plain.mixup_on is False
    imgs, tg = _inputs()
    with pytest.raises(ValueError, match="without mixup"):
        plain(imgs, tg, mixup=[None] * 3)
    with pytest.raises(ValueError, match="without mixup"):
        plain.sample_mixup(3)
    with pytest.raises(ValueError, match="records for 3 images"):
        tr(imgs, tg, mixup=[None] * 2)
    for bad in ((3, 0.5), (-1, 0.5), (1, 0.5), (0, 1.5), (0, -0.1), (0, float("nan")), (0.5, 0.5), (0,)):
        with pytest.raises(ValueError, match="mixup record 1"):
            tr(imgs, tg, mixup=[None, bad, None])
    with pytest.raises(ValueError, match="decoded images"):
        get_data_loaders("/nonexistent/train", "/nonexistent/val", "", "", batch_size=2, is_test=True, device="cpu", res=32, mixup={})
    tr_l, _ = get_data_loaders("/nonexistent/train", "/nonexistent/val", "", "", batch_size=2, is_test=True, device="cpu", res=32)
    assert not hasattr(tr_l, "set_epoch")              # the synthetic path is as before


def test_c4_set_epoch_closes_the_mixup_independently_of_the_other_two_switches(calls, tmp_path):
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
                              affine={"degrees": 10.0, "close_epochs": 1}, mixup={"p": 1.0, "close_epochs": 2})
    assert isinstance(tr, DevicePreppedLoader) and tr.transform.mixup["close_epochs"] == 2 and va.transform.mixup is None
    pf = DevicePrefetcher(tr, "cpu")
    torch.manual_seed(0)
    for epoch, (mos, aff, mix) in enumerate(((True, True, True), (True, True, True), (False, True, True), (False, True, False), (False, False, False))):
        pf.set_epoch(epoch, 5)
        assert tr.transform.mosaic_on is mos and tr.transform.affine_on is aff and tr.transform.mixup_on is mix
        del calls[:]
        for images, targets in pf:
            assert images.shape == (2, 3, 32, 32) and torch.isfinite(images).all()
            for t in targets:
                b = t["boxes"]
                assert b.shape[1] == 5 and b.dtype == torch.float32 and "labels" not in t
                assert (b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 0] + b[:, 2] <= 32.001).all() and (b[:, 1] + b[:, 3] <= 32.001).all()
        assert calls == ["image_prep_mixup" if mix else "image_prep_affine" if aff else "image_prep_mosaic" if mos else "image_prep"] * 2
    pf.set_epoch(9, 5)                                  # resumed past the end: still off
    assert tr.transform.mixup_on is False
    DevicePrefetcher(va, "cpu").set_epoch(0, 5)          # a loader whose transform has no mixup: nothing to switch
    assert va.transform.mixup_on is False
    # the mixup closes alone, too
    tr2, _ = get_data_loaders(str(tmp_path / "train.parquet"), str(tmp_path / "val.parquet"), str(tmp_path / "img"), str(tmp_path / "img"),
                              batch_size=2, is_test=True, device="cpu", res=32, mosaic={}, mixup={"close_epochs": 1})
    tr2.set_epoch(1, 2)
    assert tr2.transform.mosaic_on is True and tr2.transform.mixup_on is False and tr2.transform.affine_on is False


def test_c5_header_and_library_carry_the_entry_points():
    import ctypes
    from src.hipops import lib
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    block = next(b for b in text.split("/* ---- ") if b.startswith("on-device input pipeline"))
    protos = lib.parse_header(os.path.join(ROOT, "include", "yolo_hip.h"))
    assert len(protos["yolo_mix_bytes"][1]) == 0
    assert protos["yolo_mix_fill"][2] == ["table_host", "index", "partner", "r", "N"]
    assert protos["yolo_image_prep_mixup"][2][:11] == ["src", "tiles_dev", "table_dev", "affine_dev", "mix_dev", "N", "S", "fill", "jitter", "stage", "stage2"]
    assert len(protos["yolo_image_prep_mixup"][1]) == 21
    so = ctypes.CDLL(lib.SO_PATH)
    for name in ("yolo_mix_bytes", "yolo_mix_fill", "yolo_image_prep_mixup"):
        assert name in block and hasattr(so, name), name
    assert "floor((r * a + (1.0f - r) * b) + 0.5f)" in block and "no reference counterpart" in block.split("mixup")[1][:200]
    # the parent's three entry points are declared as they were
    assert len(protos["yolo_image_prep"][1]) == 16 and len(protos["yolo_image_prep_mosaic"][1]) == 18 and len(protos["yolo_image_prep_affine"][1]) == 20
    mb = lib.query("yolo_mix_bytes")
    assert mb == 8
    host = torch.zeros(3 * mb, dtype=torch.uint8)
    assert lib.query("yolo_mix_fill", host.data_ptr(), 1, 2, 0.3, 3) == 0
    assert host[mb:mb + 4].view(torch.int32).tolist() == [2] and host[mb + 4:2 * mb].view(torch.float32).tolist() == [float(np.float32(0.3))]
    assert int(host[:mb].sum()) == 0 and int(host[2 * mb:].sum()) == 0
    for r in (0.0, 1.0):
        assert lib.query("yolo_mix_fill", host.data_ptr(), 0, 0, r, 3) == 0
    host.zero_()
    for index, partner, r, n in ((0, 1, float("nan"), 3), (0, 1, -0.1, 3), (0, 1, 1.5, 3), (0, 1, float("inf"), 3), (0, 3, 0.5, 3), (0, -1, 0.5, 3),
                                 (-1, 1, 0.5, 3), (0, 0, 0.5, 0)):
        assert lib.query("yolo_mix_fill", host.data_ptr() + mb, index, partner, r, n) == 1001, (index, partner, r, n)
    assert int(host.sum()) == 0                         # a refused record writes nothing
    # the real leaf refuses a wrong number of records before it touches the device
    recs = [(0, 2, 2, False, (), (1.0, 1.0, 1.0, 0.0))] * 3
    ident = [(1.0, 0.0, 0.0, 0.0, 1.0, 0.0)] * 3
    for tiles, affine, mix in ((None, None, [(0, 1.0)] * 2), (None, ident[:2], [(0, 1.0)] * 3), ([None] * 4, None, [(0, 1.0)] * 3)):
        with pytest.raises(ValueError, match="image_prep_mixup: 3 records need"):
            REAL_MIXUP(torch.zeros(12, dtype=torch.uint8), recs, tiles, affine, mix, 8, 114, False, torch.float32, (0.0,) * 3, (1.0,) * 3)
