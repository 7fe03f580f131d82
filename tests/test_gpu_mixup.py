"""-m gpu: the mixup of the on-device input pipeline (csrc/image_prep.hip::k_mixup through ops.image_prep_mixup and
src/data/transforms.py::BatchTransform(mixup=...)) against tests/mixup_ref.py.

Device levels are read as tests/test_gpu_affine.py reads them: jitter off, mean 0, std 1, fp32, so round(out * 255) IS the staging
buffer.  The canvases the mix read are the device's own unmixed outputs of the same records -- the same launches write them -- so
nothing propagates from the resize, the mosaic or the warp into the mix's check, and the mix stage is held to EXACT equality with
`mix_f32`: no tolerance, no cap.  N = 3 sources of different sizes; S = 96 (vector path: 1728 vectors per image, a partial last
workgroup), S = 20 (vector path: 75 vectors, one partial workgroup), S = 33 (scalar path: odd B, unaligned image bases).
G1 identity records bit for bit; G2 exact equality on all four routes; G3 the arithmetic over every pair of levels; G4 the
sampled path end to end; G5 one captured training run."""
import os
import time

import numpy as np
import pytest
import torch

import affine_ref as ar
import mixup_ref as mr
import mosaic_ref
import strict_affine as sa
import strict_image as si
from oracle import image_prep as oip

pytestmark = pytest.mark.gpu
F32, BF = torch.float32, torch.bfloat16
NO_JITTER = (1.0, 1.0, 1.0, 0.0)
ZERO, ONE = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
C255 = np.float32(1) / np.float32(255)
SIZES = (96, 20, 33)
SOURCES = [(37, 23), (120, 161), (96, 96)]                     # upscaled, downscaled (odd sizes), and a canvas size itself
ORDERS = [(0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2)]
FACTORS = [(0.8137, 1.1871, 0.9329, -0.0871), (1.1, 0.9, 1.15, 0.06), (0.95, 1.05, 0.85, 0.1)]
FILL = 114
# a mutual pair beside an unmixed output; a chain 0 -> 1 -> 2 -> 0; two outputs sharing one partner beside an unmixed one (which
# is that partner); a mutual pair whose third output reads one of them.  The ratios are mixup_ref.RATIOS, each used at least once
RECORDS = {"mutual": [(1, 0.3), (0, 0.7), None], "chain": [(1, 0.4719), (2, 0.25), (0, 2.0 ** -10)], "shared": [(2, 0.5), (2, 0.0), None],
           "ends": [(2, 1.0), (0, 0.7), (1, 0.3)]}


def ops():
    from src.hipops import ops as o
    return o


@pytest.fixture(autouse=True, scope="module")
def _print_time():
    t0 = time.time()
    yield
    print(f"\n[mixup] wall time of tests/test_gpu_mixup.py: {time.time() - t0:.1f} s")


@pytest.fixture(scope="module")
def batch():
    """-> (flat device buffer, the three records without jitter, the images): image 0 noise, 1 and 2 photograph-like"""
    images = [si.noise(*SOURCES[0], 500)] + si.smooth_images(51, SOURCES[1:])
    offs = np.concatenate([[0], np.cumsum([im.size for im in images])])
    flat = torch.cat([torch.from_numpy(np.ascontiguousarray(im)).reshape(-1) for im in images]).cuda()
    recs = [(int(offs[i]), im.shape[0], im.shape[1], i == 1, (), NO_JITTER) for i, im in enumerate(images)]
    return flat, recs, images


def _levels(out):
    """fp32 (N, 3, S, S) written with mean 0, std 1 -> the uint8 levels (N, S, S, 3) behind it, asserting out == level * (1/255.f)"""
    out = out.float().cpu().numpy()
    lv = np.round(out.astype(np.float64) * 255.0)
    assert lv.min() >= 0 and lv.max() <= 255 and np.array_equal(lv.astype(np.float32) * C255, out), "the output is not level * (1/255.f)"
    return lv.transpose(0, 2, 3, 1)


def _tiles(S, recs):
    """a real mosaic (tests/test_gpu_affine.py's): output i has its centre off the middle and four tiles (sources i, i + 1, i + 2, i)
    touching it, tile 0 larger than its quadrant, tile 3 smaller (fill shows)"""
    out = []
    for i in range(len(recs)):
        cx, cy = S // 3 + 5 * i, S // 2 - 3 * i
        quad = []
        for k, (tw, th) in enumerate(((cx + 7, cy - 2), (S - cx, cy), (cx, S - cy + 4), (S // 4, S // 5))):
            off, h, w, flip = recs[(i + k) % len(recs)][:4]
            quad.append((off, h, w, flip ^ (k == 2), tw, th, cx if k & 1 else cx - tw, cy if k & 2 else cy - th))
        out.append((cx, cy, quad))
    return out


def _warps(S, n=3):
    from src.data.transforms import affine_matrix, affine_record
    return [affine_record(affine_matrix(sa.GENERAL[name], S)) for name in ("rot10", "combined", "gain0.5")][:n]


def _jittered(recs):
    return [(off, h, w, fl, ORDERS[i], FACTORS[i]) for i, (off, h, w, fl, _, _) in enumerate(recs)]


def _parent(flat, recs, tiles, affine, S, jitter, dtype, mean, std):
    """the parent's leaf of a route: the unmixed outputs"""
    if affine is not None:
        return ops().image_prep_affine(flat, recs, tiles, affine, S, FILL, jitter, dtype, mean, std)
    if tiles is not None:
        return ops().image_prep_mosaic(flat, recs, tiles, S, FILL, jitter, dtype, mean, std)
    return ops().image_prep(flat, recs, S, jitter, dtype, mean, std)


def _routes(S, recs):
    n = len(recs)
    return {"plain": (None, None), "mosaic": (_tiles(S, recs), None), "warp": (None, _warps(S, n)), "mosaic+warp": (_tiles(S, recs), _warps(S, n))}


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("S", SIZES)
def test_g1_identity_records_reproduce_the_three_parent_transforms_bit_for_bit(batch, S, dtype):
    flat, recs, _ = batch
    for n in (3, 1):
        for jitter in (False, True):
            r = (_jittered(recs) if jitter else recs)[:n]
            for route, (tiles, affine) in _routes(S, r).items():
                want = _parent(flat, r, tiles, affine, S, jitter, dtype, oip.MEAN, oip.STD)
                got = ops().image_prep_mixup(flat, r, tiles, affine, [(i, 1.0) for i in range(n)], S, FILL, jitter, dtype, oip.MEAN, oip.STD)
                assert got.dtype == dtype and got.shape == (n, 3, S, S)
                assert torch.equal(got, want), f"{route} N={n} S={S} {dtype} jitter={jitter}: {int((got != want).sum())} elements differ"
                # the ratio of a record without a partner is not read
                got = ops().image_prep_mixup(flat, r, tiles, affine, [(i, 0.25) for i in range(n)], S, FILL, jitter, dtype, oip.MEAN, oip.STD)
                assert torch.equal(got, want), f"{route} N={n} S={S} {dtype} jitter={jitter}, r = 0.25 without a partner"
    # ... and through the transform: None for every output is the parent's leaf, and r = 1 with a partner is the own canvas
    from src.data.transforms import BatchTransform
    imgs = [torch.from_numpy(im) for im in batch[2]]
    params = [(i == 1, ORDERS[i], FACTORS[i]) for i in range(3)]
    plain, _ = BatchTransform(True, S, "cuda", dtype)(imgs, params=params)
    tr = BatchTransform(True, S, "cuda", dtype, mixup={})
    assert torch.equal(tr(imgs, params=params, mixup=[None] * 3)[0], plain)
    assert torch.equal(tr(imgs, params=params, mixup=[(1, 1.0), None, (0, 1.0)])[0], plain)
    with pytest.raises(ValueError, match="image_prep_mixup: 3 records need"):
        ops().image_prep_mixup(flat, recs, None, None, [(0, 1.0)] * 2, S, FILL, False, dtype, oip.MEAN, oip.STD)
    with pytest.raises(RuntimeError, match="yolo_mix_fill"):
        ops().image_prep_mixup(flat, recs, None, None, [(0, 1.0), (3, 0.5), (2, 1.0)], S, FILL, False, dtype, oip.MEAN, oip.STD)


@pytest.mark.parametrize("route", ["plain", "mosaic", "warp", "mosaic+warp"])
@pytest.mark.parametrize("S", SIZES)
def test_g2_every_route_equals_mix_f32_exactly(batch, S, route):
    flat, recs, _ = batch
    tiles, affine = _routes(S, recs)[route]
    canv = _levels(_parent(flat, recs, tiles, affine, S, False, F32, ZERO, ONE))          # the device's own unmixed canvases
    used = set()
    for name, mix in RECORDS.items():
        used |= {m[1] for m in mix if m is not None}
        got = _levels(ops().image_prep_mixup(flat, recs, tiles, affine, [(i, 1.0) if m is None else m for i, m in enumerate(mix)], S, FILL,
                                             False, F32, ZERO, ONE))
        want = mr.mix_f32(canv, mix)
        for i, m in enumerate(mix):
            bad = int((got[i] != want[i]).sum())
            print(f"\n[mixup] S={S} {route} {name} output {i} {m}: {bad} of {want[i].size} elements differ from mix_f32", end="")
            assert bad == 0, f"S={S} {route} {name} output {i} {m}: {bad} elements differ"
            if m is None:
                assert np.array_equal(got[i], canv[i])
        if route in ("plain", "mosaic"):
            # the other buffer routing: an identity warp in front makes the mix read stage2 and write stage -- the same bytes
            other = _levels(ops().image_prep_mixup(flat, recs, tiles, [ar.IDENTITY] * 3, [(i, 1.0) if m is None else m for i, m in enumerate(mix)],
                                                   S, FILL, False, F32, ZERO, ONE))
            assert np.array_equal(other, got), f"S={S} {route} {name}: the result depends on which stage the mix wrote"
    assert used == set(mr.RATIOS)
    # the colour chain runs on the mixed canvas with the order and factors of output i: bf16 is the rounded fp32 output
    mix = [(1, 0.3), (2, 0.7), (0, 0.4719)]
    a = ops().image_prep_mixup(flat, _jittered(recs), tiles, affine, mix, S, FILL, True, F32, oip.MEAN, oip.STD)
    b = ops().image_prep_mixup(flat, _jittered(recs), tiles, affine, mix, S, FILL, True, BF, oip.MEAN, oip.STD)
    assert torch.equal(b, a.to(BF)) and bool(torch.isfinite(a).all())


def test_g3_the_arithmetic_over_every_pair_of_levels():
    """S = 148: 3 * 148^2 = 65 712 >= 65 536 elements on the vector path.  Two S x S sources (the resize's exact class: a source of
    the canvas's size is copied) hold every pair (a, b) of levels at the same element; the outputs are exact for every ratio."""
    S = 148
    k = np.arange(3 * S * S)
    src = [(k % 256).astype(np.uint8).reshape(S, S, 3), ((k // 256) % 256).astype(np.uint8).reshape(S, S, 3)]
    flat = torch.cat([torch.from_numpy(s).reshape(-1) for s in src]).cuda()
    recs = [(0, S, S, False, (), NO_JITTER), (3 * S * S, S, S, False, (), NO_JITTER)]
    canv = _levels(ops().image_prep(flat, recs, S, False, F32, ZERO, ONE))
    assert np.array_equal(canv[0], src[0]) and np.array_equal(canv[1], src[1])             # the exact class of the resize
    assert len(set(zip(canv[0].reshape(-1).tolist(), canv[1].reshape(-1).tolist()))) == 65536
    for r in mr.RATIOS:
        got = _levels(ops().image_prep_mixup(flat, recs, None, None, [(1, r), (0, r)], S, FILL, False, F32, ZERO, ONE))
        want = mr.mix_f32(canv, [(1, r), (0, r)])
        bad = int((got != want).sum())
        print(f"\n[mixup] every pair of levels, r = {r}: {bad} of {want.size} elements differ from mix_f32", end="")
        assert bad == 0
        assert np.array_equal(got[0], mr.blend_f32(canv[0], canv[1], r)) and np.array_equal(got[1], mr.blend_f32(canv[1], canv[0], r))
    assert np.array_equal(_levels(ops().image_prep_mixup(flat, recs, None, None, [(1, 1.0), (0, 0.0)], S, FILL, False, F32, ZERO, ONE)),
                          np.stack([canv[0], canv[0]]))


def _targets(seed, sizes):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, (h, w) in enumerate(sizes):
        m = 0 if i == 4 else 3 + i
        xy = torch.rand(m, 2, generator=g) * torch.tensor([w * 0.7, h * 0.7])
        wh = torch.rand(m, 2, generator=g) * torch.tensor([w * 0.3, h * 0.3]) + torch.tensor([w * 0.02, h * 0.02])
        out.append({"boxes": torch.cat([xy, wh], 1), "labels": torch.randint(0, 80, (m, 1), generator=g).float(), "name": f"im{i}"})
    return out


def test_g4_sampled_path_end_to_end():
    """mosaic -> warp -> mixup -> four colour ops, sampled under a fixed seed, against mosaic_ref -> affine_ref -> mix_f32 -> finish
    under the input pipeline's contract for the colour stages (tests/test_gpu_affine.py G4: >= 97 % of all elements exact, none more
    than 6 levels off); the boxes are the concatenation of affine_boxes(mosaic_boxes(...)) of the output and of its partner."""
    from src.data.transforms import BatchTransform, affine_matrix, affine_record, mosaic_geometry
    S = 64
    sizes = [(17, 301), (64, 64), (333, 500), (200, 1200), (48, 40), (480, 640), (100, 80), (64, 64)]
    imgs = [torch.from_numpy(im) for im in si.smooth_images(21, sizes)]
    tg = _targets(5, sizes)
    mcfg, acfg = {"p": 0.75, "gain": [0.4, 1.6]}, {"degrees": 20.0, "translate": 0.15, "scale": 0.4, "shear": 4.0}
    xcfg = {"p": 0.5, "alpha": 8.0}
    tr = BatchTransform(True, S, "cuda", mosaic=mcfg, affine=acfg, mixup=xcfg)
    torch.manual_seed(13)
    params = [tr.sample() for _ in imgs]
    mdraws, adraws, xdraws = tr.sample_mosaic(len(imgs)), tr.sample_affine(len(imgs)), tr.sample_mixup(len(imgs))
    assert any(d is None for d in mdraws) and sum(d is not None for d in mdraws) >= 4
    assert sum(x is not None for x in xdraws) >= 2 and any(x is None for x in xdraws), xdraws
    torch.manual_seed(13)
    got, out = tr(imgs, tg)
    assert got.shape == (8, 3, S, S) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    np_imgs = [t.numpy() for t in imgs]
    canv, unmixed = [], []
    for i, (d, a) in enumerate(zip(mdraws, adraws)):
        flip = params[i][0]
        if d is None:
            ref = torch.cat([oip.transform_boxes(tg[i]["boxes"], sizes[i][1], sizes[i][0], S, flip), tg[i]["labels"]], 1)
            rec = mosaic_ref.plain_record(i, flip, S)
        else:
            rec = mosaic_geometry(d, i, sizes, flip, S)
            ref = mosaic_ref.mosaic_boxes(rec, tg, sizes, S)
        m = affine_matrix(a, S)
        unmixed.append(ar.affine_boxes(m, ref, S))
        canv.append(ar.warp_f32(mosaic_ref.mosaic_canvas(np_imgs, rec, S, 114)[0], affine_record(m), 114))
    mixed = mr.mix_f32(np.stack(canv), xdraws)
    want = []
    for i, x in enumerate(xdraws):
        ref = unmixed[i] if x is None else mr.mixup_boxes(unmixed[i], unmixed[x[0]])
        b = out[i]["boxes"]
        # the tolerance tests/test_gpu_affine.py G4 derives for a warped mosaic's boxes; the mixup moves no box
        assert b.shape == ref.shape and b.dtype == torch.float32 and torch.allclose(b, ref, rtol=0, atol=3.5e-4), (i, b, ref)
        assert out[i]["name"] == f"im{i}" and "labels" not in out[i]
        want.append(mosaic_ref.finish(mixed[i], params[i][1], params[i][2]))
    assert sum(o["boxes"].shape[0] for o in out) > 0
    d = (got.cpu() - torch.stack(want)).abs()
    exact, lim = float((d < 1e-5).float().mean()), 6.05 / 255 / 0.224
    print(f"\n[mixup] S=64, 8 sampled outputs, mosaic + warp + mixup + four colour ops: {exact:.4%} exact, max {float(d.max()):.4f} (limit {lim:.4f})")
    assert exact >= 0.97 and float(d.max()) <= lim
    torch.manual_seed(13)
    again, out2 = tr(imgs, tg)
    assert torch.equal(again, got) and all(torch.equal(a["boxes"], b["boxes"]) for a, b in zip(out, out2))
    bf, _ = BatchTransform(True, S, "cuda", BF, mosaic=mcfg, affine=acfg, mixup=xcfg)(imgs, tg, params=params, mosaic=mdraws, affine=adraws,
                                                                                   mixup=xdraws)
    assert bf.dtype == BF and torch.equal(bf, got.to(BF))


class _Spy:
    """stands where the loader's transform stood: forwards everything, and in an epoch with all three switches off runs a transform
    built WITHOUT any of the keys on the same inputs from the same RNG state and holds the two outputs against each other"""

    def __init__(self, inner, plain):
        self.__dict__.update(inner=inner, plain=plain, log=[])

    def __getattr__(self, name):
        return getattr(self.__dict__["inner"], name)

    def __setattr__(self, name, value):
        setattr(self.__dict__["inner"], name, value)

    def __call__(self, images, targets):
        inner, plain = self.__dict__["inner"], self.__dict__["plain"]
        state = torch.get_rng_state()
        batch, out = inner(images, targets)
        same = None
        if not inner.mosaic_on and not inner.affine_on and not inner.mixup_on:
            after = torch.get_rng_state()
            torch.set_rng_state(state)
            want, want_t = plain(images, targets)
            same = torch.equal(batch, want) and torch.equal(torch.get_rng_state(), after) and \
                all(torch.equal(a["boxes"], b["boxes"]) for a, b in zip(out, want_t))
        self.__dict__["log"].append((inner.mosaic_on, inner.affine_on, inner.mixup_on, same, max(int(t["boxes"].shape[0]) for t in out)))
        return batch, out


def test_g5_one_captured_training_run_with_all_three_closed_for_the_last_epoch(tmp_path, monkeypatch):
    """Preset n on a tiny parquet dataset, two epochs of two batches at 160 x 160, 120 boxes per source image, `mosaic: {p: 1,
    close_epochs: 1}`, `affine: {degrees: 10, close_epochs: 1}` and `mixup: {p: 1, close_epochs: 1}`: every batch goes through the
    captured step (a mixed output never carries more than max_boxes = 128), the loss is finite, and the last epoch is the transform
    without any of the keys."""
    import pandas as pd
    from PIL import Image
    from src.data.data_loader import get_data_loaders
    from src.data.transforms import get_train_transforms
    from src.model.losses import YoloDFLQFLoss
    from src.model.model_builder import Model
    from src.training import train_model as tm
    from src.training.utils_train import get_optimizer
    rng = np.random.default_rng(6)
    os.makedirs(tmp_path / "img")
    rows = []
    for i, (h, w) in enumerate(((120, 160), (200, 150), (160, 160), (90, 240), (128, 96), (180, 200), (150, 100), (64, 220))):
        Image.fromarray(si.smooth_images(30 + i, [(h, w)])[0]).save(tmp_path / "img" / f"{i}.png")
        xy = rng.uniform(0, 0.75, (120, 2)) * (w, h)
        wh = rng.uniform(0.08, 0.25, (120, 2)) * (w, h)
        rows.append({"file_name": f"{i}.png", "bbox": np.concatenate([xy, wh], 1).astype(np.float32).tolist(),
                     "category_id": rng.integers(0, 80, 120).astype(np.float32).tolist(), "name": f"im{i}"})
    pd.DataFrame(rows).to_parquet(tmp_path / "train.parquet")
    pd.DataFrame(rows[:4]).to_parquet(tmp_path / "val.parquet")
    tr, va = get_data_loaders(str(tmp_path / "train.parquet"), str(tmp_path / "val.parquet"), str(tmp_path / "img"), str(tmp_path / "img"),
                              batch_size=4, is_test=True, device="cuda", num_classes=80, res=160, mosaic={"p": 1, "close_epochs": 1},
                              affine={"degrees": 10.0, "close_epochs": 1}, mixup={"p": 1, "close_epochs": 1})
    assert len(tr) == 2
    spy = _Spy(tr.transform, get_train_transforms(160, "cuda"))
    tr.transform = spy
    torch.manual_seed(0)
    model = Model(csp=[False, True], depth=[1] * 6, width=[3, 16, 32, 64, 128, 256], num_classes=80).to("cuda")
    opt, sched = get_optimizer(model, lr=1e-4, weight_decay=1e-4, patience=3, factor=0.5)
    steps = []
    orig_step = tm.CapturedTraining.step

    def spy_step(self, images, boxes):
        ld = orig_step(self, images, boxes)
        steps.append((self.captured, self.dirty, max(int(b.shape[0]) for b in boxes), ld))
        return ld
    monkeypatch.setattr(tm.CapturedTraining, "step", spy_step)
    tm.train(model=model, train_loader=tr, val_loader=va, optimizer=opt, scheduler=sched, criterion=YoloDFLQFLoss(num_classes=80),
             initial_epoch=0, num_epochs=2, device=0, num_classes=80, rank=0, checkpoint_dir=str(tmp_path), distributed_mode="ddp",
             precision="bfloat16", conf_threshold=0.01)
    assert len(steps) == 4 and all(ld is not None for *_, ld in steps), "the training batches did not go through CapturedTraining"
    assert all(captured and not dirty for captured, dirty, _, _ in steps), [s[:3] for s in steps]    # no batch was stepped eagerly
    log = spy.__dict__["log"]
    assert [e[:4] for e in log] == [(True, True, True, None), (True, True, True, None), (False, False, False, True), (False, False, False, True)], log
    counts = [n for _, _, n, _ in steps]
    assert all(0 < n <= 128 for n in counts[:2]) and counts[2:] == [120, 120] and all(e[4] <= 128 for e in log), (counts, log)
    for *_, ld in steps:
        assert all(np.isfinite(ld[k]) for k in ("total_loss", "box_loss", "cls_loss")), ld
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
