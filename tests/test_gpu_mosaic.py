"""-m gpu: the mosaic of the on-device input pipeline (csrc/image_prep.hip::k_mosaic through ops.image_prep_mosaic and
src/data/transforms.py::BatchTransform(mosaic=...)) against tests/mosaic_ref.py.

The contract for the resized pixels is the input pipeline's (tests/test_gpu_input_pipeline.py): both sides quantise to uint8
levels after the resize and after every colour op, the device sums the taps of a pixel in another order than the separable
reference, so >= 99.5 % of ALL elements of the batch agree exactly and none is more than 3 levels off after the resize alone,
>= 97 % and 6 levels after the four colour ops.  What the mosaic adds is exact: which pixels are fill, their value, and -- for
a record that describes a plain resize -- every bit of the plain transform's output.

Measured on an MI355X with these inputs (each test prints its figures): G2 99.994 % exact and at most 1 level after the resize
alone, 99.73 % and 3 levels after the four colour ops; G3 (S = 64, sampled records) 99.997 % and 1 level.  Stage by stage, with
nothing propagating, the mosaic's tile pixels are held to the resize's sets of allowed levels in tests/test_gpu_image.py."""
import os

import numpy as np
import pytest
import torch

import mosaic_ref
from oracle import image_prep as oip

pytestmark = pytest.mark.gpu
SIZES = [(17, 301), (64, 64), (333, 500), (200, 1200), (48, 40), (480, 640)]
ORDERS = [(0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2), (2, 0, 3, 1), (0, 2, 1, 3), (3, 0, 1, 2), (1, 0, 2, 3), (2, 3, 0, 1)]
NO_JITTER = (1.0, 1.0, 1.0, 0.0)


def _images(seed, sizes):
    rng = np.random.default_rng(seed)
    out = []
    for h, w in sizes:
        # smooth content + noise: like a photograph, most pixels are not on a rounding boundary after resampling
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([127 + 100 * np.sin(xx / (7.0 + c) + yy / 13.0) for c in range(3)], -1)
        out.append(torch.from_numpy(np.clip(base + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)))
    return out


def _jitter(i):
    return ORDERS[i % 8], (0.8 + 0.05 * i, 1.2 - 0.04 * i, 0.85 + 0.04 * i, -0.1 + 0.028 * i)


def _compare(got, want, what, exact_min=0.995, levels=3):
    got, want = got.float().cpu(), want.float()
    d = (got - want).abs()
    exact = float((d < 1e-5).float().mean())
    lim = (levels + 0.05) / 255 / 0.224
    print(f"\n[mosaic] {what}: {exact:.4%} exact, max {float(d.max()):.4f} (limit {lim:.4f})")
    assert exact >= exact_min and float(d.max()) <= lim, f"{what}: {exact:.4%} exact, max {float(d.max()):.4f} (limit {lim:.4f})"


@pytest.fixture(scope="module")
def sources():
    return _images(21, SIZES)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("size", [64, 96])
def test_g1_plain_records_reproduce_the_plain_transform_bit_for_bit(sources, size, dtype):
    from src.hipops import ops
    flat = torch.cat([t.reshape(-1) for t in sources]).cuda()
    for jitter in (False, True):
        recs, tiles, off = [], [], 0
        for i, t in enumerate(sources):
            h, w = int(t.shape[0]), int(t.shape[1])
            order, fac = _jitter(i) if jitter else ((), NO_JITTER)
            recs.append((off, h, w, i % 2 == 0, order, fac))
            tiles.append((size, size, [(off, h, w, i % 2 == 0, size, size, 0, 0), None, None, None]))
            off += h * w * 3
        want = ops.image_prep(flat, recs, size, jitter, dtype, oip.MEAN, oip.STD)
        got = ops.image_prep_mosaic(flat, recs, tiles, size, 114, jitter, dtype, oip.MEAN, oip.STD)
        assert got.dtype == dtype and got.shape == (len(sources), 3, size, size)
        assert torch.equal(got, want), f"S={size} {dtype} jitter={jitter}: {int((got != want).sum())} elements differ"
    # ... and through the transform: a mosaic-enabled BatchTransform whose outputs are all plain
    from src.data.transforms import BatchTransform
    params = [(i % 2 == 0, *_jitter(i)) for i in range(len(sources))]
    plain, _ = BatchTransform(True, size, "cuda", dtype)(sources, params=params)
    same, _ = BatchTransform(True, size, "cuda", dtype, mosaic={})(sources, params=params, mosaic=[None] * len(sources))
    assert torch.equal(plain, same)


def _record(cx, cy, tiles):
    """tiles: four (source, flip, tw, th); every tile touches the centre with one corner."""
    return {"cx": cx, "cy": cy, "tiles": [(s, f, tw, th, cx if k & 1 else cx - tw, cy if k & 2 else cy - th)
                                          for k, (s, f, tw, th) in enumerate(tiles)]}


S2 = 96
# sources: 0 (17, 301), 1 (64, 64), 2 (333, 500), 3 (200, 1200), 4 (48, 40), 5 (480, 640); tile 0 of output i is image i
RECORDS = [
    # centre at (S//4, S//4): tile 0 flipped, wider than its 24-wide quadrant, shorter than it (fill above); tile 1 clipped below
    # by the 24-row quadrant; tile 2 smaller than its quadrant; tile 3 the image itself again, its 17 rows upscaled to 30
    _record(24, 24, [(0, True, 40, 11), (1, False, 64, 64), (2, False, 20, 13), (0, False, 120, 30)]),
    # centre at (S - S//4, S - S//4): tile 0 upscaled 64 -> 96 and clipped on both axes; source 3 twice, once as a 1 x 1 tile
    _record(72, 72, [(1, False, 96, 96), (3, True, 24, 4), (3, False, 1, 1), (4, True, 20, 24)]),
    # an odd interior centre, quadrant edges in the middle of a wave: tiles 0 and 3 (the image itself) clipped on both axes
    _record(37, 53, [(2, True, 77, 51), (5, False, 59, 44), (4, False, 33, 40), (2, False, 96, 64)]),
    None,                                                                    # a plain output inside the mosaic batch
    _record(24, 72, [(4, False, 40, 48), (5, True, 72, 54), (1, False, 24, 24), (1, True, 100, 100)]),
    # tile 2 starts left of the canvas (x0 = -24)
    _record(72, 24, [(5, True, 64, 48), (0, False, 24, 2), (3, False, 96, 16), (2, True, 30, 20)]),
]
PLAIN_FLIP = True                                                            # of output 3


def _reference(sources, jitter):
    imgs = [t.numpy() for t in sources]
    outs, masks = [], []
    for i, rec in enumerate(RECORDS):
        rec = rec if rec is not None else mosaic_ref.plain_record(i, PLAIN_FLIP, S2)
        canvas, is_fill = mosaic_ref.mosaic_canvas(imgs, rec, S2, 114)
        order, fac = _jitter(i) if jitter else ((), NO_JITTER)
        outs.append(mosaic_ref.finish(canvas, order, fac))
        masks.append(torch.from_numpy(is_fill))
    return torch.stack(outs), torch.stack(masks)


@pytest.fixture(scope="module")
def reference(sources):
    return {False: _reference(sources, False), True: _reference(sources, True)}


def test_g2_fixed_records_against_the_reference(sources, reference):
    from src.data.transforms import BatchTransform
    tr = BatchTransform(True, S2, "cuda", mosaic={})
    params = [(PLAIN_FLIP if RECORDS[i] is None else False, (), NO_JITTER) for i in range(len(sources))]
    got, _ = tr(sources, params=params, mosaic=RECORDS)
    got = got.cpu()
    want, is_fill = reference[False]
    assert got.shape == (6, 3, S2, S2) and got.dtype == torch.float32
    # every kind of clipping is present: fill in five outputs, none in the plain one
    assert all(bool(is_fill[i].any()) for i in (0, 1, 2, 4, 5)) and not bool(is_fill[3].any())
    # the fill pixels are those that follow the fill level: the same batch with another level differs exactly there
    other, _ = BatchTransform(True, S2, "cuda", mosaic={"fill": 113})(sources, params=params, mosaic=RECORDS)
    dev_fill = (other.cpu() != got).any(1)
    assert torch.equal(dev_fill, is_fill), f"{int((dev_fill != is_fill).sum())} pixels are fill on one side only"
    assert torch.equal((other.cpu() != got).all(1), is_fill)
    fv = mosaic_ref.fill_value(114).reshape(1, 3, 1, 1).expand_as(got)
    m = is_fill[:, None].expand_as(got)
    assert torch.equal(got[m], fv[m])
    _compare(got, want, "S=96, 6 outputs, resize only")
    # the four colour ops on the finished canvas, one (order, factors) per output
    params = [(p[0], *_jitter(i)) for i, p in enumerate(params)]
    got, _ = tr(sources, params=params, mosaic=RECORDS)
    _compare(got, reference[True][0], "S=96, 6 outputs, four colour ops", 0.97, 6)


def _targets(seed, sizes):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, (h, w) in enumerate(sizes):
        m = 0 if i == 4 else 3 + i
        xy = torch.rand(m, 2, generator=g) * torch.tensor([w * 0.7, h * 0.7])
        wh = torch.rand(m, 2, generator=g) * torch.tensor([w * 0.3, h * 0.3]) + torch.tensor([w * 0.02, h * 0.02])
        out.append({"boxes": torch.cat([xy, wh], 1), "labels": torch.randint(0, 80, (m, 1), generator=g).float(), "name": f"im{i}"})
    return out


def test_g3_sampled_path_end_to_end(sources):
    from src.data.transforms import BatchTransform, mosaic_geometry
    S = 64
    imgs = sources + _images(22, [(100, 80), (64, 64)])
    sizes = [tuple(int(v) for v in t.shape[:2]) for t in imgs]
    tg = _targets(5, sizes)
    cfg = {"p": 0.75, "gain": [0.4, 1.6]}
    tr = BatchTransform(True, S, "cuda", mosaic=cfg)
    torch.manual_seed(13)
    params = [tr.sample() for _ in imgs]
    draws = tr.sample_mosaic(len(imgs))
    assert any(d is None for d in draws) and sum(d is not None for d in draws) >= 4
    torch.manual_seed(13)
    batch, out = tr(imgs, tg)
    assert batch.shape == (8, 3, S, S) and batch.dtype == torch.float32 and bool(torch.isfinite(batch).all())
    np_imgs = [t.numpy() for t in imgs]
    want = []
    for i, d in enumerate(draws):
        flip, order, fac = params[i]
        if d is None:
            ref = torch.cat([oip.transform_boxes(tg[i]["boxes"], sizes[i][1], sizes[i][0], S, flip), tg[i]["labels"]], 1)
            rec = mosaic_ref.plain_record(i, flip, S)
        else:
            rec = mosaic_geometry(d, i, sizes, flip, S)
            ref = mosaic_ref.mosaic_boxes(rec, tg, sizes, S)
        b = out[i]["boxes"]
        assert b.shape == ref.shape and b.dtype == torch.float32 and torch.allclose(b, ref, rtol=0, atol=1e-4), (i, b, ref)
        assert out[i]["name"] == f"im{i}" and "labels" not in out[i]
        if d is not None and b.numel():
            assert float(b[:, :2].min()) >= 0 and float((b[:, 0] + b[:, 2]).max()) <= S + 1e-3 and float((b[:, 1] + b[:, 3]).max()) <= S + 1e-3
            assert float(b[:, 2:4].min()) >= 2.0
        want.append(mosaic_ref.mosaic_image(np_imgs, rec, S, 114, order, fac))
    assert sum(o["boxes"].shape[0] for i, o in enumerate(out) if draws[i] is not None) > 0
    _compare(batch, torch.stack(want), "S=64, 8 sampled outputs, four colour ops", 0.97, 6)
    torch.manual_seed(13)
    again, out2 = tr(imgs, tg)
    assert torch.equal(again, batch) and all(torch.equal(a["boxes"], b["boxes"]) for a, b in zip(out, out2))
    bf, _ = BatchTransform(True, S, "cuda", torch.bfloat16, mosaic=cfg)(imgs, tg, params=params, mosaic=draws)
    assert bf.dtype == torch.bfloat16 and torch.equal(bf, batch.to(torch.bfloat16))


def test_g4_one_captured_training_run_with_the_mosaic_closed_for_the_last_epoch(tmp_path, monkeypatch):
    """Preset n on a tiny parquet dataset, two epochs of two batches, `mosaic: {p: 1, close_epochs: 1}`.  The images are
    transformed to 160 x 160, the size at which this suite already runs the captured step (test_gpu_train_loop.py).  Every
    source image carries 120 boxes -- a plain batch of four fills 480 of the captured step's 512 target slots -- so a mosaic
    collects up to 480 on its own and stays on the captured step only because it is cut to max_boxes = 128."""
    import pandas as pd
    from PIL import Image
    from src.data.data_loader import get_data_loaders
    from src.hipops import ops
    from src.model.losses import YoloDFLQFLoss
    from src.model.model_builder import Model
    from src.training import train_model as tm
    from src.training.utils_train import get_optimizer
    rng = np.random.default_rng(6)
    os.makedirs(tmp_path / "img")
    rows = []
    for i, (h, w) in enumerate(((120, 160), (200, 150), (160, 160), (90, 240), (128, 96), (180, 200), (150, 100), (64, 220))):
        Image.fromarray(_images(30 + i, [(h, w)])[0].numpy()).save(tmp_path / "img" / f"{i}.png")
        xy = rng.uniform(0, 0.75, (120, 2)) * (w, h)
        wh = rng.uniform(0.08, 0.25, (120, 2)) * (w, h)
        rows.append({"file_name": f"{i}.png", "bbox": np.concatenate([xy, wh], 1).astype(np.float32).tolist(),
                     "category_id": rng.integers(0, 80, 120).astype(np.float32).tolist(), "name": f"im{i}"})
    pd.DataFrame(rows).to_parquet(tmp_path / "train.parquet")
    pd.DataFrame(rows[:4]).to_parquet(tmp_path / "val.parquet")
    tr, va = get_data_loaders(str(tmp_path / "train.parquet"), str(tmp_path / "val.parquet"), str(tmp_path / "img"), str(tmp_path / "img"),
                              batch_size=4, is_test=True, device="cuda", num_classes=80, res=160, mosaic={"p": 1, "close_epochs": 1})
    assert len(tr) == 2
    torch.manual_seed(0)
    model = Model(csp=[False, True], depth=[1] * 6, width=[3, 16, 32, 64, 128, 256], num_classes=80).to("cuda")
    opt, sched = get_optimizer(model, lr=1e-4, weight_decay=1e-4, patience=3, factor=0.5)
    steps, mosaic_calls = [], []
    orig_step, orig_prep = tm.CapturedTraining.step, ops.image_prep_mosaic

    def spy_step(self, images, boxes):
        ld = orig_step(self, images, boxes)
        steps.append((self.captured, self.dirty, max(int(b.shape[0]) for b in boxes), ld))
        return ld

    def spy_prep(*a):
        mosaic_calls.append(tr.transform.mosaic_on)
        return orig_prep(*a)
    monkeypatch.setattr(tm.CapturedTraining, "step", spy_step)
    monkeypatch.setattr(ops, "image_prep_mosaic", spy_prep)
    tm.train(model=model, train_loader=tr, val_loader=va, optimizer=opt, scheduler=sched, criterion=YoloDFLQFLoss(num_classes=80),
             initial_epoch=0, num_epochs=2, device=0, num_classes=80, rank=0, checkpoint_dir=str(tmp_path), distributed_mode="ddp",
             precision="bfloat16", conf_threshold=0.01)
    assert len(steps) == 4 and all(ld is not None for *_, ld in steps), "the training batches did not go through CapturedTraining"
    assert mosaic_calls == [True, True] and tr.transform.mosaic_on is False      # two mosaic batches, both in the first epoch
    assert all(captured and not dirty for captured, dirty, _, _ in steps), [s[:3] for s in steps]    # nothing fell off the capture
    # the fullest image of a batch: cut to max_boxes in the mosaic epoch, all 120 boxes in the plain one
    assert [n for _, _, n, _ in steps] == [128, 128, 120, 120], [s[2] for s in steps]
    for *_, ld in steps:
        assert all(np.isfinite(ld[k]) for k in ("total_loss", "box_loss", "cls_loss")), ld
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
