"""-m gpu: the affine warp of the on-device input pipeline (csrc/image_prep.hip::k_affine through ops.image_prep_affine and
src/data/transforms.py::BatchTransform(affine=...)) against tests/strict_affine.py and tests/affine_ref.py.

Device levels are read as tests/test_gpu_image.py reads them: jitter off, mean 0, std 1, fp32, so round(out * 255) IS the staging
buffer.  The canvas the warp read is the device's own plain (or mosaic) output of the same records -- the same launch writes it
-- so nothing propagates from the resize into the warp's check.  S = 96 and S = 33 (odd: partial 32 x 8 workgroups on both axes),
N = 3 sources of different sizes.  G1 identity records bit for bit; G2 the exact class against index arithmetic; G3 general
records against the sets of allowed levels; G4 the sampled path end to end; G5 one captured training run."""
import os
import time

import numpy as np
import pytest
import torch

import affine_ref as ar
import mosaic_ref
import strict_affine as sa
import strict_image as si
from oracle import image_prep as oip

pytestmark = pytest.mark.gpu
F32, BF = torch.float32, torch.bfloat16
NO_JITTER = (1.0, 1.0, 1.0, 0.0)
ZERO, ONE = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
C255 = np.float32(1) / np.float32(255)
SOURCES = [(37, 23), (120, 161), (96, 96)]                     # upscaled, downscaled (odd sizes), and the canvas size itself
ORDERS = [(0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2)]
FACTORS = [(0.8137, 1.1871, 0.9329, -0.0871), (1.1, 0.9, 1.15, 0.06), (0.95, 1.05, 0.85, 0.1)]


def ops():
    from src.hipops import ops as o
    return o


@pytest.fixture(autouse=True, scope="module")
def _print_report():
    t0 = time.time()
    yield
    print("\n" + si.report() + f"\n[strict_affine] wall time of tests/test_gpu_affine.py: {time.time() - t0:.1f} s")


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
    """a real mosaic: output i has its centre off the middle and four tiles (sources i, i + 1, i + 2, i) touching it, tile 0
    larger than its quadrant, tile 3 smaller (fill shows)"""
    out = []
    for i in range(len(recs)):
        cx, cy = S // 3 + 5 * i, S // 2 - 3 * i
        quad = []
        for k, (tw, th) in enumerate(((cx + 7, cy - 2), (S - cx, cy), (cx, S - cy + 4), (S // 4, S // 5))):
            off, h, w, flip = recs[(i + k) % len(recs)][:4]
            quad.append((off, h, w, flip ^ (k == 2), tw, th, cx if k & 1 else cx - tw, cy if k & 2 else cy - th))
        out.append((cx, cy, quad))
    return out


def _jittered(recs):
    return [(off, h, w, fl, ORDERS[i], FACTORS[i]) for i, (off, h, w, fl, _, _) in enumerate(recs)]


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("S", sa.SIZES)
def test_g1_identity_records_reproduce_the_plain_and_the_mosaic_transform_bit_for_bit(batch, S, dtype):
    flat, recs, _ = batch
    ident = [ar.IDENTITY] * len(recs)
    tiles = _tiles(S, recs)
    for jitter in (False, True):
        r = _jittered(recs) if jitter else recs
        want = ops().image_prep(flat, r, S, jitter, dtype, oip.MEAN, oip.STD)
        got = ops().image_prep_affine(flat, r, None, ident, S, 114, jitter, dtype, oip.MEAN, oip.STD)
        assert got.dtype == dtype and got.shape == (len(recs), 3, S, S)
        assert torch.equal(got, want), f"plain S={S} {dtype} jitter={jitter}: {int((got != want).sum())} elements differ"
        want = ops().image_prep_mosaic(flat, r, tiles, S, 114, jitter, dtype, oip.MEAN, oip.STD)
        got = ops().image_prep_affine(flat, r, tiles, ident, S, 114, jitter, dtype, oip.MEAN, oip.STD)
        assert torch.equal(got, want), f"mosaic S={S} {dtype} jitter={jitter}: {int((got != want).sum())} elements differ"
    # ... and through the transform: identity matrices, and None
    from src.data.transforms import BatchTransform
    imgs = [torch.from_numpy(im) for im in batch[2]]
    params = [(i == 1, ORDERS[i], FACTORS[i]) for i in range(3)]
    plain, _ = BatchTransform(True, S, "cuda", dtype)(imgs, params=params)
    tr = BatchTransform(True, S, "cuda", dtype, affine={})
    assert torch.equal(tr(imgs, params=params, affine=[None] * 3)[0], plain)
    assert torch.equal(tr(imgs, params=params, affine=[[[1, 0, 0], [0, 1, 0]]] * 3)[0], plain)


def _canvases(batch, S, mosaic=False):
    """the device's own canvases (N, S, S, 3) of the plain resize or of the mosaic of _tiles"""
    flat, recs, _ = batch
    if mosaic:
        return _levels(ops().image_prep_mosaic(flat, recs, _tiles(S, recs), S, sa.FILL, False, F32, ZERO, ONE))
    return _levels(ops().image_prep(flat, recs, S, False, F32, ZERO, ONE))


def _warp(batch, S, records, mosaic=False, fill=sa.FILL):
    flat, recs, _ = batch
    out = ops().image_prep_affine(flat, recs, _tiles(S, recs) if mosaic else None, records, S, fill, False, F32, ZERO, ONE)
    torch.cuda.synchronize()
    return _levels(out)


@pytest.mark.parametrize("S", sa.SIZES)
def test_g2_the_exact_class_is_the_index_arithmetic_on_the_canvas(batch, S):
    from src.data.transforms import affine_record
    canv = _canvases(batch, S)
    cases = list(sa.exact_matrices(S).items())
    assert [n for n, _ in cases] == ["identity", "shift+7-5", "turn90", "turn180", "turn270", "half_pixel", "mirror_x"]
    for j in range(0, len(cases), 3):
        group = [cases[(j + i) % len(cases)] for i in range(3)]
        got = _warp(batch, S, [affine_record(m) for _, (m, _) in group])
        for i, (name, (m, want)) in enumerate(group):
            w = want(canv[i])
            assert np.array_equal(got[i], w), f"S={S} {name} image {i}: {int((got[i] != w).sum())} elements differ"
            r = sa.check_warp(f"S={S} {name} image {i}", got[i], canv[i], affine_record(m), stage="affine exact")
            assert r["ambiguous"] == 0
    # another fill level reaches exactly the pixels nothing lands on
    rec = [affine_record(cases[1][1][0])] * 3
    a, b = _warp(batch, S, rec), _warp(batch, S, rec, fill=7)
    uncovered = np.zeros((S, S), bool)
    uncovered[:, :7] = True
    uncovered[S - 5:, :] = True
    assert np.array_equal((a != b).any(-1), np.broadcast_to(uncovered, (3, S, S))) and np.array_equal((a != b).all(-1), (a != b).any(-1))
    assert (b[:, uncovered] == 7).all() and (a[:, uncovered] == sa.FILL).all()


@pytest.mark.parametrize("mosaic", [False, True], ids=["plain", "mosaic"])
@pytest.mark.parametrize("S", sa.SIZES)
def test_g3_general_records_against_the_sets_of_allowed_levels(batch, S, mosaic):
    from src.data.transforms import affine_matrix, affine_record
    canv = _canvases(batch, S, mosaic)
    names = list(sa.GENERAL)
    assert len(names) == 9
    for j in range(0, 9, 3):
        group = names[j:j + 3]
        records = [affine_record(affine_matrix(sa.GENERAL[n], S)) for n in group]
        got = _warp(batch, S, records, mosaic)
        for i, (name, rec) in enumerate(zip(group, records)):
            what = f"S={S} {'mosaic' if mosaic else 'plain'} {name} image {i}"
            out = ar.outside(rec, S)
            assert (got[i][out] == sa.FILL).all(), f"{what}: a pixel with all four taps outside is not the fill level"
            if name == "pushed_out":
                assert out.all() and (got[i] == sa.FILL).all()
            r = sa.check_warp(what, got[i], canv[i], rec)              # StrictMismatch outside the sets, CannotTell over the cap
            print(f"\n[strict_affine] {what}: {r['ambiguous'] / r['n']:.3%} ambiguous, {r['equal'] / r['n']:.4%} equal to the fp32 restatement", end="")


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
    """mosaic -> warp -> four colour ops, sampled under a fixed seed, against mosaic_ref -> affine_ref -> finish under the input
    pipeline's contract for the colour stages (tests/test_gpu_mosaic.py: >= 97 % of all elements exact, none more than 6 levels
    off); the boxes are affine_boxes(mosaic_boxes(...))."""
    from src.data.transforms import BatchTransform, affine_matrix, affine_record, mosaic_geometry
    S = 64
    sizes = [(17, 301), (64, 64), (333, 500), (200, 1200), (48, 40), (480, 640), (100, 80), (64, 64)]
    imgs = [torch.from_numpy(im) for im in si.smooth_images(21, sizes)]
    tg = _targets(5, sizes)
    mcfg, acfg = {"p": 0.75, "gain": [0.4, 1.6]}, {"degrees": 20.0, "translate": 0.15, "scale": 0.4, "shear": 4.0}
    tr = BatchTransform(True, S, "cuda", mosaic=mcfg, affine=acfg)
    torch.manual_seed(13)
    params = [tr.sample() for _ in imgs]
    mdraws, adraws = tr.sample_mosaic(len(imgs)), tr.sample_affine(len(imgs))
    assert any(d is None for d in mdraws) and sum(d is not None for d in mdraws) >= 4
    torch.manual_seed(13)
    got, out = tr(imgs, tg)
    assert got.shape == (8, 3, S, S) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    np_imgs = [t.numpy() for t in imgs]
    want = []
    for i, (d, a) in enumerate(zip(mdraws, adraws)):
        flip, order, fac = params[i]
        if d is None:
            ref = torch.cat([oip.transform_boxes(tg[i]["boxes"], sizes[i][1], sizes[i][0], S, flip), tg[i]["labels"]], 1)
            rec = mosaic_ref.plain_record(i, flip, S)
        else:
            rec = mosaic_geometry(d, i, sizes, flip, S)
            ref = mosaic_ref.mosaic_boxes(rec, tg, sizes, S)
        m = affine_matrix(a, S)
        ref = ar.affine_boxes(m, ref, S)
        b = out[i]["boxes"]
        # the mosaic's boxes agree to 1e-4 (tests/test_gpu_mosaic.py); a row of the matrix has |m00| + |m01| <= 1.4 (1 + tan 4) < 1.6,
        # a hull side takes two corners: 2 * 1.6 * 1e-4, plus fp32 roundings at 64 (a few 4e-6)
        assert b.shape == ref.shape and b.dtype == torch.float32 and torch.allclose(b, ref, rtol=0, atol=3.5e-4), (i, b, ref)
        assert out[i]["name"] == f"im{i}" and "labels" not in out[i]
        if b.numel():
            assert float(b[:, :2].min()) >= 0 and float((b[:, 0] + b[:, 2]).max()) <= S + 1e-3 and float((b[:, 1] + b[:, 3]).max()) <= S + 1e-3
            assert float(b[:, 2:4].min()) >= 2.0
        canvas = mosaic_ref.mosaic_canvas(np_imgs, rec, S, 114)[0]
        want.append(mosaic_ref.finish(ar.warp_f32(canvas, affine_record(m), 114), order, fac))
    assert sum(o["boxes"].shape[0] for o in out) > 0
    d = (got.cpu() - torch.stack(want)).abs()
    exact, lim = float((d < 1e-5).float().mean()), 6.05 / 255 / 0.224
    print(f"\n[strict_affine] S=64, 8 sampled outputs, mosaic + warp + four colour ops: {exact:.4%} exact, max {float(d.max()):.4f} (limit {lim:.4f})")
    assert exact >= 0.97 and float(d.max()) <= lim
    torch.manual_seed(13)
    again, out2 = tr(imgs, tg)
    assert torch.equal(again, got) and all(torch.equal(a["boxes"], b["boxes"]) for a, b in zip(out, out2))
    bf, _ = BatchTransform(True, S, "cuda", BF, mosaic=mcfg, affine=acfg)(imgs, tg, params=params, mosaic=mdraws, affine=adraws)
    assert bf.dtype == BF and torch.equal(bf, got.to(BF))


class _Spy:
    """stands where the loader's transform stood: forwards everything, and in an epoch with both switches off runs a transform
    built WITHOUT either key on the same inputs from the same RNG state and holds the two outputs against each other"""

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
        if not inner.mosaic_on and not inner.affine_on:
            after = torch.get_rng_state()
            torch.set_rng_state(state)
            want, want_t = plain(images, targets)
            same = torch.equal(batch, want) and torch.equal(torch.get_rng_state(), after) and \
                all(torch.equal(a["boxes"], b["boxes"]) for a, b in zip(out, want_t))
        self.__dict__["log"].append((inner.mosaic_on, inner.affine_on, same))
        return batch, out


def test_g5_one_captured_training_run_with_mosaic_and_warp_closed_for_the_last_epoch(tmp_path, monkeypatch):
    """Preset n on a tiny parquet dataset, two epochs of two batches at 160 x 160, 120 boxes per source image, `mosaic: {p: 1,
    close_epochs: 1}` and `affine: {degrees: 10, close_epochs: 1}`: every batch goes through the captured step (a warped mosaic
    never carries more than max_boxes = 128), the loss is finite, and the last epoch is the transform without either key."""
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
                              affine={"degrees": 10.0, "close_epochs": 1})
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
    assert log == [(True, True, None), (True, True, None), (False, False, True), (False, False, True)], log
    counts = [n for _, _, n, _ in steps]
    assert all(0 < n <= 128 for n in counts[:2]) and counts[2:] == [120, 120], counts
    for *_, ld in steps:
        assert all(np.isfinite(ld[k]) for k in ("total_loss", "box_loss", "cls_loss")), ld
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
