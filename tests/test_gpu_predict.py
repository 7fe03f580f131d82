"""-m gpu: `Model.predict` and its two kernels -- csrc/image_prep.hip::k_letterbox through ops.letterbox,
csrc/decode_nms.hip::k_rows_to_source through ops.rows_to_source -- and the replayed chunk of src/model/infer_graph.py.

G1  the letterbox equals the existing two-launch route (ops.image_prep_mosaic: one tile per output, jitter off) bit for bit
G2  a source at byte offset 2^31 + 5 gives what the same source gives at offset 0
G3  the inverse map against tests/predict_ref.py::rows_to_source_ref: boxes bit-equal, score within the derived SIGMOID_BOUND
G4  square sources reproduce `Model.inference`       G5  the pad is subtracted in the right direction (no resize involved)
G6  replay equals launch by launch; entries, chunks, weight updates, .half()       G7  guards"""
import ctypes
import math

import numpy as np
import pytest
import torch

import predict_ref as pr
import strict_image as si
from oracle import blocks as ob
from oracle import image_prep as oip
from oracle.params import det_fill_
from src.data.letterbox import FILL, letterbox_geometry, letterbox_records

pytestmark = pytest.mark.gpu
NO_JITTER = (1.0, 1.0, 1.0, 0.0)
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _sources(S):
    """(H, W): up- and downscales on both axes, the identity, one pixel, and a downscale with long tap loops"""
    return [(37, 41), (200, 50), (50, 200), (S, S), (1, 1), (7, 10), (300, 400)]


def _pack(images, lead=0):
    """uint8 HWC images back to back behind `lead` bytes -> (flat device tensor, offsets)"""
    offs, off = [], lead
    for im in images:
        offs.append(off)
        off += im.size
    flat = np.zeros(off, np.uint8)
    for im, o in zip(images, offs):
        flat[o:o + im.size] = im.reshape(-1)
    return torch.from_numpy(flat).cuda(), offs


def _two_launch_route(flat, offs, images, S, dtype):
    """the baseline, unchanged code: k_mosaic with every pixel in quadrant 3 (cx = cy = 0) and that quadrant's tile the
    letterbox rectangle, then k_color<T, true>"""
    from src.hipops import ops
    recs = [(o, im.shape[0], im.shape[1], False, (), NO_JITTER) for o, im in zip(offs, images)]
    tiles = []
    for o, im in zip(offs, images):
        nw, nh, left, top, _, _ = letterbox_geometry(im.shape[0], im.shape[1], S)
        t = (o, im.shape[0], im.shape[1], False, nw, nh, left, top)
        tiles.append((0, 0, [t, None, None, t]))
    return ops.image_prep_mosaic(flat, recs, tiles, S, FILL, False, dtype, oip.MEAN, oip.STD)


def _letter_recs(offs, images, S):
    return [(o, im.shape[0], im.shape[1]) + letterbox_geometry(im.shape[0], im.shape[1], S) for o, im in zip(offs, images)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("S", [96, 20, 33])
def test_g1_letterbox_equals_the_two_launch_route(S, dtype):
    from src.hipops import ops
    images = [si.noise(h, w, 700 + i) for i, (h, w) in enumerate(_sources(S))]
    for im in images:                                                   # N = 1
        flat, offs = _pack([im])
        got = ops.letterbox(flat, _letter_recs(offs, [im], S), S, FILL, dtype, oip.MEAN, oip.STD)
        want = _two_launch_route(flat, offs, [im], S, dtype)
        assert got.dtype == dtype and got.shape == (1, 3, S, S)
        assert torch.equal(got, want), f"S={S} {dtype} {im.shape}: {int((got != want).sum())} elements differ"
        if im.shape[:2] == (S, S):                                      # the resize is the identity: the source's own levels
            lv = si.normalise_f32(im, oip.MEAN, oip.STD, dtype).transpose(2, 0, 1)
            assert np.array_equal(got[0].double().cpu().numpy(), lv)
    # N = 5 with mixed sizes in one launch (an odd S and odd sizes give unaligned image bases), and a blank slot behind them
    batch = [images[k] for k in (0, 6, 3, 5, 1)]
    flat, offs = _pack(batch)
    recs = _letter_recs(offs, batch, S)
    got = ops.letterbox(flat, recs + [(0, 0, 0, 0, 0, 0, 0, 1.0, 1.0)], S, FILL, dtype, oip.MEAN, oip.STD)
    want = _two_launch_route(flat, offs, batch, S, dtype)
    assert got.shape == (6, 3, S, S) and torch.equal(got[:5], want)
    blank = si.normalise_f32(np.full((S, S, 3), FILL, np.uint8), oip.MEAN, oip.STD, dtype).transpose(2, 0, 1)
    assert np.array_equal(got[5].double().cpu().numpy(), blank)
    bars = got[0, :, :letterbox_geometry(37, 41, S)[3]]                 # the 37 x 41 picture has bars above and below
    assert bars.numel() > 0 and np.array_equal(bars.double().cpu().numpy(), blank[:, :bars.shape[1]])


def test_g2_a_source_beyond_2_to_31_bytes():
    from src.hipops import ops
    S, im = 33, si.noise(37, 41, 731)
    off = (1 << 31) + 5
    big = torch.empty((1 << 31) + (64 << 10), dtype=torch.uint8, device="cuda")
    big[off:off + im.size] = torch.from_numpy(im.reshape(-1)).cuda()    # only the picture's own bytes are written
    geo = letterbox_geometry(37, 41, S)
    got = ops.letterbox(big, [(off, 37, 41) + geo], S, FILL, torch.float32, oip.MEAN, oip.STD)
    flat, offs = _pack([im])
    want = ops.letterbox(flat, [(0, 37, 41) + geo], S, FILL, torch.float32, oip.MEAN, oip.STD)
    assert torch.equal(got, want)
    with pytest.raises(RuntimeError):                                   # one byte short of the buffer's end: refused on the host
        ops.letterbox(big, [(big.numel() - im.size + 1, 37, 41) + geo], S, FILL, torch.float32, oip.MEAN, oip.STD)


@pytest.mark.parametrize("prob", [False, True])
def test_g3_rows_to_source_against_the_reference(prob):
    from src.hipops import ops
    recs, rows, counts = pr.cases()
    src_bytes = recs[-1][0] + 3 * recs[-1][1] * recs[-1][2]
    table = ops.letter_table(recs, pr.S, src_bytes).cuda()
    dev = torch.from_numpy(rows.copy()).cuda()
    out = ops.rows_to_source(dev, torch.from_numpy(counts.copy()).cuda(), table, prob)
    assert out.data_ptr() == dev.data_ptr()                             # in place
    got = out.cpu().numpy()
    want = pr.rows_to_source_ref(rows, counts, recs, prob)
    assert np.array_equal(got[..., :4].view(np.uint32), want[..., :4].view(np.uint32)), "box columns differ from the reference"
    assert np.array_equal(got[..., 5].view(np.uint32), rows[..., 5].view(np.uint32))
    live = np.arange(pr.MAX_DET)[None, :] < counts[:, None]
    assert np.array_equal(got[~live].view(np.uint32), rows[~live].view(np.uint32)), "a row at or past its count was touched"
    if not prob:
        assert np.array_equal(got[..., 4].view(np.uint32), rows[..., 4].view(np.uint32))
        return
    err = np.abs(got[..., 4].astype(np.float64) - pr.sigmoid64(rows[..., 4]))[live]
    print(f"\n[rows_to_source] sigmoid: max |conf - sigmoid64| = {err.max():.3e} (bound {pr.SIGMOID_BOUND:.3e}); "
          f"equal to numpy's fp32 form on {int((got[..., 4] == want[..., 4])[live].sum())} of {int(live.sum())}")
    assert (err <= pr.SIGMOID_BOUND).all()
    for n, c in enumerate(counts):
        assert (np.diff(got[n, :c, 4]) <= 0).all(), "the confidences of an image must stay non-increasing"


def _model(seed=9, preset="n"):
    """a deterministic detector whose class branch is scaled as tests/test_gpu_model.py::test_replayed_inference_equals_eager_inference
    scales it: enough confident anchors for the NMS to have work"""
    from src.model.model_builder import Model
    m = Model(**ob.PRESETS[preset], num_classes=80)
    det_fill_(m.state_dict(), seed)
    m = m.cuda().eval()
    with torch.no_grad():
        for lvl in m.head.cls:
            lvl[-1].weight.mul_(0.05)
            lvl[-1].bias.copy_(torch.linspace(-2.0, 1.0, 80, device="cuda"))
    return m


def _eager(model, *a, **k):
    from src.model.model_builder import Model
    Model.graph_inference = False
    try:
        return model.predict(*a, **k)
    finally:
        Model.graph_inference = True


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def test_g4_square_sources_reproduce_inference():
    from src.data.transforms import get_val_transforms
    from src.hipops import ops
    S, c = 160, 0.6                                                     # log(0.6 / 0.4) = 0.405: inside [0, 1], where inference replays
    model = _model()
    imgs = [si.smooth_images(40 + i, [(S, S)])[0] for i in range(3)]
    with torch.autocast("cuda", dtype=torch.float16):
        got = model.predict(imgs, conf=c, size=S)
        x, _ = get_val_transforms(size=S)(imgs)
        ref = model.inference(x, conf_thres=math.log(c / (1 - c)))
    assert len(got) == len(ref) == 3
    identity, _ = letterbox_records([(S, S)] * 3, S)
    table = ops.letter_table(identity, S, 3 * 3 * S * S).cuda()
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape[0] >= 1, f"image {i}: no detection -- the test would pass on empty lists"
        assert g.shape == r.shape and g.dtype == torch.float32
        box = np.minimum(np.maximum(r[:, :4].cpu().numpy(), np.float32(0)), np.float32(S))      # the geometry is the identity
        assert np.array_equal(g[:, :4].cpu().numpy().view(np.uint32), box.view(np.uint32))
        assert torch.equal(g[:, 5], r[:, 5])
        # the confidence: the fp32 sigmoid of inference's logit as the kernel forms it
        rows = torch.zeros((3, r.shape[0], 6), device="cuda")
        rows[i] = r
        conf = ops.rows_to_source(rows, torch.full((3,), r.shape[0], dtype=torch.int32, device="cuda"), table, True)[i, :, 4]
        assert torch.equal(g[:, 4], conf)
        assert (g[:, 4] >= c - pr.SIGMOID_BOUND).all() and (g[:, 4] < 1).all()


def test_g5_pad_direction_without_a_resize():
    S = 160
    model = _model()
    a = si.smooth_images(55, [(S // 2, S)])[0]                          # W = S, H = S / 2: r = 1, top = S / 4
    assert letterbox_geometry(S // 2, S, S) == (S, S // 2, 0, S // 4, 1.0, 1.0)
    b = np.full((S, S, 3), FILL, np.uint8)
    b[S // 4:S // 4 + S // 2] = a                                       # the canvas the letterbox of A is
    with torch.autocast("cuda", dtype=torch.float16):
        da, db = model.predict(a, conf=0.6, size=S)[0], model.predict(b, conf=0.6, size=S)[0]
    assert da.shape[0] >= 1 and da.shape == db.shape, "no detections: the comparison would be empty"
    want = db.cpu().numpy().copy()
    for col in (1, 3):
        want[:, col] = np.minimum(np.maximum(want[:, col] - np.float32(S // 4), np.float32(0)), np.float32(S // 2))
    assert want.dtype == np.float32
    assert np.array_equal(da.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert (da[:, 3] > 0).any() and (da[:, 1] < S // 2).any()


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_g6_replay_equals_launch_by_launch(fused):
    S, conf = 160, 0.6
    model = _model()
    if fused:
        model.fuse()
    sizes = [(120, 160), (200, 90), (160, 160)]
    pics = si.smooth_images(61, sizes)
    other = si.smooth_images(62, [(100, 150), (190, 90), (150, 150)])    # other pictures, fewer bytes: the same capacity
    with torch.autocast("cuda", dtype=torch.float16):
        eager, replayed = _eager(model, pics, conf=conf, size=S), model.predict(pics, conf=conf, size=S)
        assert len(replayed) == 3 and sum(r.shape[0] for r in replayed) > 0 and _same(eager, replayed)
        for r, (h, w) in zip(replayed, sizes):                          # boxes in the picture's own pixels, scores probabilities
            assert (r[:, [0, 2]] >= 0).all() and (r[:, [0, 2]] <= w).all() and (r[:, [1, 3]] >= 0).all() and (r[:, [1, 3]] <= h).all()
            assert (r[:, 4] > 0.5).all() and (r[:, 4] < 1).all() and (r[1:, 4] <= r[:-1, 4]).all()
        graphs = model._infer_graphs
        assert graphs is not None and graphs.disabled is None and len(graphs.entries) == 1
        assert _same(_eager(model, other, conf=conf, size=S), model.predict(other, conf=conf, size=S))
        assert len(graphs.entries) == 1, "other pictures inside the same capacity must replay the same graph"
        four = pics + other[:1]
        assert _same(_eager(model, four, conf=conf, size=S), model.predict(four, conf=conf, size=S))
        assert len(graphs.entries) == 2, "a larger batch captures a new graph"
        chunks = model.predict(pics, conf=conf, size=S, batch=2)        # 2 + (1 + a blank slot)
        assert _same(chunks, replayed) and len(graphs.entries) == 3
        assert _same(model.predict(pics, conf=conf, size=S), replayed)
        with torch.no_grad():                                           # an in-place update of a weight: the next call must see it
            model.head.box[0][-1].weight.mul_(1.5)
        eager2, replayed2 = _eager(model, pics, conf=conf, size=S), model.predict(pics, conf=conf, size=S)
        assert _same(eager2, replayed2) and not _same(replayed2, replayed), "stale weights replayed"
    model.half()
    assert model._infer_graphs is None
    eager, replayed = _eager(model, pics, conf=conf, size=S), model.predict(pics, conf=conf, size=S)
    assert sum(r.shape[0] for r in replayed) > 0 and _same(eager, replayed)
    assert model._infer_graphs is not None and model._infer_graphs.disabled is None and len(model._infer_graphs.entries) == 1


def test_g7_guards():
    from src.hipops import lib
    n = lib.query("yolo_letter_bytes")
    buf = ctypes.create_string_buffer(2 * n)
    ptr = ctypes.addressof(buf)
    assert pr.letter_fill(lib, ptr) == 0 and pr.letter_fill(lib, ptr, index=1, **pr.LETTER_BLANK) == 0
    for bad in pr.LETTER_REFUSED:
        assert pr.letter_fill(lib, ptr, **bad) == pr.YOLO_ERR_ARG, bad
    model = _model()
    pic = si.noise(40, 50, 3)
    for conf in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            model.predict(pic, conf=conf, size=96)
    for bad in (np.zeros((40, 50), np.uint8), np.zeros((40, 50, 4), np.uint8), np.zeros((3, 40, 50), np.uint8),
                np.zeros((40, 50, 3), np.float32), torch.zeros(40, 50, 1, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            model.predict([pic, bad], size=96)
    out = model.predict(torch.from_numpy(pic), size=96)                 # one image, not a list: one result
    assert len(out) == 1 and out[0].shape[1] == 6 and out[0].dtype == torch.float32
