"""-m gpu: the on-device input pipeline (csrc/image_prep.hip: k_resize_flip, k_mosaic, k_gray_mean, k_color) held stage by
stage to tests/strict_image.py: every stored uint8 level inside the set of levels its float64 reference and derived bound
allow, from the SAME levels the device stage read; nothing propagates from one stage into the next.  The end-to-end anchor
against the oracle stays in tests/test_gpu_input_pipeline.py and tests/test_gpu_mosaic.py.

How a stage is isolated through the existing entry points (no kernel knows about the tests):
    resize alone      jitter = 0, mean 0, std 1, fp32: the output is level * (1/255.f), asserted bit for bit, so
                      round(out * 255) IS the staging buffer after the resize
    one op alone      an S x S source resizes to itself (exact class), order = (op,) pads the other slots with -1
    after every slot  the prefixes of an order as records of one batch; slot k + 1 is checked from the device's own slot-k levels
    stage / means     the call ops.image_prep makes, with test-owned scratch buffers (contrast: the means row is read back)
Paths reached: non-integer down, up along one axis and 4.7x down along the other, 30+ taps per axis, up with S > 256 (the second
x-block partial), one row / one column, the exact class (identity, 2x down), flip at odd W, a source at an odd byte offset,
hw = 2500 (grid-stride tail, gx = 10) and hw = 262144 (gx = 64, 16 trips), all three output types, the four mosaic quadrants
with a clipped, a flipped and a missing tile."""
import time

import numpy as np
import pytest
import torch

import mosaic_ref
import strict_image as si
from oracle import image_prep as oip

pytestmark = pytest.mark.gpu
F32, BF, HF = torch.float32, torch.bfloat16, torch.float16
ZERO, ONE = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
NO_JITTER = (1.0, 1.0, 1.0, 0.0)
C255 = np.float32(1) / np.float32(255)


def ops():
    from src.hipops import ops as o
    return o


@pytest.fixture(autouse=True, scope="module")
def _print_report():
    t0 = time.time()
    yield
    print("\n" + si.report() + f"\n[strict_image] wall time of tests/test_gpu_image.py: {time.time() - t0:.1f} s")


def cid(c):
    return "x".join(map(str, c))


def _table(images, recs):
    """images: uint8 (H, W, 3) arrays, back to back in one buffer; recs: (image index, flip, order, factors)
    -> (device buffer, the records ops.image_prep takes)"""
    offs = np.concatenate([[0], np.cumsum([im.size for im in images])])
    flat = torch.cat([torch.from_numpy(np.ascontiguousarray(im)).reshape(-1) for im in images]).cuda()
    return flat, [(int(offs[i]), images[i].shape[0], images[i].shape[1], fl, order, fac) for i, fl, order, fac in recs]


def _levels(out):
    """fp32 (N, 3, S, S) written with mean 0, std 1 -> the uint8 levels (N, S, S, 3) behind it, asserting out == level * (1/255.f)"""
    out = out.float().cpu().numpy()
    lv = np.round(out.astype(np.float64) * 255.0)
    assert lv.min() >= 0 and lv.max() <= 255 and np.array_equal(lv.astype(np.float32) * C255, out), "the output is not level * (1/255.f)"
    return lv.transpose(0, 2, 3, 1)


def run(images, recs, size, jitter, dtype=F32, mean=ZERO, std=ONE):
    flat, table = _table(images, recs)
    out = ops().image_prep(flat, table, size, jitter, dtype, mean, std)
    torch.cuda.synchronize()
    return out


def run_owned(images, recs, size, jitter, dtype=F32, mean=ZERO, std=ONE):
    """the lib.call of ops.image_prep with test-owned stage / means -> (out, stage (N, 3, S, S) uint8, means (4, N))"""
    o = ops()
    flat, table = _table(images, recs)
    n = len(table)
    host = torch.zeros(n * o.lib.query("yolo_prep_image_bytes"), dtype=torch.uint8).pin_memory()
    o._prep_table_fill(host, table)
    dev = host.to("cuda")
    stage = torch.zeros((n, 3, size, size), dtype=torch.uint8, device="cuda")
    means = torch.full((4 * n,), -1.0, dtype=torch.float32, device="cuda")
    out = torch.empty((n, 3, size, size), dtype=dtype, device="cuda")
    o.lib.call("yolo_image_prep", o._p(flat), o._p(dev), n, size, int(bool(jitter)), o._p(stage), o._p(means), o._p(out), o.dt(dtype),
               *[float(v) for v in mean], *[float(v) for v in std], o._stream(flat))
    torch.cuda.synchronize()
    return out, stage.cpu(), means.cpu().view(4, n)


# ------------------------------------------------------------------------------------------ resize alone
@pytest.mark.parametrize("case", si.RESIZE_CASES, ids=cid)
def test_resize_alone_noise_and_impulses_with_and_without_flip(case):
    h, w, s = case
    images, recs = si.resize_case(*case)
    if (h, w) == (17, 301):
        assert images[0].size % 2 == 1                        # the second image starts at an odd byte offset
    got = _levels(run(images, [(i, fl, (), NO_JITTER) for i, fl in recs], s, False))
    for j, ((i, fl), (x, e), orc) in enumerate(zip(recs, si.resize_case_ref(*case), si.resize_case_oracle(*case))):
        what = f"{cid(case)} image {i} flip={fl}"
        exact = e == 0
        if case in si.EXACT_CASES:                            # bit for bit, ties included, before any set is formed
            want = np.floor(x + 0.5)
            assert np.array_equal(got[j][exact], want[exact]), f"{what}: {int((got[j][exact] != want[exact]).sum())} exact-class elements differ"
            assert exact.all() or (h, w) == (128, 128)
        r = si.check_levels("resize", what, got[j], x, e, si.q_resize, si.CAP_RESIZE, orc)
        if i < 2 and not fl:
            print(f"\n[strict_image] resize {what}: {r['ambiguous'] / r['n']:.3%} ambiguous, {r['equal'] / r['n']:.4%} equal to the oracle, "
                  f"{exact.mean():.1%} exact class", end="")


# ------------------------------------------------------------------------------------------ each colour op alone
def _alone(op, f):
    fac = list(NO_JITTER)
    fac[op] = f
    return (op,), tuple(fac)


@pytest.mark.parametrize("inp", ["lattice", "50x50"])
@pytest.mark.parametrize("op", [0, 1, 2, 3], ids=si.OPS)
def test_each_colour_op_alone(op, inp):
    lv = si.lattice() if inp == "lattice" else si.small_image()
    size = lv.shape[0]
    factors = si.HUE_FACTORS if op == 3 else si.BLEND_FACTORS
    recs = [(0, False, *_alone(op, f)) for f in factors]
    out, stage, means = run_owned([lv], recs, size, True)
    got = _levels(out)
    assert np.array_equal(stage.numpy().transpose(0, 2, 3, 1), got)          # slots 1..3 hold no op: the staging buffer is the slot-0 result
    mean = si.gray_mean_ref(lv)
    if op == 1:                                               # the means row of slot 0 against the float64 mean
        si.check_close("gray_mean", f"{inp}", means[0].numpy(), np.full(len(recs), mean[2]), np.full(len(recs), mean[1] - mean[2]))
        out2, _, means2 = run_owned([lv], recs, size, True)
        print(f"\n[strict_image] contrast {inp} run twice: means bit-equal {torch.equal(means, means2)}, output bit-equal {torch.equal(out, out2)}; "
              f"means {means[0].tolist()} (float64 {mean[2]:.9g}, allowed +- {mean[1] - mean[2]:.3g})", end="")
    for j, f in enumerate(factors):
        r = si.check_op(op, f"{inp} f={f}", lv, f, got[j], mean=mean)
        print(f"\n[strict_image] {si.OPS[op]} {inp} f={f}: {r['ambiguous'] / r['n']:.3%} ambiguous, {r['n'] - r['equal']} of {r['n']} differ from the oracle", end="")


# ------------------------------------------------------------------------------------------ the chain, stage-wise
def test_the_chain_after_every_slot_from_the_device_s_own_levels():
    img = si.chain_image()
    recs = [(0, False, order[:k + 1], si.CHAIN_FACTORS) for order in si.ORDERS for k in range(4)]
    got = _levels(run([img], recs, 64, True))
    assert got.shape == (32, 64, 64, 3)
    for a, order in enumerate(si.ORDERS):
        lv = img.astype(np.float64)                           # 64 x 64 -> 64: the exact class, the resize hands the image on
        for k, op in enumerate(order):
            si.check_op(op, f"chain {order} slot {k}", lv, si.CHAIN_FACTORS[op], got[4 * a + k])
            lv = got[4 * a + k]


# ------------------------------------------------------------------------------------------ normalise
@pytest.mark.parametrize("dtype", [F32, BF, HF], ids=["f32", "bf16", "f16"])
def test_normalise_the_lattice_with_the_real_mean_and_std(dtype):
    lv = si.lattice()
    out = run([lv], [(0, False, (), NO_JITTER)], 512, False, dtype, oip.MEAN, oip.STD)
    assert out.dtype == dtype
    got = out[0].to(torch.float64).cpu().numpy().transpose(1, 2, 0)
    x, e = si.normalise_ref(lv, oip.MEAN, oip.STD, dtype)
    share = si.check_close("normalise", str(dtype), got, x, e, si.normalise_f32(lv, oip.MEAN, oip.STD, dtype))
    print(f"\n[strict_image] normalise {dtype}: largest share of the bound used {share:.3f}", end="")


# ------------------------------------------------------------------------------------------ mosaic
def test_mosaic_fill_exact_and_every_tile_pixel_in_the_set_of_its_own_resize():
    images = si.mosaic_sources()
    s = si.MOSAIC_S
    offs = np.concatenate([[0], np.cumsum([im.size for im in images])])
    flat = torch.cat([torch.from_numpy(im).reshape(-1) for im in images]).cuda()
    recs = [(int(offs[i]), images[i].shape[0], images[i].shape[1], False, (), NO_JITTER) for i in range(len(si.MOSAIC_RECORDS))]
    tiles = []
    for rec in si.MOSAIC_RECORDS:
        quad = [None if t is None else (int(offs[t[0]]), images[t[0]].shape[0], images[t[0]].shape[1], t[1], t[2], t[3], t[4], t[5])
                for t in rec["tiles"]]
        tiles.append((rec["cx"], rec["cy"], quad))
    out = ops().image_prep_mosaic(flat, recs, tiles, s, 114, False, F32, ZERO, ONE)
    torch.cuda.synchronize()
    got = _levels(out)
    for r, rec in enumerate(si.MOSAIC_RECORDS):
        canvas, is_fill = mosaic_ref.mosaic_canvas(images, rec, s, 114)
        assert is_fill.any() and (got[r][is_fill] == 114).all(), f"record {r}: a fill pixel is not the fill level"
        x, e = si.mosaic_ref_canvas(images, rec, s, 114)
        si.check_levels("mosaic", f"record {r}", got[r], x, e, si.q_resize, si.CAP_RESIZE, canvas)


def test_every_route_reproduces_the_recorded_digests():
    """The four leaves share one runner, so the identity tests between them (identity warp = no warp, r = 1 = unmixed, one-tile mosaic
    = plain resize) compare that runner with itself.  This holds it to the outputs of the commit named in
    tests/golden/image_prep_routes.json, recorded on an MI355X by tools/record_prep_digests.py before the routes were merged: all 8
    combinations of (tiles, affine, mix) through their narrowest leaf, S = 20 (16-byte mixup kernel) and S = 33 (byte kernel), fp32
    and bf16, jitter off (k_gray_mean's float atomics have no fixed order) -- 32 outputs, byte for byte."""
    import importlib.util
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("record_prep_digests", os.path.join(root, "tools", "record_prep_digests.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(root, "tests", "golden", "image_prep_routes.json")) as f:
        want = json.load(f)
    got = tool.digests()
    assert len(want["digests"]) == 32 and set(got) == set(want["digests"]) and len(set(got.values())) == 32
    bad = sorted(k for k in got if got[k] != want["digests"][k])
    print(f"\n[digests] {len(got) - len(bad)} of {len(got)} outputs equal those of commit {want['commit'][:7]}", end="")
    assert not bad, f"outputs differ from those of commit {want['commit'][:7]}: {bad}"
