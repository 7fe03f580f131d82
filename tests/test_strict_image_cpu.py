"""CPU tests of tests/strict_image.py: what proves, without a GPU, that the per-pixel sets of allowed levels of the input
pipeline pass honest fp32 arithmetic, fail arithmetic that is subtly wrong, and that the former whole-chain limit did not.

Stand-ins, with NO element outside its set at every shape of tests/test_gpu_image.py:
  (i)   the fp32 oracle's stages (oracle/image_prep.py: separable resize with normalised weights, float32(1.0 - f) from the
        double factor, the float64 gray mean rounded once)
  (ii)  the resize summed in resize_pixel's own order in fp32 (strict_image.resize_kernel_order)
  (iii) the kernel's form of the blend (1.f - ratio in fp32) with an fp32 gray mean summed in a shuffled order
The ambiguity caps (2 % resize, 1 % colour op) hold for the reference alone on every case: each check below runs under them.
Exact class: the fp32 stand-ins equal floor(x + 0.5) of the float64 value on every pixel the reference marks exact.
Every mutant of strict_image.MUTANTS raises StrictMismatch in its stage on at least one case.
Old versus new: the former `_compare` (99.5 % / 3 levels after the resize, 97 % / 6 levels after the chain), on the former
tests' own smooth images, passes the mutants of OLD_PASSES -- found by running all of them -- next to the strict failure."""
import numpy as np
import pytest
import torch

import mosaic_ref
import strict_image as si
from oracle import image_prep as oip

f32 = np.float32
F32, BF, HF = torch.float32, torch.bfloat16, torch.float16


@pytest.fixture(autouse=True, scope="module")
def _report():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    yield
    print("\n" + si.report())


def cid(c):
    return "x".join(map(str, c))


# ------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("sizes", sorted({(c[0], c[2]) for c in si.RESIZE_CASES} | {(c[1], c[2]) for c in si.RESIZE_CASES}), ids=cid)
def test_the_taps_are_the_oracle_s_weights(sizes):
    lo, n, w = si.taps(*sizes)
    for i, (olo, ow) in enumerate(oip.aa_weights(*sizes)):
        assert olo == lo[i] and len(ow) == n[i]
        assert np.array_equal(w[i, :n[i]] / w[i, :n[i]].sum(dtype=np.float32), ow)
        assert not w[i, n[i]:].any()
    assert si.HUE_K == float(f32(255.0 + 1.0 - 1e-3))


@pytest.mark.parametrize("case", si.RESIZE_CASES, ids=cid)
def test_resize_both_fp32_stand_ins_lie_in_every_set_and_the_reference_keeps_the_cap(case):
    images, recs = si.resize_case(*case)
    s = case[2]
    for (i, fl), (x, e), orc in zip(recs, si.resize_case_ref(*case), si.resize_case_oracle(*case)):
        what = f"{cid(case)} image {i} flip={fl}"
        si.check_levels("resize", what + " reference", si.q_resize(x), x, e, si.q_resize, si.CAP_RESIZE, record=False)
        si.check_levels("resize", what + " oracle", orc, x, e, si.q_resize, si.CAP_RESIZE, orc)
        si.check_levels("resize", what + " kernel order", si.resize_kernel_order(images[i], s, s, fl), x, e, si.q_resize,
                        si.CAP_RESIZE, record=False)
    # the impulse in the last column, unflipped and flipped, are mirror images (the filter is symmetric about W - 1)
    (xa, _), (xb, _) = si.resize_ref(images[-1], s, s, False), si.resize_ref(images[-1][:, ::-1], s, s, True)
    assert np.array_equal(xa, xb)


@pytest.mark.parametrize("case", si.EXACT_CASES, ids=cid)
def test_exact_class_the_fp32_stand_ins_are_the_rounded_float64_value(case):
    images, recs = si.resize_case(*case)
    h, w, s = case
    for (i, fl), (x, e), orc in zip(recs, si.resize_case_ref(*case), si.resize_case_oracle(*case)):
        exact = e == 0
        want = np.clip(np.floor(x + 0.5), 0, 255)
        assert np.array_equal(orc[exact], want[exact])
        assert np.array_equal(si.resize_kernel_order(images[i], s, s, fl)[exact], want[exact])
        if (h, w) == (128, 128):                              # 2x down: the interior; the border normalises by 1.75 and takes the set
            assert exact[1:-1, 1:-1].all() and not exact[0].any() and not exact[:, -1].any()
            assert ((x[1:-1, 1:-1] * 64) % 1 == 0).all() and (i >= 2 or ((x[1:-1, 1:-1] * 2) % 2 == 1).any())   # noise: ties are present
        else:
            assert exact.all()
    if (h, w) == (64, 64):
        assert np.array_equal(si.q_resize(si.resize_case_ref(*case)[0][0]), images[0])               # identity: the image itself


def _resize_mutant_fails(case, mut):
    images, recs = si.resize_case(*case)
    hit = []
    for (i, fl), (x, e) in zip(recs, si.resize_case_ref(*case)):
        got = si.resize_levels(images[i], case[2], case[2], fl, mut)
        hit += si.failing(lambda: si.check_levels("resize", f"{cid(case)} {mut}", got, x, e, si.q_resize, 1.0, record=False))
    return hit


@pytest.mark.parametrize("mut", si.MUTANTS["resize"])
def test_resize_mutants_fail(mut):
    failed = [c for c in si.RESIZE_CASES[:4] + [(128, 128, 64)] if _resize_mutant_fails(c, mut)]
    assert failed, mut
    if mut == "drop_last_tap":                                # the impulses in the last row / column alone see it too
        images, recs = si.resize_case(37, 23, 264)
        x, e = si.resize_case_ref(37, 23, 264)[recs.index((len(images) - 1, False))]
        got = si.resize_levels(images[-1], 264, 264, False, mut)
        with pytest.raises(si.StrictMismatch):
            si.check_levels("resize", "impulse", got, x, e, si.q_resize, 1.0, record=False)


def test_mosaic_the_oracle_s_canvas_lies_in_the_sets_and_fill_is_exact():
    images = si.mosaic_sources()
    for r, rec in enumerate(si.MOSAIC_RECORDS):
        x, e = si.mosaic_ref_canvas(images, rec, si.MOSAIC_S, 114)
        canvas, is_fill = mosaic_ref.mosaic_canvas(images, rec, si.MOSAIC_S, 114)
        assert is_fill.any() and (~is_fill).any()
        assert (e[is_fill] == 0).all() and (x[is_fill] == 114).all()
        si.check_levels("mosaic", f"record {r}", canvas, x, e, si.q_resize, si.CAP_RESIZE, canvas)
    rec = si.MOSAIC_RECORDS[0]
    assert rec["tiles"][3] is None and rec["tiles"][0][4] < 0 and rec["tiles"][0][5] < 0 and rec["tiles"][0][1]
    assert all(t[2] != t[3] for t in rec["tiles"] if t is not None)


# ------------------------------------------------------------------------------------------ colour ops
def _blend_kernel_form(a, b, ratio):
    """blend_u8 as the kernel writes it: the fp32 ratio, 1.f - ratio in fp32"""
    r = f32(ratio)
    return np.floor(np.clip(a * r + b * (f32(1) - r), 0, 255)).astype(np.float32)


def _gray_mean_shuffled(lv, seed):
    g = oip._gray(np.asarray(lv).astype(np.float32)).reshape(-1)
    g = g[np.random.default_rng(seed).permutation(g.size)]
    acc = f32(0)
    for part in np.array_split(g, 40):                        # fp32 partials divided by hw, then added: the kernel's shape
        acc = acc + part.sum(dtype=np.float32) / f32(g.size)
    return acc


def _kernel_form(op, lv, factor):
    x = np.asarray(lv).astype(np.float32)
    if op == 0:
        return _blend_kernel_form(x, f32(0), factor)
    if op == 1:
        return _blend_kernel_form(x, _gray_mean_shuffled(lv, 7), factor)
    return _blend_kernel_form(x, oip._gray(x)[..., None], factor)


COLOUR_INPUTS = {"lattice": si.lattice, "50x50": si.small_image}
DIFF_1MR = {}             # (op name, factor) -> lattice elements where the kernel's 1.f - ratio and the oracle's float32(1.0 - f) differ


@pytest.mark.parametrize("inp", list(COLOUR_INPUTS))
@pytest.mark.parametrize("op", [0, 1, 2])
def test_blends_the_oracle_and_the_kernel_s_form_lie_in_every_set(op, inp):
    lv = COLOUR_INPUTS[inp]()
    for f in si.BLEND_FACTORS:
        orc = si.op_oracle(op, lv, f)
        si.check_op(op, f"{inp} f={f} oracle", lv, f, orc)
        kf = _kernel_form(op, lv, f)
        si.check_op(op, f"{inp} f={f} kernel form", lv, f, kf, oracle=False, record=False)
        if inp == "lattice":
            DIFF_1MR[(si.OPS[op], f)] = int((kf != orc).sum())
    if op == 1:
        lo, hi, mid = si.gray_mean_ref(lv)
        assert lo <= float(_gray_mean_shuffled(lv, 3)) <= hi and lo <= float(f32(oip._gray(lv.astype(np.float32)).mean(dtype=np.float64))) <= hi
        assert hi - lo < 0.02
    if inp == "lattice" and op == 2:
        print(f"\n[strict_image] lattice elements where 1.f - ratio and float32(1.0 - f) give another level: {DIFF_1MR}")


@pytest.mark.parametrize("inp", list(COLOUR_INPUTS))
def test_hue_the_oracle_lies_in_every_set(inp):
    lv = COLOUR_INPUTS[inp]()
    for f in si.HUE_FACTORS:
        si.check_op(3, f"{inp} f={f}", lv, f, si.op_oracle(3, lv, f))


def test_the_lattice_holds_what_it_promises():
    lv = si.lattice().reshape(-1, 3).astype(np.int64)
    levels = set(si.lattice_levels().tolist())
    assert len(levels) == 64 and {0, 1, 2, 3, 126, 127, 128, 129, 252, 253, 254, 255} <= levels
    assert len(np.unique(lv[:, 0] * 65536 + lv[:, 1] * 256 + lv[:, 2])) == 512 * 512 == 64 ** 3


@pytest.mark.parametrize("stage", ["brightness", "contrast", "saturation", "hue"])
def test_colour_mutants_fail(stage):
    op = si.OPS.index(stage)
    factors = si.HUE_FACTORS if op == 3 else si.BLEND_FACTORS
    for mut in si.MUTANTS[stage]:
        hit = []
        for name, make in COLOUR_INPUTS.items():
            lv = make()
            for f in factors:
                got = si.op_levels(op, lv, f, mut)
                hit += si.failing(lambda: si.check_op(op, f"{name} f={f} {mut}", lv, f, got, oracle=False, record=False))
        assert stage in hit, (stage, mut)
    # the unmutated levels pass
    si.check_op(op, "reference", si.small_image(), factors[0], si.op_levels(op, si.small_image(), factors[0]), oracle=False, record=False)


def test_chain_stage_wise_from_the_stand_in_s_own_levels():
    img = si.chain_image()
    assert np.array_equal(si.q_resize(si.resize_ref(img, 64, 64)[0]), img)
    for order in si.ORDERS:
        lv = img.astype(np.float32)
        for k, op in enumerate(order):
            f = si.CHAIN_FACTORS[op]
            nxt = si.op_oracle(op, lv, f)
            si.check_op(op, f"chain {order} slot {k}", lv, f, nxt, record=False)
            lv = nxt


# ------------------------------------------------------------------------------------------ normalise
@pytest.mark.parametrize("dtype", [F32, BF, HF], ids=["f32", "bf16", "f16"])
def test_normalise_stand_in_passes_and_mutants_fail(dtype):
    lv = si.lattice()
    x, e = si.normalise_ref(lv, oip.MEAN, oip.STD, dtype)
    share = si.check_close("normalise", str(dtype), si.normalise_f32(lv, oip.MEAN, oip.STD, dtype), x, e)
    assert share <= 1.0
    for mut in si.MUTANTS["normalise"]:
        if mut == "bf16_trunc" and dtype != BF:
            continue
        with pytest.raises(si.StrictMismatch):
            si.check_close("normalise", f"{dtype} {mut}", si.normalise_f32(lv, oip.MEAN, oip.STD, dtype, mut), x, e, record=False)
    # resize in isolation: mean 0, std 1, fp32 gives level * (1/255.f); round(out * 255) recovers every level
    out = si.normalise_f32(np.arange(256)[:, None].repeat(3, 1), (0, 0, 0), (1, 1, 1), F32)
    assert np.array_equal(np.round(out * 255), np.arange(256)[:, None].repeat(3, 1))


# ------------------------------------------------------------------------------------------ old versus new
def _old_compare(got, want, exact_min=0.995, levels=3):
    """`_compare` of tests/test_gpu_input_pipeline.py and tests/test_gpu_mosaic.py -> passes"""
    got, want = torch.as_tensor(got).float(), torch.as_tensor(want).float()
    d = (got - want).abs()
    exact = float((d < 1e-5).float().mean())
    lim = (levels + 0.05) / 255 / 0.224
    return exact >= exact_min and float(d.max()) <= lim


OLD_SIZES = [(17, 301), (64, 64), (333, 500), (48, 40)]       # of tests/test_gpu_mosaic.py (seed 21), transformed to 96 as its g1 / g2 do
OLD_S = 96
OLD_PASSES = {"resize": [], "blend": ["gray_0299"], "hue": ["hue_nowrap"], "normalise": []}


def _old_jitter(i):
    return si.ORDERS[i % 8], (0.8 + 0.05 * i, 1.2 - 0.04 * i, 0.85 + 0.04 * i, -0.1 + 0.028 * i)


@pytest.fixture(scope="module")
def old_cases():
    imgs = si.smooth_images(21, OLD_SIZES)
    plain = [oip.transform_image(im, OLD_S, i % 2 == 0).numpy() for i, im in enumerate(imgs)]
    chain = [oip.transform_image(im, OLD_S, i % 2 == 0, *_old_jitter(i)).numpy() for i, im in enumerate(imgs)]
    return imgs, plain, chain


def _old_passes(old_cases, mut, chain, dtype=F32):
    """every image of the former test passes its `_compare` (bf16 as test_sampled_decisions_bf16_output does it)"""
    imgs, plain, full = old_cases
    ok = True
    for i, im in enumerate(imgs):
        order, fac = _old_jitter(i) if chain else ((), (1.0, 1.0, 1.0, 0.0))
        got = si.pipeline(im, OLD_S, i % 2 == 0, order, fac, dtype=dtype, mut=mut)
        want = torch.from_numpy((full if chain else plain)[i]).to(dtype).float()
        ok = ok and _old_compare(got, want, *((0.97, 6) if chain else (0.995, 3)))
    return ok


def test_the_former_limit_passes_the_honest_pipeline_and_the_listed_mutants(old_cases):
    assert _old_passes(old_cases, None, False) and _old_passes(old_cases, None, True) and _old_passes(old_cases, None, True, BF)
    passed = {
        "resize": [m for m in si.MUTANTS["resize"] if _old_passes(old_cases, m, False) and _old_passes(old_cases, m, True)],
        "blend": [m for m in dict.fromkeys(si.MUTANTS["brightness"] + si.MUTANTS["contrast"] + si.MUTANTS["saturation"])
                  if _old_passes(old_cases, m, True)],
        "hue": [m for m in si.MUTANTS["hue"] if _old_passes(old_cases, m, True)],
        "normalise": [m for m in si.MUTANTS["normalise"] if _old_passes(old_cases, m, True, BF)],
    }
    print(f"\n[strict_image] mutants the former limit passes: {passed}")
    assert passed == OLD_PASSES
    # ... and the strict sets fail each of them on the former tests' own images
    imgs = old_cases[0]
    for mut in OLD_PASSES["blend"] + OLD_PASSES["hue"]:
        hit = []
        for i, im in enumerate(imgs):
            lv = si.q_resize(si.resize_ref(im, OLD_S, OLD_S, i % 2 == 0)[0])
            for op in (1, 2, 3):
                f = si.HUE_FACTORS[0] if op == 3 else si.BLEND_FACTORS[0]
                got = si.op_f32(op, lv, f, mut)
                hit += si.failing(lambda: si.check_op(op, f"old image {i} {mut}", lv, f, got, oracle=False, record=False, cap=1.0))
        assert hit, mut
