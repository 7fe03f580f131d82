"""CPU tests of tests/strict_move.py: what proves, without a GPU, that the exact class and the derived limits of the pool /
upsample / copy / fan-in / cast family pass honest arithmetic and fail arithmetic that is subtly wrong.

Stand-ins, both with NOTHING outside any limit on the shapes of tests/test_gpu_move.py, in fp32 / bf16 / f16:
  (i)   tests/emulated_ops.py (ATen's pool and its flat indices, fp32 scatter_add / sum, one rounding)
  (ii)  strict_move's own sums in fp32 in the REVERSE order (the pool's contributions last tap first, add_n's sources
        last to first), one rounding
The exact-class references are pinned to ATen: F.max_pool2d(return_indices=True) in value and index (ties, NaN, +-inf,
all -inf windows, maps narrower than the window), F.interpolate, .to().  Every mutant of MUTANTS must raise StrictMismatch
in the family named beside it; mutants 9 and 10 assert that they really leave the limit on a counted number of elements.

Recorded maxima of the stand-ins, share of gamma_{K-1} M used (limit 1; the module prints the table, run with -s): see
STAND_IN_MAXIMA."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import emulated_ops as emu
import strict_compare as sc
import strict_move as sm

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [F32, BF, HF]
IDS = ["f32", "bf16", "f16"]
STAND_IN_MAXIMA = """both stand-ins, every case of this module, 2026-10-19: move_pool 0.478, move_up 0.393, move_copy 0.000,
move_add 0.424, move_chain 0.390 (of the propagated bound)"""


@pytest.fixture(autouse=True, scope="module")
def _threads_and_report():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    yield
    print("\n" + sc.report() + "\n" + sm.report())


def sid(s):
    return "x".join(map(str, s))


# ------------------------------------------------------------------------------------------ the references are ATen's
def _pin_input(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(*shape, generator=g) * 2).round().div(2).double()
    n, c, h, w = shape
    x[0, 0, 0, 0] = float("nan")
    x[n - 1, c - 1, h - 1, w - 1] = float("inf")
    x[0, c - 1, h // 2, w // 2] = float("-inf")
    if c > 2:
        x[0, 1] = float("-inf")
        x[n - 1, 1, h - 1, 0] = float("nan")
    elif n > 1:
        x[1, 0] = float("-inf")
    return x


@pytest.mark.parametrize("shape", [(2, 3, 9, 10), (1, 2, 1, 1), (1, 2, 1, 7), (1, 2, 6, 1), (2, 2, 3, 4)] + sm.POOL_SHAPES, ids=sid)
def test_the_pool_reference_is_aten_in_value_and_index(shape):
    for seed in (0, 1):
        x = _pin_input(shape, seed)
        val, idx = sm.pool_ref(x)
        want, widx = F.max_pool2d(x, 5, 1, 2, return_indices=True)
        assert torch.equal(sm.bits(val), sm.bits(want))
        assert torch.equal(sm.aten_index(idx), widx)
        ties = sm.pool_ref(x, "tie_last")[1]
        assert shape[2] * shape[3] < 12 or not torch.equal(ties, idx)      # the inputs do hold ties


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_pool_backward_reference_is_autograd(dtype):
    x = sm.grid((2, 24, 9, 10), 40, dtype, edges=False).double().requires_grad_(True)
    d = sm.smooth((2, 24, 9, 10), 41, dtype, edges=False).double()
    (want,) = torch.autograd.grad(F.max_pool2d(x, 5, 1, 2), x, d)
    s, m, k = sm.pool_bwd_ref(d, sm.pool_ref(x)[1])
    assert torch.equal(s, want) or float((s - want).abs().max()) <= 1e-12      # the same terms; float64 order may differ
    assert int(k.sum()) == d.numel() and int(k.max()) > 4 and int((k == 0).sum()) > 0


def test_upsample_and_cast_references_are_aten():
    x = sm.grid((2, 12, 5, 6), 3, F32)
    assert torch.equal(sm.bits(sm.up_ref(x)), sm.bits(F.interpolate(x, scale_factor=2.0, mode="nearest")))
    d = sm.smooth((2, 12, 4, 6), 4, F32, edges=False).double()
    s, m, k = sm.sum_ref(sm.up_bwd_terms(d))
    want = d.view(2, 12, 2, 2, 3, 2).sum((3, 5))                   # the 2x2 block sum
    assert k == 4 and float((s - want).abs().max()) <= 1e-14 and torch.equal(m, d.abs().view(2, 12, 2, 2, 3, 2).sum((3, 5)))
    src = torch.cat([sm.smooth((1, 8, 4, 4), 5, F32).flatten(), torch.tensor([1e-6, -3e-7, 6e-8, 65520.0, 1e39, 1.0 + 2.0 ** -8])])
    for d in DTYPES:
        assert torch.equal(sm.bits(sm.cast_ref(src, d)), sm.bits(src.to(d)))
        assert torch.equal(sm.bits(sm.cast_ref(src, d, 0.125)), sm.bits((src * 0.125).to(d)))


# ------------------------------------------------------------------------------------------ the stand-ins
def pool_stand_ins(x, dout, base, dtype):
    """-> list of (out, idx (kh * 5 + kw), dx) per stand-in"""
    val, aidx = F.max_pool2d(x.float(), 5, 1, 2, return_indices=True)
    ridx = sm.pool_ref(x)[1]
    assert torch.equal(sm.aten_index(ridx), aidx)
    dx1 = emu.maxpool5_bwd(dout, aidx, None if base is None else base.clone())
    dx2 = sm.pool_bwd_ref(dout, ridx, base, acc=F32, order=range(24, -1, -1))[0].to(dtype)
    return [(val.to(dtype), ridx, dx1), (val.to(dtype), ridx, dx2)]


POOL_CASES = [(s, d) for s in sm.POOL_SHAPES + [sm.SLICE_SHAPE, sm.SPPF_SHAPE] for d in DTYPES] + \
    [(sm.big_shape(d), d) for d in (F32, BF)]       # the second-trip shapes: the same arithmetic, two types are enough here


@pytest.mark.parametrize("shape,dtype", POOL_CASES, ids=[f"{sid(s)}-{IDS[DTYPES.index(d)]}" for s, d in POOL_CASES])
def test_pool_stand_ins_have_nothing_outside(shape, dtype):
    x, dout, base = sm.grid(shape, 40, dtype), sm.smooth(shape, 41, dtype), sm.smooth(shape, 42, dtype)
    for b in (None, base):
        for out, idx, dx in pool_stand_ins(x, dout, b, dtype):
            ridx = sm.check_pool_fwd(x, out, idx, f"pool {shape}")
            sm.check_pool_bwd(dout, ridx, dx, f"pool bwd {shape} acc={b is not None}", b)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", sm.UP_SHAPES + [sm.SLICE_SHAPE], ids=sid)
def test_upsample_stand_ins_have_nothing_outside(shape, dtype):
    n, c, h, w = shape
    x, dout, base = sm.grid(shape, 43, dtype), sm.smooth((n, c, 2 * h, 2 * w), 44, dtype), sm.smooth(shape, 45, dtype)
    sm.check_up_fwd(x, emu.upsample2x_fwd(x), f"up {shape}")
    for b in (None, base):
        sm.check_up_bwd(dout, emu.upsample2x_bwd(dout, None if b is None else b.clone()), f"up bwd {shape}", b)
        ts = sm.up_bwd_terms(dout, b)
        sm.check_up_bwd(dout, sm.sum_ref(ts, F32, range(len(ts) - 1, -1, -1))[0].to(dtype), f"up bwd reversed {shape}", b)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", sm.COPY_SHAPES, ids=sid)
def test_copy_and_add_stand_ins_have_nothing_outside(shape, dtype):
    src, dst = sm.smooth(shape, 46, dtype), sm.smooth(shape, 47, dtype)
    for acc in (False, True):
        d = dst.clone()
        emu.copy_channels(src, d, acc)
        sm.check_copy(src, dst, d, f"copy {shape} acc={acc}", acc)
    for k in (2, 3, 4):
        xs = sm.cancel([sm.smooth(shape, 50 + i, dtype) for i in range(k)])
        sm.check_add(xs, emu.add_n(xs), f"add_n {k} {shape}")
        sm.check_add(xs, sm.sum_ref(xs, F32, range(k - 1, -1, -1))[0].to(dtype), f"add_n {k} reversed {shape}")


def test_second_trip_shapes_of_upsample_copy_and_add_stand_ins():
    """the shapes with more than 1,048,576 work items, bf16: the same arithmetic at the size the GPU module uses"""
    shape = sm.big_shape(BF)
    n, c, h, w = shape
    x = sm.grid((n, c, h // 2, w // 2), 43, BF)
    sm.check_up_fwd(x, emu.upsample2x_fwd(x), "up big")
    dout, base = sm.smooth((n, c, 2 * h, 2 * w), 44, BF), sm.smooth(shape, 45, BF)
    sm.check_up_bwd(dout, emu.upsample2x_bwd(dout, base.clone()), "up bwd big", base)
    src, dst = sm.smooth(shape, 46, BF), sm.smooth(shape, 47, BF)
    d = dst.clone()
    emu.copy_channels(src, d, True)
    sm.check_copy(src, dst, d, "copy big", True)
    xs = sm.cancel([sm.smooth(shape, 50 + i, BF) for i in range(3)])
    sm.check_add(xs, emu.add_n(xs), "add_n big")


SIZES = [1, 7, 8, 9, 4095, 4096, 4097, 8195, 5000]


@pytest.mark.parametrize("scale", [1.0, 0.125, 1.0 / 3.0])
@pytest.mark.parametrize("dst", DTYPES, ids=IDS)
@pytest.mark.parametrize("src", DTYPES, ids=IDS)
def test_bucket_copy_stand_in_is_the_exact_rounding_rule(src, dst, scale):
    srcs = [sm.edge_vals((n,), 90 + i, src) for i, n in enumerate(SIZES)]
    dsts = [torch.full((n,), sm.SENTINEL, dtype=dst) for n in SIZES]
    emu.bucket_copy({"srcs": srcs, "dsts": dsts}, scale)
    for s_, d_ in zip(srcs, dsts):
        sm.check_cast(s_, d_, f"bucket_copy {src} -> {dst} x {scale:g}", scale)
        assert torch.equal(sm.bits(d_), sm.bits((s_.float() * torch.tensor(scale, dtype=F32)).to(dst)))


def chain_stand_in(x, g, dtype, order):
    """three launches, each an fp32 sum rounded once to T, reading what the one before stored"""
    c = x.shape[1]
    y1, i1 = sm.pool_ref(x)
    y2, i2 = sm.pool_ref(y1)
    y3, i3 = sm.pool_ref(y2)
    v = g[:, 3 * c:]
    for j, ik in ((2, i3), (1, i2), (0, i1)):
        v = sm.pool_bwd_ref(v, ik, g[:, j * c:(j + 1) * c], acc=F32, order=order)[0].to(dtype)
    return v


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 16, 12, 12), (2, 8, 3, 4)], ids=sid)
def test_chain_stand_ins_and_the_reference_is_autograd(shape, dtype):
    n, c, h, w = shape
    x, g = sm.grid(shape, 60, dtype), sm.smooth((n, 4 * c, h, w), 61, dtype)
    for order in (None, range(24, -1, -1)):
        _, r = sm.check_chain(x, g, chain_stand_in(x, g, dtype, order), f"chain {shape}")
    xe, ge = sm.grid(shape, 60, dtype, edges=False).double().requires_grad_(True), sm.smooth((n, 4 * c, h, w), 61, dtype, edges=False)
    y1 = F.max_pool2d(xe, 5, 1, 2)
    y2 = F.max_pool2d(y1, 5, 1, 2)
    (want,) = torch.autograd.grad(torch.cat([xe, y1, y2, F.max_pool2d(y2, 5, 1, 2)], 1), xe, ge.double())
    v0 = sm.chain_ref(xe, ge, dtype)["v0"]
    assert float((v0 - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ------------------------------------------------------------------------------------------ mutants
@contextlib.contextmanager
def wrong_on_purpose():
    """no guard 'nowhere wider than before', and nothing recorded among the maxima"""
    saved = {k: list(v) for k, v in sc.OBSERVED.items()}
    saved_exact = {k: list(v) for k, v in sm.EXACT.items()}
    sm.GUARD = False
    try:
        yield
    finally:
        sm.GUARD = True
        sc.OBSERVED.clear()
        sc.OBSERVED.update(saved)
        sm.EXACT.clear()
        sm.EXACT.update(saved_exact)


def caught(fn):
    with wrong_on_purpose():
        return sm.failing_families(fn)


def truncate(v32, dtype):
    """fp32 -> bf16 / f16 by dropping the low bits (round toward zero)"""
    drop = 16 if dtype == BF else 13
    return ((v32.contiguous().view(torch.int32) >> drop) << drop).view(F32).to(dtype)


def outside(mut, ref, mass, k, dtype):
    """number of finite elements of the mutant beyond 1/2 ulp + gamma_{K-1} M"""
    m = mut.double()
    lim = 0.5 * sm.ulp(torch.maximum(ref.abs(), m.abs()), dtype) + sm.gamma(k - 1) * mass
    return int(((m - ref).abs() > lim)[torch.isfinite(ref)].sum())


POOL_MUTANTS = {"tie_last": "pool_idx", "fmax": "pool_idx", "pad_zero": "pool_idx", "clip_right": "pool_idx"}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mut", list(POOL_MUTANTS))
def test_pool_forward_mutants_fail_on_the_index(mut, dtype):
    """1 tie takes the last maximum, 2 NaN not propagated, 3 padding counted as 0 (the all-negative channel), 4 the window one
    tap short at the right border"""
    shape = (2, 24, 9, 10)
    x = sm.grid(shape, 40, dtype)
    val, idx = sm.pool_ref(x, mut)
    assert POOL_MUTANTS[mut] in caught(lambda: sm.check_pool_fwd(x, val.to(dtype), idx, mut))
    val, idx = sm.pool_ref(x)
    assert caught(lambda: sm.check_pool_fwd(x, val.to(dtype), idx, "honest")) == []


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mut", ["swap", "no_base", "base_twice"])
def test_pool_backward_mutants_fail_in_move_pool(mut, dtype):
    """5 kh and kw swapped in the routing test, 6 acc_into's base dropped / added twice"""
    shape = (2, 24, 9, 10)
    x, dout, base = sm.grid(shape, 40, dtype), sm.smooth(shape, 41, dtype), sm.smooth(shape, 42, dtype)
    ridx = sm.pool_ref(x)[1]
    dx = sm.pool_bwd_ref(dout, ridx, base, acc=F32, mut=mut)[0].to(dtype)
    assert caught(lambda: sm.check_pool_bwd(dout, ridx, dx, mut, base)) == ["move_pool"]
    dx = sm.pool_bwd_ref(dout, ridx, base, acc=F32)[0].to(dtype)
    assert caught(lambda: sm.check_pool_bwd(dout, ridx, dx, "honest", base)) == []


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_upsample_mutants_fail_in_move_up(dtype):
    """7 the backward sums three of the four, 8 the forward reads (oh + 1) >> 1"""
    shape = (2, 12, 5, 6)
    x, dout = sm.grid(shape, 43, dtype), sm.smooth((2, 12, 10, 12), 44, dtype)
    three = sm.sum_ref(sm.up_bwd_terms(dout, mut="three"), F32)[0].to(dtype)
    assert caught(lambda: sm.check_up_bwd(dout, three, "three of four")) == ["move_up"]
    assert caught(lambda: sm.check_up_fwd(x, sm.up_ref(x, "round_up"), "(oh + 1) >> 1")) == ["move_up"]
    assert caught(lambda: sm.check_up_fwd(x, sm.up_ref(x), "honest")) == []


@pytest.mark.parametrize("dtype", [BF, HF], ids=IDS[1:])
def test_add_n_rounding_after_every_add_fails_in_move_add(dtype):
    """9: a 16-bit accumulator.  (In fp32 the mutant IS the kernel.)"""
    shape = (2, 16, 5, 7)
    xs = sm.cancel([sm.smooth(shape, 50 + i, dtype) for i in range(4)])
    acc = xs[0]
    for x in xs[1:]:
        acc = (acc.float() + x.float()).to(dtype)
    s, m, k = sm.sum_ref(xs)
    assert outside(acc, s, m, k, dtype) > 50
    assert caught(lambda: sm.check_add(xs, acc, "rounded after every add")) == ["move_add"]


@pytest.mark.parametrize("dtype", [BF, HF], ids=IDS[1:])
def test_accumulate_that_truncates_fails_in_move_copy(dtype):
    """10: round toward zero instead of to nearest even"""
    shape = (2, 16, 5, 7)
    src, dst = sm.smooth(shape, 46, dtype), sm.smooth(shape, 47, dtype)
    got = truncate(src.float() + dst.float(), dtype)
    s, m, k = sm.sum_ref([src, dst])
    assert outside(got, s, m, k, dtype) > 100               # of 1120: the sums that are inexact in T and lose more than half a spacing
    assert caught(lambda: sm.check_copy(src, dst, got, "truncating accumulate", True)) == ["move_copy"]


@pytest.mark.parametrize("dst", [BF, HF], ids=IDS[1:])
def test_cast_and_bucket_copy_mutants_fail_in_the_exact_class(dst):
    """11 the cast maps NaN to inf, 12 the scale applied after the rounding to the destination type, 13 the last n % 8
    elements not copied"""
    src = sm.smooth((1, 8, 25, 41), 70, F32).flatten()[:8195]
    honest = sm.cast_ref(src, dst, 1.0 / 3.0)
    assert caught(lambda: sm.check_cast(src, honest, "honest", 1.0 / 3.0)) == []
    nan_inf = torch.where(torch.isnan(src), torch.full_like(src, float("inf")), src).to(dst)
    assert caught(lambda: sm.check_cast(src, nan_inf, "NaN -> inf")) == ["exact"]
    late = (src.to(dst).float() * torch.tensor(1.0 / 3.0)).to(dst)
    assert int((sm.bits(late) != sm.bits(honest)).sum()) > 100
    assert caught(lambda: sm.check_cast(src, late, "scaled after the rounding", 1.0 / 3.0)) == ["exact"]
    short = torch.full_like(honest, sm.SENTINEL)
    short[:8195 & ~7] = honest[:8195 & ~7]
    assert caught(lambda: sm.check_cast(src, short, "tail dropped", 1.0 / 3.0)) == ["exact"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_store_past_the_slice_fails_the_guard(dtype):
    """14: a store 8 wide on a 6-channel slice"""
    buf = torch.full((2, 16, 5, 7), sm.SENTINEL, dtype=dtype)
    src = sm.smooth((2, 6, 5, 7), 46, dtype)
    buf[:, 4:10] = src
    assert caught(lambda: sm.assert_guard(buf, 4, 10, "honest")) == []
    buf[:, 4:12] = torch.cat([src, src[:, :2]], 1)
    assert caught(lambda: sm.assert_guard(buf, 4, 10, "8 wide on 6 channels")) == ["guard"]
    assert caught(lambda: sm.check_copy(src, None, buf[:, 4:10], "the slice itself is right", False)) == []


# ------------------------------------------------------------------------------------------ the gap this closes
def test_the_former_limit_passes_a_misrouted_gradient_the_strict_limit_fails():
    """the bf16 tie case of test_maxpool5_and_upsample (tests/test_gpu_kernels.py, seeds 40 / 41): ONE window's gradient
    (|dout| about 0.05) sent to the neighbouring tap.  check() allows 4 ulps of the tensor's largest element, 2^-5 max|dx|,
    about 0.1 here: it passes.  The derived limit fails it on the pixels it touches."""
    g = torch.Generator().manual_seed(40)
    x = (torch.randn(2, 24, 9, 10, generator=g) * 2).round().div(2).to(BF)
    g = torch.Generator().manual_seed(41)
    dout = torch.randn(2, 24, 9, 10, generator=g).to(BF)
    ridx = sm.pool_ref(x)[1]
    good = sm.pool_bwd_ref(dout, ridx, acc=F32)[0].to(BF)
    sm.check_pool_bwd(dout, ridx, good, "honest, with the guard 'nowhere wider than check()'")
    cand = ((dout[1, 5].float().abs() - 0.05).abs() + 100.0 * ((ridx[1, 5] % 5) == 4)).flatten()      # a window whose tap has a right neighbour
    p = int(cand.argmin())
    oh, ow = divmod(p, 10)
    wrong = ridx.clone()
    wrong[1, 5, oh, ow] += 1
    bad = sm.pool_bwd_ref(dout, wrong, acc=F32)[0].to(BF)
    moved = float((bad.float() - good.float()).abs().max())
    old = sm.OLD_TOL[BF] * 2.0 * float(good.float().abs().max())
    assert 0.02 < moved < 0.1 and moved <= old, (moved, old)         # check(mult=2) passes it
    with wrong_on_purpose(), pytest.raises(sm.StrictMismatch) as ei:
        sm.check_pool_bwd(dout, ridx, bad, "one window misrouted")
    assert ei.value.count >= 1 and set(ei.value.hist["image"]) == {1} and set(ei.value.hist["channel_block"]) == {0}


# ------------------------------------------------------------------------------------------ the failure report
def test_a_failure_names_the_image_the_pixel_block_and_the_channel_block():
    x = sm.grid((2, 24, 9, 10), 40, BF)
    val, idx = sm.pool_ref(x)
    idx[1, 17, 4, 3] += 1
    with wrong_on_purpose(), pytest.raises(sm.StrictMismatch) as ei:
        sm.check_pool_fwd(x, val.to(BF), idx, "one argmax off")
    e = ei.value
    assert e.families == ["pool_idx"] and e.count == 1 and e.hist["image"] == {1: 1} and e.hist["channel_block"] == {1: 1}
    assert e.hist["pixel_block"] == {(90 + 4 * 10 + 3) // 16: 1} and "by 16-pixel block" in str(e)
    flat = sm.smooth((1, 8, 5, 5), 1, F32).flatten()
    got = flat.to(HF)
    got[37] = 0.5
    with wrong_on_purpose(), pytest.raises(sm.StrictMismatch) as ei:
        sm.check_cast(flat, got, "flat buffer")
    assert ei.value.hist["pixel_block"] == {2: 1}
