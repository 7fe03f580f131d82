"""CPU tests of tests/strict_loss.py: what proves, without a GPU, that the derived per-element limits of the loss pass the
kernels' arithmetic and fail arithmetic that is subtly wrong.

Two stand-ins, both with NOTHING outside any limit on every case of tests/test_gpu_loss.py, in fp32 / bf16 / f16:
  (i)   oracle/loss.py under fp32 autograd, its gradient (times grad_scale, in fp32) rounded once to T, with the oracle's
        own fp32 box decode as pbox
  (ii)  strict_loss.evaluate() in fp32: the plain-torch restatement in the kernel's operation order (GT after GT, the
        closed-form qfl_elem), with its own fp32 decode
(on the CPU torch's vectorised exp is not bit-identical between two positions of a tensor, so the duplicated anchors'
pbox rows are copied, as the kernel's per-thread scalar code makes them.)  Every mutant of MUTANTS must raise
StrictMismatch in the family named beside it.  The float64 restatement is pinned to the oracle (value and gradient, fp32,
loss_small), and tests/test_oracle_golden.py pins the oracle to the reference's own outputs.

Recorded maxima of the stand-ins, largest share of the noise budget used ((|got - ref| - 1/2 ulp) / noise, limit 1; the
module prints the table when it finishes, run with -s): see STAND_IN_MAXIMA below."""
import contextlib

import pytest
import torch

import strict_compare as sc
import strict_loss as sl
from conftest import load_golden
from oracle import loss as ol

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [F32, BF, HF]
IDS = ["f32", "bf16", "f16"]
# N, A, nc, empty images: the shapes of tests/test_gpu_loss.py
SHAPES = [(1, 84, 1, ()), (3, 724, 8, (0,)), (3, 1032, 80, (2,)), (5, 1030, 8, (2,)), (3, 84, 8, (0, 1, 2)), (1, 724, 80, ()),
          (5, 84, 80, (0, 4)), (3, 1030, 1, (1,))]
FULL = (3, 724, 8, (0,))               # every built target set, an empty image, collisions, four tie pairs
STAND_IN_MAXIMA = """both stand-ins, every case of this module, 2026-10-19: loss_decode 0.229, loss_assign 0.000, loss_dense 0.246,
loss_box 0.684, loss_slot 0.263, loss_scalars 0.036"""


@pytest.fixture(autouse=True, scope="module")
def _threads_and_report():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    yield
    print("\n" + sc.report())


# ------------------------------------------------------------------------------------------ the stand-ins
def twin(case, pbox):
    for i, j in case.pairs:
        pbox[:, j] = pbox[:, i]
    return pbox


def stand_in_ii(case, mut=None, idx_mut=None):
    pbox = twin(case, sl.decode64(case, F32)[0])
    idx = sl.assign_cpu(case, pbox)
    if idx_mut is not None:
        idx = idx_mut(idx)
    r = sl.evaluate(case, idx, pbox, F32, mut)
    return {"out": r["out"], "dp": sl.round_to(r["dp"], case.dtype), "dp32": r["dp"], "pbox": pbox, "idx": idx}


def stand_in_i(case):
    p = case.preds.float().transpose(1, 2)
    pbox = twin(case, ol.decode_boxes(p[:, :, :64].reshape(case.N, -1, 4, 16), case.anchors.float().t(), case.strides.float().t()))
    idx = sl.assign_cpu(case, pbox)
    per_image, row = [], 0
    for g in case.gts:
        per_image.append(idx[row:row + g.shape[0]])
        row += g.shape[0]
    live = iter([v for v in per_image if v.numel()])
    saved = ol.assign
    ol.assign = lambda g, b: next(live)                       # the duplicated anchors: the assignment from the copied rows
    try:
        x = case.preds.float().clone().requires_grad_(True)
        tot, dfl, cls = ol.dfl_qfl_loss(x, case.gts, case.anchors.float(), case.strides.float(), case.nc,
                                        lambda_cls=case.lam[1], lambda_dfl=case.lam[0])
        (g,) = torch.autograd.grad(tot, x)
    finally:
        ol.assign = saved
    if case.grad_scale is not None:
        g = g * torch.tensor(case.grad_scale, dtype=F32)
    return {"out": torch.stack([tot, dfl, cls]).detach(), "dp": g.to(case.dtype), "pbox": pbox.detach(), "idx": idx}


def verify(case, r, old=None):
    return sl.verify(case, r["out"], r["dp"], r["pbox"], r["idx"], old)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"N{s[0]}-A{s[1]}-nc{s[2]}")
def test_stand_ins_have_nothing_outside(shape, dtype):
    case = sl.make_case(*shape[:3], dtype, shape[3])
    verify(case, stand_in_i(case))
    verify(case, stand_in_ii(case))


@pytest.mark.parametrize("dtype,scale", [(HF, 65536.0), (BF, 1024.0)], ids=["f16-65536", "bf16-1024"])
def test_stand_ins_with_grad_scale(dtype, scale):
    case = sl.make_case(*FULL[:3], dtype, FULL[3], grad_scale=scale)
    verify(case, stand_in_i(case))
    verify(case, stand_in_ii(case))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stand_ins_just_over_the_grid_cap(dtype):
    a = 2920 if dtype == F32 else 5832
    case = sl.make_case(5, a, 80, dtype, (), built=False, seed=3)
    verify(case, stand_in_ii(case))
    if dtype == BF:
        verify(case, stand_in_i(case))


def test_the_restatement_is_pinned_to_the_oracle_on_loss_small():
    """evaluate() in fp32 with idx from oracle.loss.assign against oracle/loss.py::dfl_qfl_loss under autograd: value and
    gradient to fp32 rounding (a few 2^-24 of each element; 1e-9 absolute for the gradients that are sums of cancelling terms)"""
    gd = load_golden("loss_small")
    gts = [gd["gt0"], gd["gt1"].reshape(0, 5), gd["gt2"]]
    case = sl.Case(gd["preds"].float(), gd["anchors"].float(), gd["strides"].float(), gts, 8, F32, "loss_small")
    p = case.preds.transpose(1, 2)
    pbox = ol.decode_boxes(p[:, :, :64].reshape(case.N, -1, 4, 16), case.anchors.t(), case.strides.t())
    idx = torch.cat([ol.assign(g[:, :2].float(), pbox[n, :, :2]) for n, g in enumerate(case.gts) if g.shape[0]])
    keys = (case.img * case.A + idx).tolist()
    assert len(set(keys)) < len(keys)                         # the collision on anchor 26 is in
    r = sl.evaluate(case, idx, pbox, F32)
    x = case.preds.clone().requires_grad_(True)
    tot, dfl, cls = ol.dfl_qfl_loss(x, case.gts, case.anchors, case.strides, 8)
    (g,) = torch.autograd.grad(tot, x)
    want = torch.stack([tot, dfl, cls]).detach()
    assert torch.allclose(r["out"], want, rtol=1e-6, atol=0), (r["out"], want)
    assert torch.allclose(r["dp"], g, rtol=2e-5, atol=1e-9), float((r["dp"] - g).abs().max())
    r64 = sl.evaluate(case, idx, pbox)                        # and the float64 evaluation is the same function
    assert torch.allclose(r64["dp"].float(), g, rtol=2e-5, atol=1e-9) and torch.allclose(r64["out"].float(), want, rtol=1e-6)


# ------------------------------------------------------------------------------------------ mutants
MUTANTS = {"iou_detached": "loss_box", "loser_without_iou_gradient": "loss_box", "first_gt_wins_the_slot": "loss_slot",
           "textbook_iou": "loss_box", "dfl_by_distinct_anchors": "loss_box", "empty_image_left_out": "loss_dense",
           "clamp_at_15": "loss_box", "tie_to_the_highest_index": "loss_assign", "tie_gradient_to_one_operand": "loss_box",
           "dense_times_1_plus_2^-7": "loss_dense", "grad_scale_after_the_rounding": "loss_dense", "slot_with_target_0": "loss_slot"}


@contextlib.contextmanager
def wrong_on_purpose():
    """no guard 'nowhere wider than before', and nothing recorded among the maxima"""
    saved = {k: list(v) for k, v in sc.OBSERVED.items()}
    sl.GUARD = False
    try:
        yield
    finally:
        sl.GUARD = True
        sc.OBSERVED.clear()
        sc.OBSERVED.update(saved)


def mutant(case, mut):
    if mut == "tie_to_the_highest_index":
        up = dict(case.pairs)
        return stand_in_ii(case, idx_mut=lambda idx: torch.tensor([up.get(int(k), int(k)) for k in idx]))
    if mut == "dense_times_1_plus_2^-7":
        r = stand_in_ii(case)
        r["dp32"][:, 64:] *= 1.0 + 2.0 ** -7
        r["dp"] = sl.round_to(r["dp32"], case.dtype)
        return r
    if mut == "grad_scale_after_the_rounding":
        r = stand_in_ii(case.with_(grad_scale=None))
        r["dp"] = (r["dp"].float() * case.grad_scale).to(case.dtype)
        return r
    return stand_in_ii(case, mut)


def caught_in(case, r):
    with wrong_on_purpose():
        return sl.failing_families(lambda: verify(case, r))


# one mutant is about one type: only f16 (5 exponent bits) loses a gradient that is scaled after its rounding; a power of two
# applied to a rounded bf16 or fp32 value is exact.  (1 + 2^-7 is one to two ulps of bf16, the coarsest type: it fails in all.)
ONE_TYPE = {"grad_scale_after_the_rounding": HF}
MUTANT_CASES = [(m, d) for m in MUTANTS for d in DTYPES if ONE_TYPE.get(m, d) == d]


@pytest.mark.parametrize("mut,dtype", MUTANT_CASES, ids=[f"{m}-{IDS[DTYPES.index(d)]}" for m, d in MUTANT_CASES])
def test_every_mutant_fails_in_its_family(mut, dtype):
    scale = 65536.0 if mut == "grad_scale_after_the_rounding" else None
    case = sl.make_case(*FULL[:3], dtype, FULL[3], grad_scale=scale)
    assert MUTANTS[mut] in caught_in(case, mutant(case, mut)), mut
    assert caught_in(case, stand_in_ii(case)) == []           # and the same call without the mutant passes


# ------------------------------------------------------------------------------------------ the gap this closes
def s640_case(dtype):
    """the inputs of test_loss_random_s640_shape (tests/test_gpu_kernels.py), seed 70"""
    from oracle.blocks import make_anchors
    g = torch.Generator().manual_seed(70)
    preds = torch.randn(4, 144, 8400, generator=g)
    preds[:, 64:] = preds[:, 64:] * 0.7 - 3.5
    a, s = make_anchors([(80, 80), (40, 40), (20, 20)], [8.0, 16.0, 32.0])
    gts = []
    for i in range(4):
        m = int(torch.randint(1, 21, (1,), generator=g))
        gts.append(torch.cat([torch.rand(m, 2, generator=g) * 640, torch.rand(m, 2, generator=g) * 256 + 8,
                              torch.randint(0, 80, (m, 1), generator=g).float()], 1))
    return sl.Case(preds, a.t().contiguous(), s.t().contiguous(), gts, 80, dtype, f"s640 seed 70 {str(dtype)[6:]}")


def old_check_passes(dp, want, dtype):
    err = float((dp.float() - want.float()).abs().max()) / float(want.float().abs().max())
    return err, err <= sl.OLD_TOL[dtype]


def test_the_former_limit_passes_two_mutants_the_strict_limit_fails():
    """max |dp - ref| / max |ref| <= 2^-6 on the seed-70 case in bf16: a loss whose IoU is detached (no IoU gradient reaches a
    box logit) moves the tensor by 6.4e-4 of its maximum, one whose whole dense class gradient is zero by 1.5e-3; both pass.
    The derived limits fail both, each in its family."""
    case = s640_case(BF)
    assert sl.guard_ok(case)
    good = stand_in_ii(case)
    want = good["dp32"]
    verify(case, good, old=sl.old_abs(want.double(), BF))     # with the guard: the new limit is nowhere wider than the former
    for mut, fam, moved in (("iou_detached", "loss_box", 6.4e-4), ("dense_zeroed", "loss_dense", 1.5e-3)):
        r = stand_in_ii(case, mut)
        err, ok = old_check_passes(r["dp"], want, BF)
        assert ok and err < 2.0 ** -6 / 4, (mut, err)
        assert 0.5 * moved < float((r["dp32"] - want).abs().max() / want.abs().max()) < 2.0 * moved, mut
        assert fam in caught_in(case, r), mut


# ------------------------------------------------------------------------------------------ the failure report
def test_a_failure_names_the_image_and_the_anchor_block():
    case = sl.make_case(*FULL[:3], BF, FULL[3])
    r = stand_in_ii(case)
    ref = sl.evaluate(case, r["idx"], r["pbox"])
    dp = r["dp"].clone()
    dp[2, 64 + 5, 333] *= 1.25                                # image 2, class 5, anchor 333: a dense class gradient
    with wrong_on_purpose(), pytest.raises(sl.StrictMismatch) as ei:
        sl.check_gradients(case, dp, ref)
    h = ei.value.hist
    assert ei.value.families == ["loss_dense"] and ei.value.count == 1
    assert set(h["image"]) == {2} and set(h["pixel_block"]) == {(2 * 724 + 333) // 16} and set(h["channel_block"]) == {0}, h
    k = int(r["idx"][0])                                      # a matched anchor of image 1: its box logits
    dp = r["dp"].clone()
    dp[1, 16:32, k] += 0.01
    with wrong_on_purpose(), pytest.raises(sl.StrictMismatch) as ei:
        sl.check_gradients(case, dp, ref)
    h = ei.value.hist
    assert ei.value.families == ["loss_box"] and set(h["image"]) == {1} and set(h["pixel_block"]) == {(724 + k) // 16}
    assert set(h["channel_block"]) == {1} and "anchor block" in str(ei.value)
    dp = r["dp"].clone()
    dp[1, 3, 700 if 700 not in r["idx"].tolist() else 701] = 1e-30       # an unmatched anchor's box logit: exactly zero or nothing
    with wrong_on_purpose(), pytest.raises(sl.StrictMismatch):
        sl.check_gradients(case, dp, ref)
