"""-m gpu: the loss kernels of csrc/loss.hip (k_front, k_assign, k_back) held to the derived per-element limits of
tests/strict_loss.py, stage by stage, at the smallest shapes where they can go wrong.

Every case is compared in all six families (loss_decode, loss_assign, loss_dense, loss_box, loss_slot, loss_scalars) from
the buffers the launch itself left in its workspace (pbox at byte 0, idx at byte N A 16), and additionally: two launches on
the same inputs are bit-identical, and `out` is bit-identical with and without the gradient and with and without grad_scale.
The cases build their own anchors and strides (strict_loss.make_case): A in {84, 724, 1032, 1030} (tail loop only; one
unrolled trip plus the tail; two trips plus 8; A % 8 = 4 -- scalar in 16 bit, vector in fp32 --, A % 8 = 0 -- vector in both
--, A % 4 = 2 -- scalar in both), nc in {1, 8, 80}, N in {1, 3, 5}, the first / a middle / the last / every image empty; the
target sets (collisions of two, of three, across more than four rows, more than 64 GTs in an image; exact distance ties in
every position of assign_wave; DFL targets below 0, above 14.99 and an exact integer; min/max ties, a touching and a
disjoint GT) are built and asserted on the CPU when the case is made."""
import os
import re

import pytest
import torch

import emulated_ops as emu
import strict_compare as sc
import strict_loss as sl

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF, HF = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF, HF]
IDS = ["f32", "bf16", "f16"]
# N, A, nc, empty images
SHAPES = [(1, 84, 1, ()), (3, 724, 8, (0,)), (3, 1032, 80, (2,)), (5, 1030, 8, (2,)), (3, 84, 8, (0, 1, 2)), (1, 724, 80, ()),
          (5, 84, 80, (0, 4)), (3, 1030, 1, (1,))]


@pytest.fixture(autouse=True, scope="module")
def _print_observed_maxima():
    yield
    print("\n" + sc.report())


def launch(case, want_grad=True, grad_scale="case"):
    """-> out (3,), dpreds or None, pbox (N, A, 4), idx (G,) on the CPU, as the launch left them"""
    from src.hipops import ops as o
    from src.model.losses import PackedTargets
    pk = PackedTargets([g.to(DEV) for g in case.gts], DEV)
    gs = case.grad_scale if grad_scale == "case" else grad_scale
    gsd = None if gs is None else torch.tensor([gs], dtype=F32, device=DEV)
    out, dp, ws = o.loss_fwd_bwd(case.preds.to(DEV), case.anchors.to(DEV), case.strides.to(DEV), *pk.as_tuple(), case.nc,
                                 case.lam[0], case.lam[1], want_grad, gsd)
    torch.cuda.synchronize()
    na = case.N * case.A
    pbox = ws[:na * 16].view(F32).view(case.N, case.A, 4).cpu()
    idx = ws[na * 16:na * 16 + 4 * max(pk.n_gt, 1)].view(torch.int32)[:pk.n_gt].cpu()
    return out.cpu(), None if dp is None else dp.cpu(), pbox, idx


def full_check(case):
    out, dp, pbox, idx = launch(case)
    for i, j in case.pairs:                                   # the duplicated anchors decode bit-identically
        assert torch.equal(pbox[:, i], pbox[:, j]), (i, j)
    assert bool(((idx >= 0) & (idx < case.A)).all())
    sl.verify(case, out, dp, pbox, idx)
    out2, dp2, pbox2, idx2 = launch(case)
    assert torch.equal(out, out2) and torch.equal(dp, dp2) and torch.equal(pbox, pbox2) and torch.equal(idx, idx2)
    out3, dp3, _, idx3 = launch(case, want_grad=False)
    assert dp3 is None and torch.equal(out, out3) and torch.equal(idx, idx3)
    other = None if case.grad_scale is not None else 1024.0
    out4, _, _, _ = launch(case, grad_scale=other)
    assert torch.equal(out, out4)
    return out, dp, pbox, idx


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"N{s[0]}-A{s[1]}-nc{s[2]}-empty{''.join(map(str, s[3])) or 'none'}")
def test_every_stage_within_its_limit(shape, dtype):
    n, a, nc, empty = shape
    case = sl.make_case(n, a, nc, dtype, empty)
    out, dp, pbox, idx = full_check(case)
    if len(empty) == n:
        assert idx.numel() == 0 and not bool(dp[:, :64].any())


@pytest.mark.parametrize("dtype,scale", [(HF, 65536.0), (BF, 1024.0)], ids=["f16-65536", "bf16-1024"])
def test_grad_scale_every_element_at_the_scaled_magnitude(dtype, scale):
    """the factor is applied in fp32 before the one rounding: every element within u_T of the SCALED float64 gradient"""
    case = sl.make_case(3, 724, 8, dtype, (0,), grad_scale=scale)
    out, dp, pbox, idx = full_check(case)
    assert bool(torch.isfinite(dp.float()).all())
    if dtype == HF:                                           # the values that would be subnormal or zero without the scale
        _, dp1, _, _ = launch(case, grad_scale=None)
        small = (dp1.float().abs() < 6e-5) & (dp.float() != 0)
        assert int(small.sum()) > 1000


def dense_blocks():
    src = os.path.join(os.path.dirname(__file__), "..", "custom-yolo-implmentation_amd", "csrc", "loss.hip")
    return int(re.search(r"constexpr int DENSE_BLOCKS = (\d+);", open(src).read()).group(1))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dense_pass_just_over_the_grid_cap(dtype):
    """N A (64 + nc) just over DENSE_BLOCKS * 256 * V elements: the grid is capped, the packets of the last blocks fall past
    the end and the guarded tail of the four-in-flight loop applies"""
    v = 4 if dtype == F32 else 8
    n, nc = 5, 80
    cap = dense_blocks() * 256 * v
    a = -(-cap // (n * (64 + nc)))
    a = -(-a // 8) * 8
    assert n * (a - 8) * (64 + nc) <= cap < n * a * (64 + nc)
    case = sl.make_case(n, a, nc, dtype, (), built=False, seed=3)
    out, dp, pbox, idx = launch(case)
    sl.verify(case, out, dp, pbox, idx)


def _non_finite_case(dtype, variant):
    case = sl.make_case(3, 724, 8, dtype, (1,) if variant == "empty" else (), built=False, seed=5)
    pbox = sl.decode64(case)[0]
    idx = sl.assign_cpu(case, pbox)
    img = case.img
    p = case.preds.float()
    if variant == "box":
        hit = 0
        m = int(idx[(img == hit).nonzero()[0, 0]])             # a matched anchor of image 0
        un = next(k for k in range(case.A) if k not in set(idx[img == hit].tolist()))
        p[hit, 3, m] = float("nan")
        p[hit, 40, un] = float("inf")
    elif variant == "empty":                                  # an image without GTs: nothing is matched there
        hit = 1
        p[hit, 20, 100] = float("nan")
    else:
        hit = 1
        r = int((img == hit).nonzero()[0, 0])
        p[hit, 64 + int(case.gt[r, 4]), int(idx[r])] = float("inf")     # the slot's own class logit
        p[hit, 64 + 2, 7] = float("-inf")
        p[hit, 64 + 5, 300] = float("inf")
    bad = sl.Case(p, case.anchors.float(), case.strides.float(), case.gts, case.nc, dtype, case.what + " non-finite " + variant)
    return bad, hit


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("variant", ["box", "cls", "empty"])
def test_a_non_finite_input_never_becomes_a_finite_gradient(variant, dtype):
    """fp16 loss scaling depends on non-finite values surfacing.  One image at a time gets a NaN and a +inf box logit (a
    matched and an unmatched anchor), +-inf class logits, or a NaN box logit in an image without GTs: wherever the fp32 CPU
    oracle's dpreds or loss is non-finite the kernel's is too, idx stays in range and is argmin's NaN-wins choice on the
    kernel's pbox, and the images without a non-finite input keep their dpreds within the limits.  (Every index stays in
    range by construction: no fault.)  The `box` and `empty` variants are the regression test of k_back's NaN sweep: before
    it, the NaN logit of an anchor that ends up unmatched (every GT goes to the lowest anchor with a NaN box) got gradient 0."""
    case, hit = _non_finite_case(dtype, variant)
    out, dp, pbox, idx = launch(case)
    assert bool(((idx >= 0) & (idx < case.A)).all())
    assert torch.equal(idx.long(), sl.assign_cpu(case, pbox))
    gt = case.gt
    offs = torch.tensor([0] + [g.shape[0] for g in case.gts]).cumsum(0).int()
    ref_out, ref_dp, _ = emu.loss_fwd_bwd(case.preds.float(), case.anchors.float(), case.strides.float(), gt, offs, case.img.int(),
                                          gt.shape[0], case.nc, case.lam[0], case.lam[1], True)
    nf = ~torch.isfinite(ref_dp)
    assert not bool((nf & torch.isfinite(dp.float())).any()), \
        f"finite where the oracle is not: {(nf & torch.isfinite(dp.float())).nonzero()[:16].tolist()}"
    assert not bool((~torch.isfinite(ref_out) & torch.isfinite(out)).any()), (out, ref_out)
    if variant == "box":
        assert int(nf.sum()) >= 64 and not bool(torch.isfinite(out[0]))
    if variant == "empty":                                    # autograd's softmax backward: p (g - sum g p) with p = NaN
        assert int(nf[hit, 16:32, 100].sum()) == 16
    clean = [i for i in range(case.N) if i != hit]
    sub = sl.Case(case.preds[clean].float(), case.anchors.float(), case.strides.float(), [case.gts[i] for i in clean], case.nc,
                  dtype, case.what + f" images {clean}")
    sub.n_mean = case.N
    rows = torch.cat([(case.img == i).nonzero().flatten() for i in clean])
    ref = sl.evaluate(sub, idx[rows].long(), pbox[clean])
    sl.check_gradients(sub, dp[clean], ref)
