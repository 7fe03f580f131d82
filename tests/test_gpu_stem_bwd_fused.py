"""-m gpu: the stem's one-pass backward (ops.stem_bn_wgrad: BatchNorm sums and weight gradient from one pass over dout, y and
the image, no dz tensor) against the float64 reference and the derived per-element limit of tests/strict_stem_bwd.py, whose
power tests/test_stem_bwd_bound_cpu.py proves without a GPU.

y, scale, shift, mean, invstd come from the project's own stem_conv_fwd + bn_act_fwd_train; dout is seeded noise with a mean
(D carries the mean of dz).  The parent's path (bn_act_bwd_train + stem_wgrad) is held to the SAME limit against the SAME
reference; the two paths are never compared with each other.  Every element of dW, dgamma and dbeta is compared.

Under a captured step the op is covered by the train-loop tests (tests/test_gpu_train_loop.py: the runner captures the
whole backward, the stem's included, and compares its gradients with plain autograd); a hand-made capture of one autograd
node would test the capture of AccumulateGrad, not this op."""
import pytest
import torch

import strict_compare as sc
import strict_stem_bwd as ss
from test_gpu_kernels import DEV, dev, nhwc, ops

pytestmark = pytest.mark.gpu
DOUT_MEAN = 0.25


@pytest.fixture(autouse=True, scope="module")
def _print_observed_maxima():
    yield
    print("\n" + sc.report())


_CASES = {}


def case(key, n, h, w, cout, dtype, act, pdt=torch.float32, pad=0):
    """device inputs through the project's own forward, CPU copies and the float64 reference: built once, left unchanged"""
    if key in _CASES:
        return _CASES[key]
    o = ops()
    img, wt, gamma, beta, dout = ss.make_inputs(n, h, w, cout, dtype, pdt, seed=key if isinstance(key, int) else 10 + cout // 16)
    dout = nhwc((dout.float() + DOUT_MEAN).to(dtype), pad)            # pad: dout as a channel slice of a wider buffer
    g = {"img": img.to(DEV), "gamma": gamma.to(DEV), "beta": beta.to(DEV), "dout": dev(dout)}
    acc = o.bn_acc_new(cout, DEV)
    g["y"] = o.stem_conv_fwd(g["img"], o.stem_pack_weights(wt.to(DEV), dtype), cout, dtype, acc)
    rm, rv = torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV)
    _, g["mean"], g["invstd"], g["scale"], g["shift"] = o.bn_act_fwd_train(g["y"], acc, g["gamma"], g["beta"], rm, rv, 0.03, 1e-3, act)
    torch.cuda.synchronize()
    host = (img, dout, g["y"].cpu(), g["scale"].cpu(), g["shift"].cpu(), g["mean"].cpu(), g["invstd"].cpu(), gamma, act)
    g["host"] = host
    _CASES[key] = (g, ss.reference(*host), act)
    return _CASES[key]


def fused(g, act, w_dtype=torch.float32):
    return ops().stem_bn_wgrad(g["img"], g["dout"], g["y"], g["scale"], g["shift"], g["mean"], g["invstd"], g["gamma"], act, w_dtype)


def parent(g, act, w_dtype=torch.float32):
    o = ops()
    acc = o.bn_acc_new(g["y"].shape[1], DEV)
    dy, dgamma, dbeta = o.bn_act_bwd_train(g["dout"], g["y"], g["scale"], g["shift"], g["mean"], g["invstd"], g["gamma"], act, acc)
    return o.stem_wgrad(g["img"], dy, w_dtype), dgamma, dbeta


@pytest.mark.parametrize("i", range(len(ss.SHAPES)), ids=ss.IDS)
def test_one_pass_backward_within_the_derived_limit(i):
    g, ref, act = case(i, *ss.SHAPES[i])
    dw, dgamma, dbeta = fused(g, act)
    ex = ss.check(dw, dgamma, dbeta, ref, f"one pass {ss.IDS[i]}")
    print(f"\none pass {ss.IDS[i]}: excess {ex:.2f} x 2^-24 M")
    if not act:         # identity rounds nothing in this kernel: also inside the limit without the rounding term
        ss.check(dw, dgamma, dbeta, ss.reference(*g["host"], dz_exact=True), f"one pass, exact dz, {ss.IDS[i]}")


@pytest.mark.parametrize("i", range(len(ss.SHAPES)), ids=ss.IDS)
def test_three_launch_path_within_the_same_limit(i):
    g, ref, act = case(i, *ss.SHAPES[i])
    dw, dgamma, dbeta = parent(g, act)
    ss.check(dw, dgamma, dbeta, ref, f"three launches {ss.IDS[i]}")


@pytest.mark.parametrize("i", range(len(ss.SHAPES)), ids=ss.IDS)
def test_two_launches_give_the_same_bits(i):
    g, _, act = case(i, *ss.SHAPES[i])
    a, b = fused(g, act), fused(g, act)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("pdt,w_dtype", [(torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32)], ids=["bf16", "f32"])
@pytest.mark.parametrize("cout", [64, 96, 128])
def test_parameter_dtypes_channel_counts_and_a_sliced_dout(pdt, w_dtype, cout):
    """gamma / dgamma / dbeta and dW in the parameters' own dtype; the channel counts whose chunk walk leaves threads idle
    (96) or fills the LDS (128); dout a channel slice of a wider buffer"""
    g, ref, act = case(("p", pdt, cout), 2, 18, 270, cout, torch.bfloat16, 1, pdt, pad=16)
    dw, dgamma, dbeta = fused(g, act, w_dtype)
    assert dw.dtype == w_dtype and dgamma.dtype == pdt and dbeta.dtype == pdt
    ss.check(dw, dgamma, dbeta, ref, f"one pass cout {cout} w {w_dtype} p {pdt}")
    dw, dgamma, dbeta = parent(g, act, w_dtype)
    ss.check(dw, dgamma, dbeta, ref, f"three launches cout {cout} w {w_dtype} p {pdt}")


@pytest.mark.parametrize("switch", [True, False], ids=["one-pass", "three-launch"])
def test_conv_block_backward_takes_the_path_the_switch_names(switch, monkeypatch):
    """a ConvBnAct stem block through autograd: with the switch on its gradients ARE the op's outputs, with it off the
    parent's path runs (and the op does not)"""
    from src.hipops import functions as F_
    from src.model.model_blocks import Conv
    o = ops()
    calls = {}

    def spy(name):
        real = getattr(o, name)

        def wrapped(*a, **k):
            calls[name] = (a, real(*a, **k))
            return calls[name][1]
        monkeypatch.setattr(o, name, wrapped)
    for nm in ("stem_bn_wgrad", "stem_wgrad", "bn_act_bwd_train"):
        spy(nm)
    monkeypatch.setattr(F_, "STEM_BWD_FUSED", switch)
    monkeypatch.setattr(F_.BnArena, "current", F_.BnArena(DEV, F_.BnArena.elems_for([32])))     # as inside a Model pass
    torch.manual_seed(3)
    block = Conv(3, 32, torch.nn.SiLU(), 3, 2, 1).to(DEV).train()
    img = torch.randn(2, 3, 38, 70, generator=torch.Generator().manual_seed(4)) + 0.5
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = block(img.to(DEV))
    out.backward((torch.randn(out.shape, generator=torch.Generator().manual_seed(5)) + DOUT_MEAN).to(DEV, out.dtype))
    torch.cuda.synchronize()
    wg, gg, bg = block.conv.weight.grad, block.norm.weight.grad, block.norm.bias.grad
    if switch:
        assert set(calls) == {"stem_bn_wgrad"}
        (_, dout, y, scale, shift, mean, invstd, gamma, act, _), (dw, dgamma, dbeta) = calls["stem_bn_wgrad"]
    else:
        assert set(calls) == {"stem_wgrad", "bn_act_bwd_train"}
        (dout, y, scale, shift, mean, invstd, gamma, act, _), (_, dgamma, dbeta) = calls["bn_act_bwd_train"]
        dw = calls["stem_wgrad"][1]
    assert torch.equal(wg, dw) and torch.equal(gg, dgamma) and torch.equal(bg, dbeta)
    assert wg.shape == (32, 3, 3, 3) and wg.dtype == torch.float32
    ref = ss.reference(img, dout.cpu(), y.cpu(), scale.cpu(), shift.cpu(), mean.cpu(), invstd.cpu(), gamma.detach().cpu(), act)
    ss.check(wg, gg, bg, ref, f"block backward, switch {switch}")
