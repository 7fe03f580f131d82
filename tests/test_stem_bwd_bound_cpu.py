"""CPU proof of tests/strict_stem_bwd.py: an fp32 emulation of the one-pass stem backward (csrc/stem.hip: dz in fp32, one
rounding to T, fp32 sums per workgroup -- here: per image --, the combination and dW = A G1 + B G2 + D G3 in double) has
nothing outside the limit on the four shapes of the GPU test, and the mistakes this kernel invites fall outside it.

What the limit sees, measured here (worst |error| / limit over dW; the tests print it, run with -s):
  dout shifted by one image row     far outside on every shape (no relation between dz and X is left)
  D G3 dropped                      outside on every shape (tens to hundreds of limits at a dout mean of 0.25)
  padded pixels counted in G3       outside wherever the tile holds a pixel past the image end that has a tap inside it (H even
                                    with OH odd, or W even): three of the four shapes.  At 37 x 261 (H and W odd) row 2 OH - 1 = H
                                    and column 2 OW - 1 = W lie outside the image: the mutant is the same arithmetic, nothing
                                    to see; the test asserts exactly that.
  unrounded image                   NOT visible under SiLU, and that is a property of the limit, not a gap in the test: the
                                    error sum dz (X - Xh) is at most u_T sum |dz| |X|, the very term the limit grants for the
                                    rounding of dz.  Under identity dz = dout is a value of T and the one-pass kernel is held to
                                    the limit WITHOUT that term (reference(dz_exact=True)): there the mutant is outside on all
                                    four geometries -- asserted on the identity shape of the list and on the identity variants
                                    of the other three (5 to 900 limits)."""
import pytest
import torch

import strict_bn as sb
import strict_compare as sc
import strict_stem_bwd as ss

MUTANTS = ("drop_DG3", "padded_pixels", "unrounded_image", "dout_row_shift")
DOUT_MEAN = 0.25        # the mean of dz is what D carries: the GPU test's dout has it too


@pytest.fixture(autouse=True, scope="module")
def _threads():
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    yield
    print("\n" + sc.report())


_CASES = {}


def case(i, act=None):
    """inputs, forward stand-in and reference of shape i (act: override), built once and left unchanged"""
    n, h, w, cout, dtype, a = ss.SHAPES[i]
    a = a if act is None else act
    if (i, a) not in _CASES:
        img, wt, gamma, beta, dout = ss.make_inputs(n, h, w, cout, dtype, seed=i)
        dout = (dout.float() + DOUT_MEAN).to(dtype)
        y, scale, shift, mean, invstd = ss.cpu_forward(img, wt, gamma, beta, dtype)
        args = (img, dout, y, scale, shift, mean, invstd, gamma, a)
        _CASES[(i, a)] = (args, ss.reference(*args, dz_exact=not a))   # the one-pass arithmetic: identity rounds nothing
    return _CASES[(i, a)]


def tile_pixels(xi, oh, ow):
    """unfold of every pixel a tile holds that can have a tap inside the image: (N, 27, OH + er, OW + ec) -- output row OH
    exists in a half-empty row pair (OH odd), column OW in a partial 128-pixel segment"""
    er, ec = oh % 2, int(ow % 128 != 0)
    xp = ss.unfold(torch.nn.functional.pad(xi, (0, 2, 0, 2))).reshape(xi.shape[0], 27, oh + 1, ow + 1)
    return xp[:, :, :oh + er, :ow + ec]


def emulate(img, dout, y, scale, shift, mean, invstd, gamma, act, w_dtype=torch.float32, mut=None):
    """the kernel's arithmetic in fp32 torch code: a 'workgroup' is one image"""
    T = y.dtype
    n, c, oh, ow = y.shape
    h, w = img.shape[2:]
    d, a = dout.float(), y.float()
    if mut == "dout_row_shift":
        d = torch.roll(d, 1, 2)
    if act:
        z = a * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        s = 1.0 / (1.0 + torch.exp(-z))
        dz = d * (s * (1.0 + z * (1.0 - s)))
    else:
        dz = d
    s_ = dz.sum((2, 3)).double().sum(0)                       # fp32 per workgroup, double across
    q_ = (dz * a).sum((2, 3)).double().sum(0)
    xi = img if mut == "unrounded_image" else img.to(T).float()
    x = ss.unfold(xi)
    g1 = torch.einsum("ncp,nkp->nck", dz.to(T).float().reshape(n, c, -1), x).double().sum(0)
    g2 = torch.einsum("ncp,nkp->nck", a.reshape(n, c, -1), x).double().sum(0)
    if mut == "padded_pixels":
        # every pixel of the tile: output row OH exists in a half-empty row pair, column OW in a partial segment
        x = tile_pixels(xi, oh, ow).reshape(n, 27, -1)
    g3 = x.sum(2).double().sum(0)[None]
    is_, mu = invstd.double(), mean.double()
    cnt = float(n * oh * ow)
    dgam = is_ * (q_ - mu * s_)
    k0, c1, c2 = gamma.double() * is_, s_ / cnt, dgam / cnt
    A, B, D = k0[:, None], (-k0 * c2 * is_)[:, None], (-k0 * c1 + k0 * c2 * mu * is_)[:, None]
    dw = A * g1 + B * g2 + (0.0 if mut == "drop_DG3" else D * g3)
    return dw.float().to(w_dtype).reshape(c, 3, 3, 3), dgam.float().to(gamma.dtype), s_.float().to(gamma.dtype)


def share(dw, ref):
    """worst |error| / limit over dW"""
    r, m, e = ref["dw"]
    g = dw.double()
    lim = 0.5 * sc.ulp(torch.maximum(r.abs(), g.abs()), dw.dtype) + sc.C["stem_wgrad"] * sc.U24 * m + e
    return float(((g - r).abs() / lim).max())


@pytest.mark.parametrize("i", range(len(ss.SHAPES)), ids=ss.IDS)
def test_emulation_of_the_fused_arithmetic_passes(i):
    args, ref = case(i)
    dw, dgamma, dbeta = emulate(*args)
    print(f"\n{ss.IDS[i]}: emulation uses {share(dw, ref):.3f} of the limit")
    ss.check(dw, dgamma, dbeta, ref, ss.IDS[i])


@pytest.mark.parametrize("w_dtype,pdt", [(torch.bfloat16, torch.bfloat16), (torch.float32, torch.float32)], ids=["bf16", "f32"])
def test_emulation_passes_in_the_parameters_own_dtypes(w_dtype, pdt):
    n, h, w, cout, dtype, act = ss.SHAPES[0]
    img, wt, gamma, beta, dout = ss.make_inputs(n, 18, 22, cout, dtype, pdt, seed=9)
    y, scale, shift, mean, invstd = ss.cpu_forward(img, wt, gamma, beta, dtype)
    args = (img, dout, y, scale, shift, mean, invstd, gamma, act)
    dw, dgamma, dbeta = emulate(*args, w_dtype=w_dtype)
    assert dw.dtype == w_dtype and dgamma.dtype == pdt and dbeta.dtype == pdt
    ss.check(dw, dgamma, dbeta, ss.reference(*args), f"w {w_dtype} p {pdt}")


@pytest.mark.parametrize("i", range(len(ss.SHAPES)), ids=ss.IDS)
@pytest.mark.parametrize("mut", MUTANTS)
def test_mutant_is_outside_the_limit(mut, i):
    n, h, w, cout, dtype, act = ss.SHAPES[i]
    # the unrounded image hides under SiLU behind the term granted for dz's rounding (module docstring): identity variant
    args, ref = case(i, 0 if mut == "unrounded_image" else None)
    dw, dgamma, dbeta = emulate(*args, mut=mut)
    sh = share(dw, ref)
    print(f"\n{mut} on {ss.IDS[i]}: {sh:.2f} limits")
    if mut == "padded_pixels" and h % 2 == 1 and w % 2 == 1:
        oh, ow = ss.out_hw(h, w)                            # no pixel past the end has a tap inside the image
        xp = tile_pixels(args[0], oh, ow)
        assert float(xp[:, :, oh:].abs().sum()) == 0.0 and float(xp[:, :, :, ow:].abs().sum()) == 0.0
        return
    with pytest.raises(sc.StrictMismatch):
        ss.check(dw, dgamma, dbeta, ref, f"{mut} {ss.IDS[i]}")
    assert sh > 1.0                                         # ... and it is dW that is outside, not dgamma / dbeta


@pytest.mark.parametrize("i", [0, 1, 3], ids=[ss.IDS[0], ss.IDS[1], ss.IDS[3]])
def test_unrounded_image_under_silu_is_inside_the_term_granted_for_dz(i):
    """recorded, not hidden: the limit cannot tell the unrounded image from the rounding of dz it allows (module docstring)"""
    args, ref = case(i)
    r, m, e = ref["dw"]
    dw = emulate(*args, mut="unrounded_image")[0]
    err = (dw.double() - r).abs()
    n, c, oh, ow = args[2].shape
    x, xh = ss.unfold(args[0].double()), ss.unfold(args[0].to(args[2].dtype).double())
    dz = sb.bwd_dz(*args[1:5], args[8])[0].reshape(n, c, -1)
    a = (sb.d64(args[7]) * sb.d64(args[6]))[:, None].abs()                 # |A| = |gamma invstd|
    granted = ss.UNIT[args[2].dtype] * a * torch.einsum("ncp,nkp->ck", dz.abs(), xh.abs())
    moved = a * torch.einsum("ncp,nkp->ck", dz.abs(), (x - xh).abs())
    assert bool((moved <= granted * (1 + 1e-9)).all())
    print(f"\nunrounded image on {ss.IDS[i]} (SiLU): {share(dw, ref):.3f} of the limit, max error {float(err.max()):.3g}")
