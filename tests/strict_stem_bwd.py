"""Float64 reference and derived per-element limit for the stem's one-pass backward (ops.stem_bn_wgrad, csrc/stem.hip),
shared by tests/test_stem_bwd_bound_cpu.py (the proof of the limit, no GPU) and tests/test_gpu_stem_bwd_fused.py.

Reference, all in float64 on the CPU: dz, the two channel sums and the coefficients A, B, D come from tests/strict_bn.py
(bwd_dz, sums_bwd, coef_bwd) out of the published fp32 scale / shift / mean / invstd; with Xh the image rounded to the
compute type T and unfolded (k = ci*9 + kh*3 + kw, padding taps 0, existing output pixels only)

    dW_ref[co][k] = sum_p Xh[p][k] (A_co dz[p][co] + B_co y[p][co] + D_co) = A G1 + B G2 + D G3

Limit of element (co, k), no fitted constant:
    1/2 ulp of dW's own type                                    what the comparator grants every element
  + u_T |A| sum_p |dz| |Xh|                                     the ONE rounding of dz to T (u_T = 2^-8 bf16, 2^-11 f16); the
                                                                three-launch path rounds A dz + B y + D there instead.
                                                                dz_exact (one-pass kernel under identity: dz = dout * 1.0f
                                                                is a value of T, nothing rounds): 0, the tighter limit
  + c 2^-24 (|A| sum |dz| |Xh| + |B| sum |y| |Xh| + |D| sum |Xh|)    strict_compare's fp32-accumulation rule, c = 16, on the
                                                                absolute masses of the three terms (fp32 MFMA sums per workgroup,
                                                                the VALU sum of G3; combined and multiplied in double)
  + dB |G2| + dD |G3|                                           coef_bwd's input errors: the limits of the two channel sums
dgamma, dbeta: the limits strict_bn derives for them (coef_bwd with the sums' limits as input errors).

The first term is worst-case linear in the pixel count while a rounding error grows like its square root: under SiLU the
limit is wide against random perturbations of relative size u_T.  What it can and cannot see is measured by
tests/test_stem_bwd_bound_cpu.py."""
import torch
import torch.nn.functional as F

import strict_bn as sb
import strict_compare as sc

UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# N, H, W, Cout, dtype, act: the smallest shapes at which each part of the kernel can go wrong
SHAPES = [(2, 38, 262, 32, torch.bfloat16, 1),     # OW = 131: a second segment with 3 live pixels; OH = 19: half-empty last row pair
          (2, 37, 261, 16, torch.float16, 1),      # W % 4 != 0: the scalar staging path; odd H
          (1, 8, 8, 48, torch.bfloat16, 0),        # one tile, almost all padding: the validity mask of G3
          (8, 520, 64, 32, torch.bfloat16, 1)]     # 1040 tiles: more than the grid holds, the grid-stride loop
IDS = ["2x38x262c32-bf16-silu", "2x37x261c16-f16-silu", "1x8x8c48-bf16-id", "8x520x64c32-bf16-silu"]


def out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def make_inputs(n, h, w, cout, dtype, pdt=torch.float32, seed=0):
    """-> img (fp32 NCHW, mean 0.5: D G3 and B G2 matter), conv weight, gamma, beta (pdt), dout (dtype): seeded noise"""
    g = torch.Generator().manual_seed(7100 + seed)
    oh, ow = out_hw(h, w)
    img = torch.randn(n, 3, h, w, generator=g) + 0.5
    wt = torch.randn(cout, 3, 3, 3, generator=g) * 0.2
    gamma = (1 + 0.1 * torch.randn(cout, generator=g)).to(pdt)
    beta = (0.1 * torch.randn(cout, generator=g)).to(pdt)
    dout = torch.randn(n, cout, oh, ow, generator=g).to(dtype)
    return img, wt, gamma, beta, dout


def cpu_forward(img, wt, gamma, beta, dtype, eps=1e-3):
    """stand-in for stem_conv_fwd + bn_act_fwd_train where there is no GPU: -> y (dtype), scale, shift, mean, invstd (fp32)"""
    y = F.conv2d(img.to(dtype).float(), wt.to(dtype).float(), None, 2, 1).to(dtype)
    yd = y.double()
    m = yd.mean((0, 2, 3))
    var = (yd * yd).mean((0, 2, 3)) - m * m
    invstd = ((var.clamp_min(0.0) + sb.f32_of(eps)) ** -0.5).float()
    mean = m.float()
    scale = gamma.float() * invstd
    shift = beta.float() - mean * scale
    return y, scale, shift, mean, invstd


def unfold(x):
    """(N, 3, H, W) -> (N, 27, OH*OW), k = ci*9 + kh*3 + kw"""
    return F.unfold(x, 3, padding=1, stride=2)


def reference(img, dout, y, scale, shift, mean, invstd, gamma, act, dz_exact=False):
    """-> {"dw": (ref, mass, extra) as (Cout, 3, 3, 3) float64, "dgamma" / "dbeta": (ref, noise) of strict_bn}.
    dz_exact: the tighter limit without the rounding term -- for the one-pass kernel under identity only (dz = dout is a
    value of T); the three-launch path rounds A dz + B y + D to T whatever the activation and keeps the term"""
    assert not (dz_exact and act)
    T, pdt = y.dtype, gamma.dtype
    n, c, oh, ow = y.shape
    dz, ddz, dga = sb.bwd_dz(dout, y, scale, shift, act)
    sums = sb.sums_bwd(dz, ddz, dga, y)
    k = sb.coef_bwd(sums["s"][0], sums["q"][0], n * oh * ow, gamma, mean, invstd, pdt, sums["s"][1], sums["q"][1])
    x = unfold(img.detach().cpu().to(T).double())
    yd, dzf = sb.d64(y).reshape(n, c, -1), dz.reshape(n, c, -1)
    g1, m1 = torch.einsum("ncp,nkp->ck", dzf, x), torch.einsum("ncp,nkp->ck", dzf.abs(), x.abs())
    g2, m2 = torch.einsum("ncp,nkp->ck", yd, x), torch.einsum("ncp,nkp->ck", yd.abs(), x.abs())
    g3, m3 = x.sum((0, 2))[None], x.abs().sum((0, 2))[None]
    a, b, d = (k[nm][:, None] for nm in ("A", "B", "D"))
    ref = a * g1 + b * g2 + d * g3
    mass = a.abs() * m1 + b.abs() * m2 + d.abs() * m3
    unit = 0.0 if dz_exact else UNIT[T]
    extra = unit * a.abs() * m1 + k["dB"][:, None] * g2.abs() + k["dD"][:, None] * g3.abs()
    return {"dw": tuple(t.reshape(c, 3, 3, 3) for t in (ref, mass, extra)), "dgamma": k["dgamma"], "dbeta": k["dbeta"]}


def check(dw, dgamma, dbeta, ref, what):
    """every element of dW, dgamma and dbeta; the dtypes are the callers' (dW: the weight's, the other two: gamma's)"""
    r, m, e = ref["dw"]
    sb.assert_within(dbeta, ref["dbeta"], dbeta.dtype, f"{what} dbeta", "bn_dbeta")
    sb.assert_within(dgamma, ref["dgamma"], dgamma.dtype, f"{what} dgamma", "bn_dgamma")
    return sc.assert_close(dw, r, m, dw.dtype, f"{what} dW", "stem_wgrad", e_act=e)
