"""Float64 references and per-element bounds for the AdamW step and its loss-scaling / clipping kernels (csrc/optim.hip:
k_adamw, k_grad_sqnorm, k_clip_finalize, k_found_inf, k_amp_update), shared by tests/test_strict_optim_cpu.py (the proof of
the comparator, no GPU) and tests/test_gpu_adamw.py (-m gpu).

The model.  One step is compared against the float64 rule stepped from the device's OWN fp32 state read back before the
step, so no error is carried from step to step.  U = 2^-24 (one fp32 rounding, relative).  The kernel forms, from eight fp32
coefficients rounded from doubles (b1, 1-b1, b2, 1-b2, lr/bc1, sqrt(bc2), 1-lr*wd, eps; bc_i = 1 - b_i^t in double):

    gg  = fl(g * gs)                       gs = fl(fl(1/scale) * coef), 1 without loss scaling and clipping
    m'  = fma(b1, m, fl((1-b1) * gg))
    v'  = fma(b2, v, fl(fl((1-b2) * gg) * gg))
    den = fl(fl(hwsqrt(v') / sqrt(bc2)) + eps)
    p'  = store(fma(p, decay, -fl(fl((lr/bc1) * m') / den)))

(the last fma is how `fl(p*decay) - ...` is compiled under the default contraction; hwsqrt is the hardware root, within
1 ulp).  Against the float64 values of the same rule, first order in U, every term non-negative:

    E_gg  = 3U|gg| when gs != 1 (the fp32 1/scale, its product with the clip coefficient, the product with g), else 0.
            The tests hand `gs` over as the fp32 value the kernel forms; the first two of the three then cost nothing.
    E_m   = U(|m'| + |b1 m| + 2|(1-b1) gg|) + (1-b1) E_gg + T        result; b1; 1-b1 and the inner product; the input
    E_v   = U(|v'| + |b2 v| + 3 (1-b2) gg^2) + 2 (1-b2) |gg| E_gg + T   result; b2; 1-b2 and two inner products; the input
    s = sqrt(v'), q = s / sqrt(bc2), den = q + eps
    E_s   = min(E_v / 2s, sqrt(E_v)) + 2U s          |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= sqrt|a - b|; every
            term of v' is non-negative, so E_v <= 11 U v' and the first form is the sharp one wherever v' > 0; the min keeps
            the bound finite (0) at v' = 0.  2U s is the 1-ulp root: the ISA manual's figure, not measured here.
    E_den = E_s / sqrt(bc2) + 2U q + U den + U eps   sqrt(bc2) and the division; the sum; eps
    w = (lr/bc1) m' / den
    E_w   = |w| (3U + E_den / den) + (lr/bc1) / den * E_m            lr/bc1, the product, the division; den; m'
    E_p   = 1/2 ulp_store(|p'| + rest) + rest,  rest = U|p'| + 2U|p decay| + E_w
            the fp32 result, then the store (strict_compare.ulp: bf16 8 significant bits, f16 11 with its subnormal
            spacing, fp32 24; taken at the upper end of where the fp32 result can lie, so that the bound does not depend on
            the kernel's output).  2U|p decay| = the rounding of `decay` + one more for a compiler that does NOT fuse the
            last operation: the bound holds for either code.
    T = 2^-149: a result below the smallest normal fp32 is rounded absolutely, not relatively (added for completeness; no
            input of the tests comes near it).

The GPU tests allow HEADROOM = 2 x these bounds (tests/test_gpu_sgd.py's convention: the usual headroom over a counted
number of roundings, it also absorbs the second-order terms); the CPU stand-ins must stay inside 1 x.

Mutants (`mutant=`), each the float64 rule with ONE thing changed; a comparator that cannot tell them from the kernel is
too weak:  eps_before (s + eps) / sqrt(bc2);  eps_inside sqrt(v'/bc2 + eps);  bc2_unrooted s / bc2 + eps;  l2 weight decay
added to the gradient, no decay factor;  wd_after (p - w) * decay;  step_off bias corrections of step t - 1 (from step 2 on).

Other references: clip_finalize_ref (float64 min(1, max / (norm + 1e-6)); an infinite norm gives 0, nan gives nan),
sqnorm_ref (float64 sum of squares of one 4096-element chunk, bound 14 U sum g^2: the count of k_grad_sqnorm's comment),
amp_update_ref (torch._amp_update_scale_ on CPU tensors, including its refusal to grow into inf).

The inputs (grad_values): 0.004 N(0,1) scaled per step by (1, 30, 0.01, 5); in every tensor's first eighth an "eps block",
|g| log-uniform in [1e-10, 1e-6] with random sign on EVERY step, so that sqrt(v) stays next to eps = 1e-8 there; in its
second eighth exact zeros on even steps (0, 2, ...: v' = m' = 0 on the first step, zero gradients on live moments later).

Recorded maxima (2026-10-20, this file's first commit, on top of 7394f32; the tests print them again on every run).
Largest err / E, E WITHOUT the headroom, per quantity and stored type; per mutant the fraction of its block outside 2 E_p at
its best step.
  CPU stand-ins (tests/test_strict_optim_cpu.py; 37 789 stepped elements, 6 steps, gs alternating 1 and fl(0.37 fl(1/1536))):
    E_m 0.718    E_v 0.819    E_p fp32 store 0.302 with the last operation fused, 0.539 unfused    bf16 store 1.000    f16 0.999
    mutants: eps_before, eps_inside, bc2_unrooted, l2, step_off 1.0000; wd_after 0.9902
  MI355X (tests/test_gpu_adamw.py; all of its tests, the maximum over them):
    E_m 0.721    E_v 0.859    E_p fp32 store 0.325    bf16 store 0.9997    f16 store 0.9996
      per test (E_m, E_v, E_p fp32): parity 0.718 0.859 0.325; GradScaler protocol at 1024 0.718 0.607 0.300; DeviceGradScaler at
      1536 0.716 0.605 0.300; clipped 0.718 0.741 0.301; 300-record table 0.721 0.608 0.304; after skipped steps 0.714 0.605 0.309
    mutants: eps_before 0.9991, eps_inside 0.9996, bc2_unrooted 0.9997, l2 1.0000, wd_after 0.9934, step_off 0.9996
    k_grad_sqnorm's partials: at most 0.056 of 14 U sum g^2 (packet, bf16, f16, odd length, unaligned view)
  No share exceeds 1: the headroom of 2 is unused on the device.  The fp32 store's 0.325 sits where the fused stand-in's 0.302
  does and well below the unfused one's 0.539, as the assembly says it should (one rounding for decay and subtraction).  A
  16-bit store's share is the half ulp of the store itself; the shares just under 1 are parameters whose fp32 result fell
  next to the middle between two neighbours of the stored type.
"""
import math

import torch

from strict_compare import ulp

U = 2.0 ** -24
TINY = 2.0 ** -149
HEADROOM = 2.0
CHUNK = 4096
SQNORM_ROUNDINGS = 14
MUTANTS = ("eps_before", "eps_inside", "bc2_unrooted", "l2", "wd_after", "step_off")
EPS_BLOCK_MUTANTS = ("eps_before", "eps_inside")        # shown by the eps block; the others by every element
STD = 0.004
SCALES = (1.0, 30.0, 0.01, 5.0)
HYPER = (1e-2, 0.9, 0.999, 1e-8, 0.1)                   # lr, beta1, beta2, eps, weight decay of the parity tests
# Every layout in one optimizer: a multiple of 4 over several chunks, sizes 1 and 3, an empty parameter (one idle chunk in the
# job table), a chunk edge (4096, 4097), a gradient that is a view one element into its storage (4-byte aligned only), an fp32
# parameter with a bf16 / an f16 `lowp_grad`, a parameter without gradient, a bf16 and an f16 parameter with fp32 gradients
SHAPES = [(64, 32, 3, 3), (1,), (3,), (0,), (4096,), (4097,), (5000,), (4099,), (515,), (516,), (33,), (515,), (515,)]
KINDS = ["f32", "f32", "f32", "empty", "f32", "f32", "f32", "view", "g_bf16", "g_f16", "nograd", "p_bf16", "p_f16"]
P_DTYPE = {"p_bf16": torch.bfloat16, "p_f16": torch.float16}
G_DTYPE = {"g_bf16": torch.bfloat16, "g_f16": torch.float16}


def f32(x):
    """The fp32 value nearest to the Python double x, as a Python double (how the kernel rounds a coefficient)."""
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


def eps_block(n):
    return slice(0, n // 8)


def zero_run(n):
    return slice(n // 8, n // 4)


def grad_values(shapes, seed, step):
    """The gradient values of step `step` (0, 1, ...) for every shape, fp32 on the host: see "The inputs" above."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in shapes:
        n = math.prod(s)
        v = (torch.randn(n, generator=g) * (STD * SCALES[step % 4]))
        k = n // 8
        mag = 10.0 ** (-10.0 + 4.0 * torch.rand(k, generator=g, dtype=torch.float64))
        sign = torch.randint(0, 2, (k,), generator=g).double() * 2.0 - 1.0
        v[eps_block(n)] = (mag * sign).float()
        if step % 2 == 0:
            v[zero_run(n)] = 0.0
        out.append(v.reshape(s))
    return out


def adamw_ref(p, g, m, v, gs, hyper, t, store_dtype, mutant=None):
    """One AdamW step in float64.  p, g, m, v: float64 tensors holding the device's values (a 16-bit parameter or gradient
    widened exactly); gs: the factor on the gradient (a Python float; the fp32 value the kernel forms); hyper = (lr, beta1,
    beta2, eps, weight_decay) as Python doubles; t = 1, 2, ...: the step being taken; store_dtype: the parameter's type.
    -> p', m', v', E_p, E_m, E_v (no headroom).  With `mutant` the bounds are still those of the true rule."""
    assert mutant is None or mutant in MUTANTS, mutant
    lr, b1, b2, eps, wd = hyper
    tb = t - 1 if mutant == "step_off" and t >= 2 else t
    bc1, bc2 = 1.0 - b1 ** tb, 1.0 - b2 ** tb
    rbc2 = math.sqrt(bc2)
    decay = 1.0 - lr * wd
    gg = g * gs
    e_gg = 3.0 * U * gg.abs() if gs != 1.0 else torch.zeros_like(gg)
    gm = gg + wd * p if mutant == "l2" else gg
    m1 = b1 * m + (1.0 - b1) * gm
    v1 = b2 * v + (1.0 - b2) * gm * gm
    s = v1.sqrt()
    q = s / rbc2
    den = q + eps
    if mutant == "eps_before":
        den_used = (s + eps) / rbc2
    elif mutant == "eps_inside":
        den_used = (v1 / bc2 + eps).sqrt()
    elif mutant == "bc2_unrooted":
        den_used = s / bc2 + eps
    else:
        den_used = den
    w = (lr / bc1) * m1 / den_used
    if mutant == "l2":
        p1 = p - w
    elif mutant == "wd_after":
        p1 = (p - w) * decay
    else:
        p1 = p * decay - w
    # the bounds, of the true rule at these values
    e_m = U * (m1.abs() + (b1 * m).abs() + 2.0 * ((1.0 - b1) * gg).abs()) + (1.0 - b1) * e_gg + TINY
    e_v = U * (v1.abs() + (b2 * v).abs() + 3.0 * (1.0 - b2) * gg * gg) + 2.0 * (1.0 - b2) * gg.abs() * e_gg + TINY
    e_s = torch.minimum(e_v / (2.0 * s).clamp_min(1e-300), e_v.sqrt()) + 2.0 * U * s
    e_den = e_s / rbc2 + 2.0 * U * q + U * den + U * eps
    wt = (lr / bc1) * m1 / den
    e_w = wt.abs() * (3.0 * U + e_den / den) + (lr / bc1) / den * e_m
    rest = U * p1.abs() + 2.0 * U * (p * decay).abs() + e_w
    e_p = 0.5 * ulp(p1.abs() + rest, store_dtype) + rest
    return p1, m1, v1, e_p, e_m, e_v


def _fma(a, b, c):
    """fp32 fused multiply-add emulated through float64: the product of two fp32 values is exact there, the sum is rounded
    to 53 bits and then to 24 (the double rounding moves a result by far less than the bounds' second-order terms)."""
    return (a.double() * b.double() + c.double()).float()


def adamw_standin(p, g, m, v, scale, coef, hyper, t, fused=True):
    """The kernel's sequence in plain torch CPU fp32 operations, one rounding per line of the model above.  p: the parameter
    as stored (fp32, bf16 or f16), g: the gradient as stored, m, v: fp32; scale / coef: fp32 tensors of one element or None.
    fused: the last operation as one fma (what the compiler emits) or as a rounded product and a subtraction.
    -> p' (p's dtype), m', v' (fp32), and gs as the Python float the kernel forms."""
    lr, b1, b2, eps, wd = hyper
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    c = lambda x: torch.tensor(x, dtype=torch.float64).to(torch.float32)
    b1f, omb1, b2f, omb2 = c(b1), c(1.0 - b1), c(b2), c(1.0 - b2)
    step_size, bc2s, decay, epsf = c(lr / bc1), c(math.sqrt(bc2)), c(1.0 - lr * wd), c(eps)
    gs = torch.tensor(1.0) if scale is None else torch.tensor(1.0) / scale
    if coef is not None:
        gs = gs * coef
    pf = p.float()
    gg = g.float() * gs
    m1 = _fma(b1f, m, omb1 * gg)
    v1 = _fma(b2f, v, (omb2 * gg) * gg)
    den = v1.sqrt() / bc2s + epsf
    w = (step_size * m1) / den
    p1 = _fma(pf, decay, -w) if fused else pf * decay - w
    return p1.to(p.dtype), m1, v1, float(gs)


def clip_finalize_ref(partials, max_norm, scale=None):
    """k_clip_finalize in float64: partials (any float tensor, may be empty), max_norm and scale as Python floats (the fp32
    values the device holds) -> (total_norm, coef) as Python floats."""
    total = float(partials.double().sum()) if partials.numel() else 0.0
    norm = math.sqrt(total) if total == total and total >= 0.0 else float("nan")
    if scale is not None:
        norm = norm / scale
    c = max_norm / (norm + 1e-6)
    return norm, (c if c < 1.0 else (c if c != c else 1.0))


def sqnorm_ref(g_chunk):
    """Float64 sum of squares of one chunk (<= 4096 elements, any float type) and its bound, 14 U sum g^2."""
    assert g_chunk.numel() <= CHUNK
    s = float((g_chunk.double() ** 2).sum())
    return s, SQNORM_ROUNDINGS * U * s


def amp_update_ref(scale, tracker, found, growth, backoff, interval):
    """torch._amp_update_scale_ on CPU tensors -> (scale, tracker) after the update."""
    s = torch.tensor([scale], dtype=torch.float32)
    k = torch.tensor([tracker], dtype=torch.int32)
    torch._amp_update_scale_(s, k, torch.tensor([float(found)], dtype=torch.float32), float(growth), float(backoff), int(interval))
    return float(s), int(k)


class Worst:
    """Largest err / E per key, printed by the tests."""

    def __init__(self):
        self.w = {}

    def add(self, key, err, e):
        r = float((err / e.clamp_min(1e-300)).max()) if err.numel() else 0.0
        self.w[key] = max(self.w.get(key, 0.0), r)
        return r

    def __str__(self):
        return "  ".join(f"{k} {v:.4f}" for k, v in sorted(self.w.items()))
