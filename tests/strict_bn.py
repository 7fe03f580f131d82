"""Strict per-element comparator for the BatchNorm kernels of csrc/elementwise.hip: float64 references and derived limits,
on top of strict_compare.py (its ulp(), assert_close, StrictMismatch, OBSERVED / report() and failure histograms).  Shared
by tests/test_strict_bn_cpu.py (the proof of the comparator, no GPU) and tests/test_gpu_bn.py (the kernels).

Every stage is compared with the float64 evaluation of its formula from exactly the buffers that stage receives (the
kernel's own accumulator, its published scale / shift / mean / invstd), so that an error of one stage cannot hide in the
slack of another.  Where a buffer is not exposed (the partial rows of bn_train_stats, bn_act_bwd, channel_sum) the limits
compose: every coefficient limit takes the error of the sums it starts from as an argument (ds, dq); zero gives the
stage-wise test.  Notation: U = 2^-24; u_T(x) = 1/2 ulp_T(x) (what the comparator itself grants every element, in the
type the element is stored in); N = pixel count; c = 16 (sc.C per family, the rule of strict_compare.py applies);
E_exp(z) = (|z| + 4) 2^-22, the __expf model of strict_compare's E_act (multiply by log2 e, exp2 and reciprocal of about
an ulp each, doubled).

Sums (bn_sum, bn_sumsq; bn_bwd_sum, bn_bwd_sumsq).  fp32 partial sums per thread, an fp32 add per workgroup row, then
either float atomics into 8 replicas or one partial row per workgroup; the fold is in double.
    sum y      |got - S| <= c U sum|y|             any fp32 summation order of K terms obeys (K - 1) U mass
    sum y^2    c U sum y^2, + U sum y^2 for fp32 inputs: the square rounds (a 16-bit square is exact in fp32)
Forward coefficients (bn_coef), bn_fwd_coef from the sums S~, Q~ the kernel read, all in double:
    m = S~ / N, var = max(Q~ / N - m^2, 0), invstd = (var + eps)^-1/2, scale = gamma invstd, shift = beta - m scale
    mean     u_32 only: (float) m                       invstd   u_32 only: (float) of the double expression
    scale    U |scale| + u_32: invstd's rounding, then the fp32 product
    shift    U (3 |m scale| + |beta|) + u_32: (float) m, scale's two roundings above on the product's mass, the product
             m scale itself counted with the subtraction in |beta| + u_32
    running  r' = (1 - mom) r + mom x, x = mean or the unbiased variance var N / (N - 1) (N = 1: var as it is), mom as the
             fp32 value the kernel receives: 3 U ((1 - mom) |r| + mom |x|) -- the rounding of 1 - mom and of the first
             product on the first term, x's own rounding and the second product on the second, the add -- then u_bdt
    with a sum error (ds, dq):  dm = ds / N, dvar = dq / N + 2 |m| ds / N, d invstd = invstd dvar / (2 (var + eps))
             (first order: dvar is at most 1e-2 of eps on every class here), d scale = |gamma| d invstd,
             d shift = |scale| dm + |m| d scale, d running = mom dm, mom dvar N / (N - 1)
    bn_eval_coeffs: scale = gamma / sqrtf(rvar + eps): 2 U |scale| + u_32 (the add counts half, sqrtf one, rounded up;
             the IEEE division is the u_32); shift: U (4 |rmean scale| + |beta|) + u_32 (one more rounding than above)
Forward apply (bn_fwd): z = y scale + shift from the PUBLISHED fp32 scale and shift, out = act(z) (+ res)
    u_T + 2 U (|y scale| + |shift|) (x 1.1 under SiLU, max |silu'|)      product and add, or one fma
        + E_exp(z) |silu(z)| + U |silu(z)|                               __expf; the hardware reciprocal of sigmoid_rcp
        + U (|act(z)| + |res|) with a residual                           the fp32 add
Backward reduction: dz = dout act'(z), act'(z) = s (1 + z (1 - s)), s = sigmoid(z), cancels near z = -1.28; bounded on its
    mass Ga = s (1 + |z| (1 - s)):
    |d act'| <= Ga (2 E_exp(z) + 4 U) + 1/2 dz_in      s enters twice; four fp32 operations; |act''| <= 1/2 on the error
                                                      dz_in = 2 U (|y scale| + |shift|) of z
    |d dz|   <= |dout| |d act'| + U |dz|              identity: dz = dout * 1.0f is exact, d dz = 0
    sum dz     c U sum |dout| Ga + sum |d dz|         sum dz y    (c + 1) U sum |dout| Ga |y| + sum |d dz| |y|
Backward coefficients and apply (bn_dbeta, bn_dgamma, bn_dy), bn_bwd_coef from the accumulator the kernel read and the
    mean, invstd, gamma it was given, in double:  dbeta = S, dgamma = invstd (Q - mean S), k0 = gamma invstd, c1 = S / N,
    c2 = dgamma / N, A = k0, B = -k0 c2 invstd, D = -k0 c1 + k0 c2 mean invstd
    dbeta, dgamma   u_pdt; a 16-bit parameter dtype rounds the fp32 value again: + U |value|
    dy = A dz + B y + D    u_T + |A| |d dz| + 4 U (|A dz| + |B y| + |D|): (float) of each constant, the product, two adds
                    on at most the whole mass.  |B y| + |D| grows with |mean| / std: the cancellation of the three-constant
                    form, stated as it is.  Eval-mode backward: A = scale, B = D = 0
    with (ds, dq):  d dgamma = invstd (dq + |mean| ds), dB = |k0 invstd| d dgamma / N,
                    dD = |k0| ds / N + |k0 mean invstd| d dgamma / N, dy gets dB |y| + dD more

What strict_compare.assert_close receives: c = 1 and mass = noise / U, so its limit IS u_T + noise and the figure it
records per family is the largest share of the noise budget used, (|got - ref| - u_T) / noise, limit 1.  A per-channel
vector goes in as (1, C, 1): its histogram by 16-channel block names the channel group.

Input classes (make_y): plain (mean 0.3, std 1.5); offset (mean 6, std 0.25: var = Q / N - m^2 and
dgamma = invstd (sum dz y - mean sum dz) both cancel, |mean| / std = 24); tiny (mean 0.02, std 0.01: variance below
eps = 1e-3); const (plain, every third channel one 16-bit value: true variance 0, the clamp applies, invstd = eps^-1/2).

Recorded maxima, largest share of the noise budget used per family (limit 1; c = 16 held for every family).
MI355X, tests/test_gpu_bn.py, 2026-10-18, on the kernels of commit db5b4ad (231 cases, 128 M elements of out and of dy):
    bn_sum 0.20   bn_sumsq 0.23 (3.6 x 2^-24 of the mass)   bn_bwd_sum 0.08   bn_bwd_sumsq 0.13   bn_coef 0.94
    bn_fwd 0.42   bn_dbeta 0.11   bn_dgamma 0.12   bn_dy 0.62
    `offset` against float64 from the INPUTS (not from the accumulator), 429 and 22 000 pixels, worst channel:
      invstd, relative error   fp32 1.4e-4 (accumulator path) / 1.0e-4 (deterministic)   bf16 3.4e-5 / 5.8e-8   f16 4.7e-5 / 7.5e-5
      dgamma, of max |dgamma|  fp32 1.1e-4 / 7.1e-5   bf16 2.8e-5 / 7.8e-6   f16 3.2e-5 / 6.4e-5
                               (at most 11.6 x 2^-24 of its mass invstd sum |dz y|)
    against a composed allowance of about 1e-3 on invstd there: E[y^2] - m^2 at |mean| / std = 24 uses about a sixth of it.
CPU stand-ins: tests/test_strict_bn_cpu.py, STAND_IN_MAXIMA."""
import torch

import strict_compare as sc
from strict_compare import U24, StrictMismatch, image_pattern, ulp  # noqa: F401  (re-exported for the tests)

F32 = torch.float32
FAMILIES = ("bn_sum", "bn_sumsq", "bn_bwd_sum", "bn_bwd_sumsq", "bn_coef", "bn_fwd", "bn_dgamma", "bn_dbeta", "bn_dy")
for _f in FAMILIES:
    sc.C[_f] = sc.C_DEFAULT
    sc.BUDGET_FAMILIES.add(_f)
CLASSES = ("plain", "offset", "tiny", "const")
MEAN_STD = {"plain": (0.3, 1.5), "offset": (6.0, 0.25), "tiny": (0.02, 0.01), "const": (0.3, 1.5)}
CONST_VALUE = 179.0 / 128.0          # 8 significant bits: exact in bf16, f16 and fp32; its square needs 16
# the limits check() applied to the BatchNorm leaves before (share of the tensor's largest magnitude): only for the guard
# 'nowhere wider than before'
OLD_TOL = {torch.float32: 1e-4, torch.bfloat16: 2.0 ** -6, torch.float16: 2.0 ** -9}


# At a handful of pixels out and dy are differences of nearly equal terms (one pixel: y = mean, out = beta and dy = 0 up to
# rounding), and a share of the tensor's largest magnitude is no limit at all: the guard is asserted at the pixel counts the
# former tests had (429 and 22 000).
GUARD_MIN_COUNT = 100
GUARD = True      # the guard is for sound outputs (1/2 ulp of a wild `got` is wide): the mutant tests switch it off


def old_abs(ref, dtype, mult=1.0):
    return OLD_TOL[dtype] * mult * max(float(ref.abs().max()), 1e-6)


def make_y(cls, n, c, h, w, dtype, seed=0):
    """(n, c, h, w) in `dtype` on the CPU: min(n, 3) base images laid out by image_pattern(), so neighbours differ"""
    assert cls in CLASSES
    g = torch.Generator().manual_seed(300 + seed)
    mean, std = MEAN_STD[cls]
    base = torch.randn(min(n, 3), c, h, w, generator=g) * std + mean
    if cls == "const":
        base[:, ::3] = CONST_VALUE
    return base[image_pattern(n, seed)].to(dtype)


def d64(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def _bc(v):
    return v.view(1, -1, 1, 1)


def f32_of(x):
    """the fp32 value a kernel receives for a Python float (eps, momentum)"""
    return float(torch.tensor(x, dtype=torch.float32))


def fold(acc, c):
    """accumulator fp32 [8][2][C] -> (S~, Q~) in double, as acc_fold does"""
    a = d64(acc).view(-1, 2, c).sum(0)
    return a[0], a[1]


# ---------------------------------------------------------------------------------------------- references and limits
def sums_fwd(y, dtype):
    """-> {"s": (sum y, noise), "q": (sum y^2, noise)} per channel"""
    y = d64(y)
    q = (y * y).sum((0, 2, 3))
    cq = sc.C["bn_sumsq"] + (1.0 if dtype == F32 else 0.0)
    return {"s": (y.sum((0, 2, 3)), sc.C["bn_sum"] * U24 * y.abs().sum((0, 2, 3))), "q": (q, cq * U24 * q)}


def coef_fwd(s, q, n, eps, gamma, beta, rmean=None, rvar=None, momentum=0.0, ds=0.0, dq=0.0):
    """-> {name: (ref, noise)} for mean, invstd, scale, shift (+ rmean, rvar: the updated running statistics)"""
    eps, mom = f32_of(eps), f32_of(momentum)
    gamma, beta = d64(gamma), d64(beta)
    m = s / n
    var = (q / n - m * m).clamp_min(0.0)
    dm = ds / n
    dvar = dq / n + 2.0 * m.abs() * dm
    inv = (var + eps) ** -0.5
    dinv = inv * dvar / (2.0 * (var + eps))
    scale = gamma * inv
    dscale = gamma.abs() * dinv
    out = {"mean": (m, dm + 0.0 * m), "invstd": (inv, dinv + 0.0 * m), "scale": (scale, U24 * scale.abs() + dscale),
           "shift": (beta - m * scale, U24 * (3.0 * (m * scale).abs() + beta.abs()) + scale.abs() * dm + m.abs() * dscale)}
    if rmean is not None:
        k = n / (n - 1.0) if n > 1 else 1.0
        rm, rv = d64(rmean), d64(rvar)
        out["rmean"] = ((1.0 - mom) * rm + mom * m, 3.0 * U24 * ((1.0 - mom) * rm.abs() + mom * m.abs()) + mom * dm)
        out["rvar"] = ((1.0 - mom) * rv + mom * var * k, 3.0 * U24 * ((1.0 - mom) * rv.abs() + mom * var * k) + mom * dvar * k)
    return out


def coef_eval(gamma, beta, rmean, rvar, eps):
    gamma, beta, rm, rv = d64(gamma), d64(beta), d64(rmean), d64(rvar)
    scale = gamma / torch.sqrt(rv + f32_of(eps))
    return {"scale": (scale, 2.0 * U24 * scale.abs()),
            "shift": (beta - rm * scale, U24 * (4.0 * (rm * scale).abs() + beta.abs()))}


def _z(y, scale, shift):
    ys = d64(y) * _bc(d64(scale))
    sh = _bc(d64(shift))
    return ys + sh, ys.abs() + sh.abs()


def fwd_apply(y, scale, shift, act, res=None):
    """-> (out, noise) from the published fp32 scale and shift"""
    z, zm = _z(y, scale, shift)
    if act:
        o = z * torch.sigmoid(z)
        noise = 2.2 * U24 * zm + (z.abs() + 4.0) * 2.0 ** -22 * o.abs() + U24 * o.abs()
    else:
        o, noise = z, 2.0 * U24 * zm
    if res is not None:
        r = d64(res)
        noise = noise + U24 * (o.abs() + r.abs())
        o = o + r
    return o, noise


def bwd_dz(dout, y, scale, shift, act):
    """-> (dz, |d dz|, |dout| Ga)"""
    d = d64(dout)
    if not act:
        return d, torch.zeros_like(d), d.abs()
    z, zm = _z(y, scale, shift)
    s = torch.sigmoid(z)
    ga = s * (1.0 + z.abs() * (1.0 - s))
    dact = ga * (2.0 * (z.abs() + 4.0) * 2.0 ** -22 + 4.0 * U24) + 0.5 * 2.0 * U24 * zm
    dz = d * s * (1.0 + z * (1.0 - s))
    return dz, d.abs() * dact + U24 * dz.abs(), d.abs() * ga


def sums_bwd(dz, ddz, dga, y):
    y = d64(y)
    ax = (0, 2, 3)
    return {"s": (dz.sum(ax), sc.C["bn_bwd_sum"] * U24 * dga.sum(ax) + ddz.sum(ax)),
            "q": ((dz * y).sum(ax), (sc.C["bn_bwd_sumsq"] + 1.0) * U24 * (dga * y.abs()).sum(ax) + (ddz * y.abs()).sum(ax))}


def coef_bwd(s, q, n, gamma, mean, invstd, pdt=F32, ds=0.0, dq=0.0):
    """-> {"dbeta", "dgamma": (ref, noise); "A", "B", "D": double; "dB", "dD": their input error}"""
    g, mu, inv = d64(gamma), d64(mean), d64(invstd)
    lo = 0.0 if pdt == F32 else U24
    dg = inv * (q - mu * s)
    ddg = inv.abs() * (dq + mu.abs() * ds)
    k0, c1, c2 = g * inv, s / n, dg / n
    return {"dbeta": (s, ds + lo * s.abs()), "dgamma": (dg, ddg + lo * dg.abs()),
            "A": k0, "B": -k0 * c2 * inv, "D": -k0 * c1 + k0 * c2 * mu * inv,
            "dB": (k0 * inv).abs() * ddg / n, "dD": k0.abs() * ds / n + (k0 * mu * inv).abs() * ddg / n}


def bwd_apply(dz, ddz, y, a, b=None, d=None, db=0.0, dd=0.0):
    """dy = A dz + B y + D -> (dy, noise); b = d = None: the eval-mode backward"""
    y, a = d64(y), _bc(d64(a))
    if b is None:
        return a * dz, a.abs() * ddz + 4.0 * U24 * (a * dz).abs()
    b, d = _bc(b), _bc(d)
    db = _bc(db) if torch.is_tensor(db) else db
    dd = _bc(dd) if torch.is_tensor(dd) else dd
    return a * dz + b * y + d, a.abs() * ddz + 4.0 * U24 * ((a * dz).abs() + (b * y).abs() + d.abs()) + db * y.abs() + dd


# ---------------------------------------------------------------------------------------------- the comparison
def assert_within(got, ref_noise, dtype, what, family, old=None):
    """got: (N, C, H, W) or a per-channel vector (C,); ref_noise: (ref, noise) float64 of that shape.  Limit:
    u_dtype(max(|ref|, |got|)) + noise.  old: the absolute limit asserted before (guard 'nowhere wider')."""
    ref, noise = ref_noise
    got = got.detach().to("cpu")
    if got.dim() == 1:
        got, ref, noise = got.view(1, -1, 1), ref.view(1, -1, 1), noise.view(1, -1, 1)
    try:
        return sc.assert_close(got, ref, noise / U24, dtype, what, family=family, c=1.0, old_abs=old if GUARD else None)
    except StrictMismatch as ex:
        raise StrictMismatch(f"[BatchNorm: c = 1 on M = noise / 2^-24, the noise budget of strict_bn.py at c = "
                             f"{sc.C.get(family, sc.C_DEFAULT):g}; a per-channel vector is one 'image' of C 'channels']\n{ex}",
                             ex.count, ex.hist, ex.worst) from None


class Case:
    """the inputs of one BatchNorm layer, on the CPU: y, dout, res (N, C, H, W) in `dtype`; gamma, beta in pdt; rmean, rvar
    (the running statistics BEFORE the step) in bdt"""

    def __init__(self, cls, n, c, h, w, dtype, act, with_res=False, pdt=F32, bdt=F32, seed=0, momentum=0.03, eps=1e-3):
        self.cls, self.shape, self.dtype, self.act, self.pdt, self.bdt = cls, (n, c, h, w), dtype, act, pdt, bdt
        self.momentum, self.eps, self.count = momentum, eps, n * h * w
        self.y = make_y(cls, n, c, h, w, dtype, seed)
        g = torch.Generator().manual_seed(400 + seed)
        self.dout = torch.randn(min(n, 3), c, h, w, generator=g)[image_pattern(n, seed + 1)].to(dtype)
        self.res = torch.randn(min(n, 3), c, h, w, generator=g)[image_pattern(n, seed + 2)].to(dtype) if with_res else None
        self.gamma, self.beta = (1 + 0.1 * torch.randn(c, generator=g)).to(pdt), (0.1 * torch.randn(c, generator=g)).to(pdt)
        self.rmean, self.rvar = (0.1 * torch.randn(c, generator=g)).to(bdt), (1 + 0.1 * torch.randn(c, generator=g).abs()).to(bdt)
        self.what = f"{cls} {n}x{c}x{h}x{w} {str(dtype)[6:]} act {act}"


def _guard(case, ref, mult=1.0):
    return old_abs(ref, case.dtype, mult) if case.count >= GUARD_MIN_COUNT else None


def check_sums(case, s, q=None, x=None, what="stats"):
    """(sum x, sum x^2) per channel of x (default: the layer's y), as folded from the accumulator or as channel_sum gives it"""
    r = sums_fwd(case.y if x is None else x, case.dtype)
    big = old_abs(r["s"][1] / (sc.C["bn_sum"] * U24), F32, 20.0)         # check(..., mult=20, scale=max sum |y|)
    assert_within(s, r["s"], F32, f"{case.what} {what} sum", "bn_sum", old=big)
    if q is not None:
        assert_within(q, r["q"], F32, f"{case.what} {what} sumsq", "bn_sumsq", old=old_abs(r["q"][0], F32, 20.0))
    return r


def check_coef(case, got, s, q, ds=0.0, dq=0.0, rmean=None, rvar=None, what="coef"):
    """got: (mean, invstd, scale, shift) fp32; s, q: the sums they were formed from (the kernel's own, or the float64 sums
    of y with their limit as ds, dq); rmean / rvar: the running statistics AFTER the step, where the call updated them"""
    r = coef_fwd(s, q, case.count, case.eps, case.gamma, case.beta, case.rmean, case.rvar, case.momentum, ds, dq)
    for g, nm in zip(got, ("mean", "invstd", "scale", "shift")):
        assert_within(g, r[nm], F32, f"{case.what} {what} {nm}", "bn_coef")
    if rmean is not None:
        assert rmean.dtype == case.bdt and rvar.dtype == case.bdt, (rmean.dtype, rvar.dtype, case.bdt)
        assert_within(rmean, r["rmean"], case.bdt, f"{case.what} {what} running_mean", "bn_coef")
        assert_within(rvar, r["rvar"], case.bdt, f"{case.what} {what} running_var", "bn_coef")
    return r


def check_out(case, out, scale, shift, res=None, mult=1.0, what="out"):
    r = fwd_apply(case.y, scale, shift, case.act, res)
    assert_within(out, r, case.dtype, f"{case.what} {what}", "bn_fwd", old=_guard(case, r[0], mult))


def check_bwd(case, scale, shift, mean, invstd, dy, dgamma, dbeta, acc=None, what="bwd"):
    """the backward from the published scale, shift, mean, invstd.  acc = (S~, Q~): the kernel's own accumulator, checked
    against the float64 sums and then taken as the coefficients' input (stage-wise); None: the float64 sums with their
    limit as the input error (the deterministic path exposes no partial rows)"""
    dz, ddz, dga = bwd_dz(case.dout, case.y, scale, shift, case.act)
    sums = sums_bwd(dz, ddz, dga, case.y)
    if acc is not None:
        assert_within(acc[0], sums["s"], F32, f"{case.what} {what} sum dz", "bn_bwd_sum")
        assert_within(acc[1], sums["q"], F32, f"{case.what} {what} sum dz y", "bn_bwd_sumsq")
        k = coef_bwd(acc[0], acc[1], case.count, case.gamma, mean, invstd, case.pdt)
    else:
        k = coef_bwd(sums["s"][0], sums["q"][0], case.count, case.gamma, mean, invstd, case.pdt, sums["s"][1], sums["q"][1])
    assert dgamma.dtype == case.pdt and dbeta.dtype == case.pdt, (dgamma.dtype, dbeta.dtype, case.pdt)
    assert_within(dbeta, k["dbeta"], case.pdt, f"{case.what} {what} dbeta", "bn_dbeta")
    assert_within(dgamma, k["dgamma"], case.pdt, f"{case.what} {what} dgamma", "bn_dgamma")
    r = bwd_apply(dz, ddz, case.y, k["A"], k["B"], k["D"], k["dB"], k["dD"])
    # check(dy, ..., mult=2): the guard holds stage-wise.  Composed with the sums' limit the dy limit is wide by construction
    # (under `offset`, and in fp32 at a handful of pixels): there the former assertion itself stays, on the plain inputs of
    # tests/test_gpu_kernels.py
    guard = _guard(case, r[0], 2.0) if acc is not None else None
    assert_within(dy, r, case.dtype, f"{case.what} {what} dy", "bn_dy", old=guard)
    return k


def check_bwd_eval(case, scale, shift, dy, what="bwd eval"):
    dz, ddz, _ = bwd_dz(case.dout, case.y, scale, shift, case.act)
    r = bwd_apply(dz, ddz, case.y, scale)
    assert_within(dy, r, case.dtype, f"{case.what} {what} dy", "bn_dy", old=_guard(case, r[0]))


def truth(case):
    """float64 from the INPUTS alone (not from any accumulator): invstd and dgamma, for the headroom figures"""
    s = sums_fwd(case.y, case.dtype)
    k = coef_fwd(s["s"][0], s["q"][0], case.count, case.eps, case.gamma, case.beta)
    dz, ddz, dga = bwd_dz(case.dout, case.y, k["scale"][0], k["shift"][0], case.act)
    b = sums_bwd(dz, ddz, dga, case.y)
    kb = coef_bwd(b["s"][0], b["q"][0], case.count, case.gamma, k["mean"][0], k["invstd"][0])
    return {"invstd": k["invstd"][0], "dgamma": kb["dgamma"][0],
            "dgamma_mass": k["invstd"][0] * ((dz * d64(case.y)).abs().sum((0, 2, 3)))}


def verify_accumulator_path(case, r):
    """r: what bn_stats_acc -> bn_act_fwd_train (or bn_finalize_acc) -> bn_act_bwd_train left behind: acc_f, acc_b (fp32
    [8][2][C], read AFTER the calls), mean, invstd, scale, shift, rmean, rvar (updated), out, dy, dgamma, dbeta; any may be
    missing (then its stage is not compared).  Every stage from the buffers it received."""
    c = case.shape[1]
    s, q = fold(r["acc_f"], c)
    check_sums(case, s, q, what="acc")
    check_coef(case, [r[k] for k in ("mean", "invstd", "scale", "shift")], s, q, rmean=r.get("rmean"), rvar=r.get("rvar"), what="acc")
    if "out" in r:
        check_out(case, r["out"], r["scale"], r["shift"], case.res, mult=2.0, what="acc out")
    if "dy" in r:
        check_bwd(case, r["scale"], r["shift"], r["mean"], r["invstd"], r["dy"], r["dgamma"], r["dbeta"], acc=fold(r["acc_b"], c),
                  what="acc bwd")


def verify_deterministic_path(case, r):
    """r: bn_train_stats -> bn_act_fwd -> bn_act_bwd / bn_act_bwd_eval, channel_sum(dout), bn_eval_coeffs(updated running
    statistics): mean, invstd, scale, shift, rmean, rvar, out, dy, dgamma, dbeta, dy_eval, csum, eval_scale, eval_shift.  The
    partial rows are not exposed: the sums' limit enters the coefficients' as their input error."""
    t = sums_fwd(case.y, case.dtype)
    check_coef(case, [r[k] for k in ("mean", "invstd", "scale", "shift")], t["s"][0], t["q"][0], t["s"][1], t["q"][1],
               rmean=r.get("rmean"), rvar=r.get("rvar"), what="det")
    check_out(case, r["out"], r["scale"], r["shift"], case.res, what="det out")
    check_bwd(case, r["scale"], r["shift"], r["mean"], r["invstd"], r["dy"], r["dgamma"], r["dbeta"], what="det bwd")
    check_bwd_eval(case, r["scale"], r["shift"], r["dy_eval"])
    check_sums(case, r["csum"], x=case.dout, what="channel_sum")
    e = coef_eval(case.gamma, case.beta, r["rmean"], r["rvar"], case.eps)
    assert_within(r["eval_scale"], e["scale"], F32, f"{case.what} eval scale", "bn_coef")
    assert_within(r["eval_shift"], e["shift"], F32, f"{case.what} eval shift", "bn_coef")
