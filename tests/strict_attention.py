"""Strict per-element comparator for the attention kernels (csrc/attention.hip, csrc/attention_fused.hip): float64
references and derived limits, on top of strict_compare.py (its ulp(), StrictMismatch, OBSERVED / report() and failure
histograms).  Shared by tests/test_strict_attention_cpu.py (the proof of the comparator) and the -m gpu tests.

Everything here works on float64 tensors of shape (B, T, d), B = image * heads + head, built by split() from the very
buffers the kernel reads (so the 16-bit inputs are exact).  Notation: u(x) = 1/2 ulp_T(x) (strict_compare.ulp: f16
subnormals included); U = 2^-24; c = 16 (C below, per family, the rule of strict_compare.py applies); for query i and key j
s = scale q_i.k_j, Ms = scale |q_i|.|k_j|.

Forward, 16-bit routes.  The kernels form p~_ij = exp(s_ij - m_i) in fp32, l_i = sum_j p~_ij, and
o = sum_j round_T(p~_ij) v_j / l_i, rounded once.  m_i cancels in the quotient: no error term for it (the key-blocked
kernel only moves m between blocks; every rescale is one more exp of the same model and one multiply).  One p~_ij has the
relative error
    e_ij = c U Ms_ij  +  (|s_ij - m_i| + 4) 2^-22  +  U |s_ij|
(fp32 sum of exact products; the __expf model of strict_compare's E_act: multiply by log2 e, exp2, about an ulp each,
doubled; the multiply by scale).  Numerator and denominator both carry at most max_j e_ij, the fp32 sums of the
numerator (MFMA accumulation) and of l add c U: E_i = 2 max_j e_ij + c U.  With P = p~ / l:
    |got - o|  <=  u(max(|o|, |got|))  +  sum_j u(p~_ij) |v_jd| / l_i  +  E_i sum_j P_ij |v_jd|
The batched-GEMM route rounds the NORMALISED probability and does not divide afterwards: u(P_ij) replaces u(p~_ij) / l_i.
The fp32 route rounds nothing in between: the middle term is dropped and ulp is fp32's.
Stashes.  Fused / fp32 routes, row log-sum-exp (fp32): |got - lse| <= max_j e_ij + 4 U max(1, |lse|) (m is exact, log(l)
carries l's relative error as an absolute one, __logf and the add a few ulps of fp32; coded as 3 U max(1, |lse|) plus the
comparator's own 1/2 ulp_fp32 <= U |lse|).  GEMM route, stashed P: u(P) + e_ij P_ij.

Backward: the float64 evaluation of the formulas in the kernels' header comments from exactly the buffers the kernel
receives.  Fused and fp32 routes read the forward's STORED o and lse:
    P = exp(s - lse_i)   dP = dO_i.v_j   D_i = sum_d dO_id o_id   dS = P (dP - D) scale
    dQ = sum_j dS k_j    dK = sum_i dS q_i    dV = sum_i P dO_i + d_vp
The GEMM route never reads o: P is its stash, D_i = sum_j P_ij dP_ij, nothing else changes.  e is as above with lse_i for
m_i, plus U |lse_i| (the stored fp32 value is used as it is; the subtraction rounds once).  Per pair (i, j):
    A_ij = P scale [ e |dP - D| + c U (sum_d |dO_id| |v_jd| + MD_i) ]  +  3 U |dS|  +  u(dS)
           (P's relative error on the product; the fp32 sums behind dP and D, MD_i = sum_d |dO_id| |o_id| -- GEMM route:
           sum_j P_ij sum_d |dO_id| |v_jd|, the mass of the sum it forms; three fp32 operations; dS rounded to T.
           The GEMM route rounds x = P (dP - D) and multiplies by scale in the next product: its last term is
           scale u(x), which is u(dS) when scale is a power of two (dk 16) and up to sqrt 2 either side of it at dk 32;
           with u(dS) the CPU stand-in of that route left 13 of 29696 dQ elements out at 449 sharpened tokens.)
    B_ij = u(P) + e P                                    (P rounded to T for the dV product)
    dQ: sum_j A_ij |k_jc| + c U sum_j |dS_ij| |k_jc|     dK: the same over i with |q_ic|
    dV: sum_i B_ij |dO_id| + c U (sum_i P_ij |dO_id| + |d_vp_jd|)
each plus u(output).  fp32 route: the u(.) terms inside A and B are dropped and ulp is fp32's.  dQ, dK and dV are three
tensors under three family names: the magnitude of one never excuses another.

What strict_compare.assert_close receives: (B, d, T padded to a multiple of 16) with c = 1 and mass = noise / U, so its
limit IS 1/2 ulp + noise, its 'image' axis is image * heads + head, its 16-pixel blocks are 16-token blocks of one
(image, head) and its channel blocks 16-channel blocks; the figure it records per family is the largest share of the
noise budget used, (|got - ref| - 1/2 ulp) / noise, limit 1.

Observed on the MI355X (largest share of the noise budget per family; c = 16 held everywhere): see DESIGN.md, 'What the
attention tests can see'.  The CPU stand-ins' maxima are in tests/test_strict_attention_cpu.py."""
import math

import torch

import strict_compare as sc
from strict_compare import U24, StrictMismatch, ulp  # noqa: F401  (re-exported for the tests)

ROUTES = ("fused", "long", "gemm", "fp32")
FAMILIES = ([f"attn_{r}_{t}" for r in ("fused", "gemm", "fp32") for t in ("o", "dq", "dk", "dv")] +
            ["attn_long_o", "attn_fused_lse", "attn_fp32_lse", "attn_gemm_p"])
for _f in FAMILIES:
    sc.C[_f] = sc.C_DEFAULT
    sc.BUDGET_FAMILIES.add(_f)
CLASSES = ("plain", "sharp", "negative")


def hw(t):
    """an h x w map with h * w = t tokens, as square as t allows"""
    h = max(d for d in range(1, int(math.isqrt(t)) + 1) if t % d == 0)
    return h, t // h


def make_qkv(n, heads, dk, dh, t, cls, seed, dtype):
    """(n, heads * (2 dk + dh), h, w) in `dtype`, n distinct images.  plain: unit Gaussians; sharp: q and k of every head
    x 2.5 (row maxima of neighbouring key blocks differ by several units); negative: q = |q|, k = -|k| - 0.5, every score
    below zero, so that a spurious zero-score key outweighs the real ones."""
    assert cls in CLASSES
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, heads, 2 * dk + dh, t, generator=g)
    if cls == "sharp":
        x[:, :, :2 * dk] *= 2.5
    elif cls == "negative":
        x[:, :, :dk] = x[:, :, :dk].abs()
        x[:, :, dk:2 * dk] = -x[:, :, dk:2 * dk].abs() - 0.5
    return x.reshape(n, heads * (2 * dk + dh), *hw(t)).to(dtype)


def split(t, heads):
    """(N, heads * d, H, W), any device / layout -> float64 (N * heads, T, d)"""
    n, c = t.shape[:2]
    x = t.detach().to("cpu", torch.float64).reshape(n, heads, c // heads, -1)
    return x.transpose(2, 3).reshape(n * heads, -1, c // heads)


def split_qkv(qkv, heads, dk, dh):
    x = split(qkv, heads)
    return x[..., :dk], x[..., dk:2 * dk], x[..., 2 * dk:]


def merge(x, n, h, w):
    """(N * heads, T, d) -> (N, heads * d, H, W)"""
    b, t, d = x.shape
    return x.reshape(n, b // n, t, d).transpose(2, 3).reshape(n, b // n * d, h, w)


def head_pattern(pattern, heads):
    return [p * heads + h for p in pattern for h in range(heads)]


def _u(x, dtype, route):
    return torch.zeros_like(x) if route == "fp32" else 0.5 * ulp(x, dtype)


def forward(q, k, v, scale, dtype, route, c=sc.C_DEFAULT):
    """-> dict: o, o_noise (B, T, dh); lse, lse_noise (B, T, 1); P, P_noise (B, T, T)"""
    assert route in ROUTES
    s = scale * (q @ k.mT)
    ms = scale * (q.abs() @ k.abs().mT)
    m = s.amax(-1, keepdim=True)
    pt = torch.exp(s - m)
    l = pt.sum(-1, keepdim=True)
    p = pt / l
    e = c * U24 * ms + ((s - m).abs() + 4.0) * 2.0 ** -22 + U24 * s.abs()
    emax = e.amax(-1, keepdim=True)
    big_e = 2.0 * emax + c * U24
    va = v.abs()
    if route == "gemm":
        mid = _u(p, dtype, route) @ va
    else:
        mid = (_u(pt, dtype, route) @ va) / l
    lse = m + torch.log(l)
    return {"o": p @ v, "o_noise": mid + big_e * (p @ va),
            "lse": lse, "lse_noise": emax + 3.0 * U24 * lse.abs().clamp_min(1.0),
            "P": p, "P_noise": e * p}


def backward(q, k, v, d_o, d_vp, scale, dtype, route, o=None, lse=None, p_stash=None, c=sc.C_DEFAULT):
    """fused / fp32: o (B, T, dh) and lse (B, T, 1) as the forward STORED them; gemm: p_stash (B, T, T) as stored.
    -> dict: dq, dq_noise, dk, dk_noise, dv, dv_noise"""
    assert route in ("fused", "gemm", "fp32")
    s = scale * (q @ k.mT)
    ms = scale * (q.abs() @ k.abs().mT)
    dp = d_o @ v.mT
    mdp = d_o.abs() @ v.abs().mT
    if route == "gemm":
        p = p_stash
        lse = torch.logsumexp(s, -1, keepdim=True)
        d = (p * dp).sum(-1, keepdim=True)
        md = (p * mdp).sum(-1, keepdim=True)
    else:
        p = torch.exp(s - lse)
        d = (d_o * o).sum(-1, keepdim=True)
        md = (d_o.abs() * o.abs()).sum(-1, keepdim=True)
    e = c * U24 * ms + ((s - lse).abs() + 4.0) * 2.0 ** -22 + U24 * s.abs() + U24 * lse.abs()
    ds = p * (dp - d) * scale
    # the rounding of dS sits where the kernel has it: the fused kernels round P (dP - D) scale, the GEMM route rounds
    # P (dP - D) and leaves the scale to the next product
    u_ds = scale * _u(ds / scale, dtype, route) if route == "gemm" else _u(ds, dtype, route)
    a = p * scale * (e * (dp - d).abs() + c * U24 * (mdp + md)) + 3.0 * U24 * ds.abs() + u_ds
    b = _u(p, dtype, route) + e * p
    dsa, doa = ds.abs(), d_o.abs()
    out = {"dq": ds @ k, "dq_noise": a @ k.abs() + c * U24 * (dsa @ k.abs()),
           "dk": ds.mT @ q, "dk_noise": a.mT @ q.abs() + c * U24 * (dsa.mT @ q.abs()),
           "dv": p.mT @ d_o, "dv_noise": b.mT @ doa + c * U24 * (p.mT @ doa)}
    if d_vp is not None:
        out["dv"] = out["dv"] + d_vp
        out["dv_noise"] = out["dv_noise"] + c * U24 * d_vp.abs()
    return out


def assert_within(got, ref, noise, dtype, what, family, pattern=None, old_abs=None):
    """got (B', T, d) float64 / any float, ref and noise (B, T, d) float64; pattern: base row of ref for every row of got
    (default: the same row).  Limit: 1/2 ulp_dtype(max(|ref|, |got|)) + noise.  old_abs as in strict_compare."""
    t = got.shape[1]
    pad = -t % 16

    def lay(x):                                               # (B, T, d) -> (B, d, T padded to 16-token blocks)
        x = x.detach().to("cpu", torch.float64).transpose(1, 2)
        return torch.nn.functional.pad(x, (0, pad)) if pad else x
    try:
        return sc.assert_close(lay(got), lay(ref), lay(noise) / U24, dtype, what, family=family, c=1.0, pattern=pattern,
                               old_abs=old_abs)
    except StrictMismatch as ex:
        raise StrictMismatch(f"[attention: 'image' = image * heads + head; pixel blocks = 16-token blocks of one (image, head), "
                             f"{(t + pad) // 16} per row of the histogram; c = 1 on M = noise / 2^-24, the noise budget of "
                             f"strict_attention.py at c = {sc.C.get(family, sc.C_DEFAULT):g}]\n{ex}", ex.count, ex.hist, ex.worst) from None


# the limits check() applied to attention before (share of the tensor's largest magnitude): only for the guard
# 'nowhere wider than before'
OLD_O = {torch.float32: 2e-4, torch.bfloat16: 2.0 ** -5, torch.float16: 2.0 ** -8}
OLD_DQKV = {torch.float32: 4e-4, torch.bfloat16: 2.0 ** -4, torch.float16: 2.0 ** -7}
OLD_LSE_FP32 = 4e-4


def check_forward(route, q, k, v, scale, dtype, got_o, got_lse=None, got_p=None, pattern=None, what="", guard=True):
    """q, k, v: (bases * heads, T, d) float64 of the base images; got_*: (B', ...) of the kernel, row r against base row
    pattern[r].  Compares o (family attn_<route>_o) and, where given, the stash.  -> the reference dict"""
    f = forward(q, k, v, scale, dtype, route, sc.C[f"attn_{route}_o"])
    old = OLD_O[dtype] * max(float(f["o"].abs().max()), 1e-6) if guard else None
    assert_within(got_o, f["o"], f["o_noise"], dtype, f"{what} o", f"attn_{route}_o", pattern, old_abs=old)
    if got_lse is not None:
        old = OLD_LSE_FP32 * max(float(f["lse"].abs().max()), 1e-6) if guard and dtype == torch.float32 else None
        assert_within(got_lse, f["lse"], f["lse_noise"], torch.float32, f"{what} lse", f"attn_{route}_lse", pattern, old_abs=old)
    if got_p is not None:
        assert_within(got_p, f["P"], f["P_noise"], dtype, f"{what} stashed P", f"attn_{route}_p", pattern)
    return f


def check_backward(route, q, k, v, d_o, d_vp, scale, dtype, got_dq, got_dk, got_dv, o=None, lse=None, p_stash=None, what="",
                   guard=True):
    """every tensor (B, T, d) float64, row for row (the stored o / stash belong to one run: no pattern here)"""
    fam = "fused" if route == "long" else route
    b = backward(q, k, v, d_o, d_vp, scale, dtype, fam, o=o, lse=lse, p_stash=p_stash, c=sc.C[f"attn_{fam}_dq"])
    old = OLD_DQKV[dtype] * max(float(max(b["dq"].abs().max(), b["dk"].abs().max(), b["dv"].abs().max())), 1e-6) if guard else None
    for name, got in (("dq", got_dq), ("dk", got_dk), ("dv", got_dv)):
        assert_within(got, b[name], b[name + "_noise"], dtype, f"{what} {name}", f"attn_{fam}_{name}", old_abs=old)
    return b
