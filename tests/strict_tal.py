"""Strict comparator for the kernels of csrc/loss_tal.hip (k_tal_decode, k_tal_topk, k_tal_resolve, k_tal_final): the float64
reference of tests/tal_ref.py and derived limits, on top of strict_compare.py (ulp(), assert_close, StrictMismatch,
OBSERVED / report()) in the manner of strict_loss.py.  Shared by tests/test_tal_cpu.py (the proof of the comparator and the
CPU stand-in, no GPU) and tests/test_gpu_tal.py.

Every stage is compared with the float64 evaluation of its formula from exactly the buffers that stage receives (`State`: what
one launch left in its workspace): the decode from the rounded inputs (strict_loss.decode64, family loss_decode: it is the
same device code), the metrics and the top-k from the kernel's pbox, the owners from the kernel's lists, the targets from the
kernel's lists and owners, the gradients and the scalars from the kernel's pbox, (label, t) words and tss.

Arithmetic model: as strict_loss.py.  Inputs exact, fp32 without contraction, ONE rounding to T (after grad_scale, applied in
fp32).  U = 2^-24 relative per operation, 2 U for expf / logf / log1pf / atanf, c = 16 (sc.C per family) on summations only;
everything else is the first-order propagation of those roundings through the kernel's formula, carried next to the value
by the small `V` class below (value, absolute error): a + b, a * b, a / b propagate the operands' errors and add U |result|;
min / max keep the larger operand error; clamp(min = 0) keeps the error where it passes; a multiplication by a power of
two is exact.  The same code runs in float64 (the limits) and in fp32 (the CPU stand-in of the kernel).

Discrete stages, checked in float64:
    top-k     every chosen anchor is a float64 candidate, the count is min(topk, candidates); with m_k the k-th largest
              float64 metric among the candidates: metric(chosen) >= m_k - margin, metric(not chosen) <= m_k + margin,
              margin = e(chosen or not chosen) + e(k-th), e the propagated error of  sigm(x)^alpha iou^beta:  sigm 4 U,
              x^p = exp(p log x): |p| (3 U |log x| + e_x / x) + 2 U relative, the IoU through its corners, products and
              the division.  Where the gap between the k-th and the (k+1)-th metric exceeds the margin (or they are exactly
              equal: the lower anchor then has to be the one chosen) the chosen set must equal the reference's.  The stored
              align / iou are within e of their float64 values and the list is sorted by (align descending, anchor).
    owner     among the rows that chose an anchor the owner has iou >= max iou - margin (the stored fp32 iou are compared
              exactly as the kernel compares them: the owner must be THE maximum of the stored values, lower row first).
Value families (c = 1 on M = noise / U handed to assert_close, the recorded figure is a share of the budget, limit 1):
    tal_target   ma, mi (exact maxima of the stored values: noise 0), t = al mi / (ma + 1e-9) (3 roundings), per-row sum of t
    tal_dense    (s - t) lambda_cls / tss [grad_scale] for every class element; exact 0 for the box logits of anchors that are
                 not positives (NaN pattern of poisoned anchors asserted separately)
    tal_box      the 64 box-logit gradients of a positive: the CIoU chain term by term plus the DFL pair, through the
                 softmax of the side; reference by autograd in float64 (tal_ref.terms at the kernel's pbox)
    tal_scalars  out[4] and tss: c U on the sums of absolute terms + the propagated error of every term

Redraws: a random draw is rejected when, at a reference positive, a min / max or clamp operand pair of the CIoU is closer
than 2^-10 px without being equal, or when an anchor point is closer than 2^-10 px to a GT side without lying on it.  The
GT corners are drawn on the lattice k / 4 + 1 / 8 px, which no anchor point (a multiple of 4 px) comes near, so only the
first condition ever fires; make_case asserts that at most one draw in four is rejected.

Recorded maxima, largest share of the noise budget used per family (limit 1; c = 16 held for every family, none was raised):
RECORDED below.  MI355X: target 0.573, dense 0.295, box 0.120, scalars 0.068, decode 0.192, top-k and owner 0 (the float64
choice everywhere).  CPU stand-in: target 0.467, dense 0.294, box 0.094, scalars 0.030, decode 0.126, top-k and owner 0."""
import torch

import strict_compare as sc
import strict_loss as sl
import tal_ref as tr
from strict_compare import U24, StrictMismatch  # noqa: F401

F32, F64, BF, HF = torch.float32, torch.float64, torch.bfloat16, torch.float16
REG, KMAX = 16, 16
FAMILIES = ("tal_target", "tal_dense", "tal_box", "tal_scalars", "tal_topk", "tal_owner")
for _f in FAMILIES:
    sc.C[_f] = sc.C_DEFAULT
    sc.BUDGET_FAMILIES.add(_f)
GUARD_GAP = 2.0 ** -10
U = U24

# largest share of the noise budget used per family, (|got - ref| - u_T) / noise; tal_topk / tal_owner: largest share of
# the margin used by a chosen anchor / an owner that is not the float64 maximum (0: the float64 choice everywhere)
RECORDED = {
    "MI355X (tests/test_gpu_tal.py, 73 tests, 2026-10-19)":
        dict(loss_decode=0.192, tal_topk=0.000, tal_owner=0.000, tal_target=0.573, tal_dense=0.295, tal_box=0.120, tal_scalars=0.068),
    "CPU stand-in (tests/test_tal_cpu.py::test_stand_in_has_nothing_outside, STAND_IN_MAXIMA)":
        dict(loss_decode=0.126, tal_topk=0.000, tal_owner=0.000, tal_target=0.467, tal_dense=0.294, tal_box=0.094, tal_scalars=0.030),
}
# tal_topk / tal_owner 0.000: every chosen set and every owner was the float64 choice itself, on every case of both runs.
# Not measured: the error of expf / logf / log1pf / atanf on their own (the 2 U above is a model, checked through these shares
# only); topk other than 1, 10 and 13.


# ------------------------------------------------------------------------------------------- value with propagated error
class V:
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @staticmethod
    def of(x, like):
        return x if isinstance(x, V) else V(torch.as_tensor(x, dtype=like.v.dtype).expand_as(like.v))

    def _r(self, v, e):
        return V(v, e + U * v.abs())

    def __add__(self, o):
        o = V.of(o, self)
        return self._r(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o, self)
        return self._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return V.of(o, self) - self

    def __neg__(self):
        return V(-self.v, self.e)

    def __mul__(self, o):
        o = V.of(o, self)
        return self._r(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o, self)
        r = self.v / o.v
        return self._r(r, self.e / o.v.abs() + r.abs() * o.e / o.v.abs())

    def __rtruediv__(self, o):
        return V.of(o, self) / self

    def pow2(self, k):                      # exact scaling by a power of two
        return V(self.v * k, self.e * abs(k))

    def mask(self, m):                      # multiply by an exact 0 / 0.5 / 1 mask
        return V(self.v * m, self.e * m)

    def __getitem__(self, i):
        return V(self.v[i], self.e[i])


def vmin(a, b):
    return V(torch.minimum(a.v, b.v), torch.maximum(a.e, b.e))


def vmax(a, b):
    return V(torch.maximum(a.v, b.v), torch.maximum(a.e, b.e))


def vrelu(a):
    return V(a.v.clamp(min=0), a.e * (a.v >= 0))


def vexp(a):
    r = torch.exp(a.v)
    return V(r, r * a.e + 2 * U * r)


def vlog(a):
    r = torch.log(a.v)
    return V(r, a.e / a.v.abs() + 2 * U * r.abs())


def vlog1p(a):
    r = torch.log1p(a.v)
    return V(r, a.e / (1 + a.v) + 2 * U * r.abs())


def vatan(a):
    r = torch.atan(a.v)
    return V(r, a.e / (1 + a.v * a.v) + 2 * U * r.abs())


def vsum(a, dim, c):
    k = a.v.shape[dim]
    return V(a.v.sum(dim), a.e.sum(dim) + min(c, max(k - 1, 0)) * U * a.v.abs().sum(dim))


def vpow(x, p):
    """x^p = exp(p log x) for x > 0; 0 (1 for p = 0) at x = 0"""
    pos = x.v > 0
    safe = V(torch.where(pos, x.v, torch.ones_like(x.v)), torch.where(pos, x.e, torch.zeros_like(x.e)))
    r = vexp(vlog(safe) * float(p))
    at0 = 1.0 if p == 0 else 0.0
    return V(torch.where(pos, r.v, torch.full_like(r.v, at0)), torch.where(pos, r.e, torch.zeros_like(r.e)))


def lt_half(a, b):
    return (a < b).to(a.dtype) + 0.5 * (a == b).to(a.dtype)


# -------------------------------------------------------------------------------------------------------- the formulas
def gt_corners(rows):
    """rows (M, 5) in dt -> four V (the kernel computes gx - gw / 2 in fp32: one rounding)"""
    gx, gy, gw, gh = (V(rows[:, i]) for i in range(4))
    return gx - gw.pow2(0.5), gy - gh.pow2(0.5), gx + gw.pow2(0.5), gy + gh.pow2(0.5)


def box_corners(pb):
    cx, cy, w, h = (V(pb[..., i]) for i in range(4))
    return cx - w.pow2(0.5), cy - h.pow2(0.5), cx + w.pow2(0.5), cy + h.pow2(0.5)


def metric_chain(pb, rows, logit, alpha, beta):
    """pb (M, 4), rows (M, 5), logit (M,) in dt -> (align V, iou V): k_tal_topk's consider()"""
    X1, Y1, X2, Y2 = box_corners(pb)
    g = gt_corners(rows)
    iw, ih = vrelu(vmin(X2, g[2]) - vmax(X1, g[0])), vrelu(vmin(Y2, g[3]) - vmax(Y1, g[1]))
    inter = iw * ih
    den = (X2 - X1) * (Y2 - Y1) + (g[2] - g[0]) * (g[3] - g[1]) - inter + tr.EPS7
    iou = inter / den
    s = 1.0 / (1.0 + vexp(-V(logit)))
    return vpow(s, alpha) * vpow(iou, beta), iou


def ciou_chain(pb, rows):
    """-> (ciou V, [d ciou / d X1, Y1, X2, Y2] V): ciou_terms() of the kernel, operation by operation"""
    X1, Y1, X2, Y2 = box_corners(pb)
    g = gt_corners(rows)
    w1, h1, w2, h2 = X2 - X1, (Y2 - Y1) + tr.EPS7, g[2] - g[0], (g[3] - g[1]) + tr.EPS7
    iwr, ihr = vmin(X2, g[2]) - vmax(X1, g[0]), vmin(Y2, g[3]) - vmax(Y1, g[1])
    iw, ih = vrelu(iwr), vrelu(ihr)
    inter = iw * ih
    uni = w1 * h1 + w2 * h2 - inter + tr.EPS7
    iou = inter / uni
    cw, ch = vmax(X2, g[2]) - vmin(X1, g[0]), vmax(Y2, g[3]) - vmin(Y1, g[1])
    c2 = cw * cw + ch * ch + tr.EPS7
    sx, sy = (g[0] + g[2]) - (X1 + X2), (g[1] + g[3]) - (Y1 + Y2)
    rho2 = (sx * sx + sy * sy).pow2(0.25)
    da = vatan(w2 / h2) - vatan(w1 / h1)
    v = tr.KV * da * da
    av = v / (v - iou + 1.0 + tr.EPS7)
    pen = rho2 / c2
    pw, ph = (iwr.v >= 0).to(pb.dtype), (ihr.v >= 0).to(pb.dtype)
    dI = [-(ih.mask(pw * lt_half(g[0].v, X1.v))), -(iw.mask(ph * lt_half(g[1].v, Y1.v))),
          ih.mask(pw * lt_half(X2.v, g[2].v)), iw.mask(ph * lt_half(Y2.v, g[3].v))]
    dA = [-h1, -w1, h1, w1]
    kA = inter / (uni * uni)
    kI = 1.0 / uni + kA
    dC = [-(cw.pow2(2.0).mask(lt_half(X1.v, g[0].v))), -(ch.pow2(2.0).mask(lt_half(Y1.v, g[1].v))),
          cw.pow2(2.0).mask(lt_half(g[2].v, X2.v)), ch.pow2(2.0).mask(lt_half(g[3].v, Y2.v))]
    dR = [-(sx.pow2(0.5)), -(sy.pow2(0.5)), -(sx.pow2(0.5)), -(sy.pow2(0.5))]
    kP = rho2 / (c2 * c2)
    kv = (da * tr.KV).pow2(-2.0) / (w1 * w1 + h1 * h1)
    dV = [-(kv * h1), kv * w1, kv * h1, -(kv * w1)]
    dc = [(kI * dI[k] - kA * dA[k]) - (dR[k] / c2 - kP * dC[k]) - av * dV[k] for k in range(4)]
    return iou - (pen + v * av), dc


def softmax_side(x):
    """x (M, 4, 16) exact -> p (M, 4, 16), lse (M, 4, 1), ev (M, 4, 1) as V: side_softmax() of the kernel"""
    c = sc.C["tal_box"]
    mx = x.amax(2, keepdim=True)
    ex = vexp(V(x) - V(mx.expand_as(x)))
    ssum = vsum(ex, 2, c)
    ssum = V(ssum.v.unsqueeze(2), ssum.e.unsqueeze(2))
    p = ex / V(ssum.v.expand_as(x), ssum.e.expand_as(x))
    lse = V(mx) + vlog(ssum)
    bins = torch.arange(REG, dtype=x.dtype).view(1, 1, REG)
    ev = vsum(p * V(bins.expand_as(x)), 2, c)
    return p, lse, V(ev.v.unsqueeze(2), ev.e.unsqueeze(2))


def positives_chain(x, pb, rows, anchors, strides, t, tss, hyper, gsc):
    """x (M, 64) box logits, pb (M, 4), rows (M, 5), anchors (M, 2), strides (M,), t (M,) in dt, tss V (M,)
    -> (grad V (M, 64) incl. grad_scale, box_e V (M,) = t (1 - ciou), dfl_e V (M,) = t dfl): positive_part() of the kernel"""
    dt = x.dtype
    m = x.shape[0]
    xs = x.view(m, 4, REG)
    p, lse, ev = softmax_side(xs)
    bins = torch.arange(REG, dtype=dt).view(1, 1, REG).expand(m, 4, REG)
    g = gt_corners(rows)
    ax, ay, st = V(anchors[:, 0]), V(anchors[:, 1]), V(strides)
    px, py = ax * st, ay * st
    tvs = [(px - g[0]) / st, (py - g[1]) / st, (g[2] - px) / st, (g[3] - py) / st]
    tv = V(torch.stack([q.v for q in tvs], 1), torch.stack([q.e for q in tvs], 1))
    inside = (tv.v >= 0) & (tv.v <= tr.CLAMP)
    tv = V(tv.v.clamp(0.0, tr.CLAMP), tv.e * inside)
    lo = tv.v.floor()
    wl, wr = (lo + 1.0) - tv, tv - lo
    oh_lo, oh_hi = (bins == lo[:, :, None]).to(dt), (bins == lo[:, :, None] + 1.0).to(dt)
    # the floor may fall on the other side of an integer within the target's own error: weight <= e_tv moves one bin over
    near_lo, near_hi = (wr.v <= tv.e).to(dt)[:, :, None], (wl.v <= tv.e).to(dt)[:, :, None]
    spill = ((bins == lo[:, :, None] - 1.0).to(dt) * near_lo + (bins == lo[:, :, None] + 2.0).to(dt) * near_hi) * tv.e[:, :, None]
    lx = V(lse.v.expand(m, 4, REG), lse.e.expand(m, 4, REG)) - V(xs)
    wl3, wr3 = V(wl.v[:, :, None].expand(m, 4, REG), wl.e[:, :, None].expand(m, 4, REG)), \
        V(wr.v[:, :, None].expand(m, 4, REG), wr.e[:, :, None].expand(m, 4, REG))
    contrib = (wl3 * lx).mask(oh_lo) + (wr3 * lx).mask(oh_hi)
    dfl = vsum(V(contrib.v.reshape(m, 64), contrib.e.reshape(m, 64)), 1, sc.C["tal_box"]).pow2(0.25)
    gbody = p - wl3.mask(oh_lo) - wr3.mask(oh_hi)
    gbody = V(gbody.v, gbody.e + spill)
    tV = V(t)
    cd = (hyper["dfl"] * tV / tss).pow2(0.25)
    cd3 = V(cd.v[:, None, None].expand(m, 4, REG), cd.e[:, None, None].expand(m, 4, REG))
    gacc = cd3 * gbody
    ciou, dc = ciou_chain(pb, rows)
    cb = hyper["box"] * tV / tss
    sign = (1.0, 1.0, -1.0, -1.0)
    gs = [(st * (cb * dc[k])) if sign[k] > 0 else (-st) * (cb * dc[k]) for k in range(4)]
    gs = V(torch.stack([q.v for q in gs], 1)[:, :, None].expand(m, 4, REG), torch.stack([q.e for q in gs], 1)[:, :, None].expand(m, 4, REG))
    evx = V(ev.v.expand(m, 4, REG), ev.e.expand(m, 4, REG))
    gacc = gacc + gs * p * (V(bins) - evx)
    if gsc is not None:
        gacc = gacc * float(gsc)
    return V(gacc.v.reshape(m, 64), gacc.e.reshape(m, 64)), tV * (1.0 - ciou), tV * dfl


def dense_chain(xc, target, tss, lam_cls, gsc):
    """xc (N, nc, A) class logits, target (N, nc, A) in dt, tss V scalar-shaped -> (grad V, value V): dense_part() of the kernel"""
    x = V(xc)
    ab = xc.abs()
    ex = vexp(V(-ab))
    den = 1.0 + ex
    s_pos, s_neg = 1.0 / den, ex / den
    ge = xc >= 0
    s = V(torch.where(ge, s_pos.v, s_neg.v), torch.where(ge, s_pos.e, s_neg.e))
    val = V(xc.clamp(min=0)) - x * V(target) + vlog1p(ex)
    coef = lam_cls / tss
    if gsc is not None:
        coef = coef * float(gsc)
    coef = V(coef.v.expand_as(xc), coef.e.expand_as(xc))
    return (s - V(target)) * coef, val


# ------------------------------------------------------------------------------------------------------ cases and state
class Case:
    """preds (N, 64 + nc, A), anchors (2, A), strides (1, A) in `dtype` on the CPU; gts: N tensors (M, 5) fp32"""

    def __init__(self, preds, anchors, strides, gts, nc, dtype, what, hyper=None, grad_scale=None, capacity=None):
        self.preds, self.anchors, self.strides = preds.to(dtype), anchors.to(dtype), strides.to(dtype)
        self.gts = [g.reshape(-1, 5).to(F32) for g in gts]
        self.nc, self.dtype, self.what, self.grad_scale = nc, dtype, what, grad_scale
        self.hyper = dict(tr.DEFAULTS, **(hyper or {}))
        self.N, _, self.A = preds.shape
        self.capacity = capacity            # StaticTargets: rows of the buffers (> live count), the spare rows hold garbage
        self.props = {}
        self.tss = None                     # override: the case is a slice of a larger batch
        self.redraws = 0

    @property
    def gt(self):
        live = [g for g in self.gts if g.shape[0]]
        return torch.cat(live) if live else torch.zeros(0, 5)

    @property
    def img(self):
        return torch.tensor([i for i, g in enumerate(self.gts) for _ in range(g.shape[0])], dtype=torch.long)

    def f(self, dt):
        return self.preds.to(dt), self.anchors.to(dt), self.strides.to(dt)


class State:
    """what one launch leaves behind, on the CPU: pbox (N, A, 4) f32; lists: per live row [(anchor, align, iou)] from the
    stored fp32 values; owner (N, A) long, -1 none; label (N, A) long (-1 none, -2 poisoned); t (N, A) f32; ma, mi, ts (G,)
    f32; tss float; out (4,) f32; dp (N, 64 + nc, A) or None"""

    def __init__(self, pbox, lists, owner, label, t, ma, mi, ts, tss, out, dp):
        self.pbox, self.lists, self.owner, self.label, self.t = pbox, lists, owner, label, t
        self.ma, self.mi, self.ts, self.tss, self.out, self.dp = ma, mi, ts, tss, out, dp

    @staticmethod
    def from_views(v, g_live, out, dp):
        """v: ops.loss_tal_workspace_views(...) moved to the CPU"""
        lists = [[(int(v["la"][j, r]), float(v["lal"][j, r]), float(v["lio"][j, r])) for r in range(int(v["cnt"][j]))]
                 for j in range(g_live)]
        low = v["owner"] & 0xffffffff
        owner = torch.where(v["owner"] == 0, torch.full_like(low, -1), 0xffffffff - low)
        return State(v["pbox"].clone(), lists, owner, v["tl"][..., 0].long(), v["tl"][..., 1].contiguous().view(F32).clone(),
                     v["gma"][:g_live].clone(), v["gmi"][:g_live].clone(), v["gts"][:g_live].clone(), float(v["tss"][0]), out, dp)


def lattice(g, lo, hi):
    """a coordinate on the lattice k / 4 + 1 / 8 in [lo, hi)"""
    return float(torch.randint(int(lo * 4), int(hi * 4), (1,), generator=g)) / 4 + 0.125


def rand_gt(g, w, h, cls, wmin=6.0, wmax=0.7):
    x1, y1 = lattice(g, 0, w - wmin - 1), lattice(g, 0, h - wmin - 1)
    x2, y2 = lattice(g, x1 + wmin, min(w, x1 + wmin + wmax * w)), lattice(g, y1 + wmin, min(h, y1 + wmin + wmax * h))
    return [(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, float(cls)]


def box_gt(x1, y1, x2, y2, cls):
    return [(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, float(cls)]


def reference(case):
    """the pure float64 reference of the case -> (assignment, terms)"""
    return tr.loss(case.preds, case.anchors, case.strides, case.gts, case.hyper, case.grad_scale)


def guard_ok(case, asg=None):
    p, an, st = case.f(F64)
    if asg is None:
        asg = tr.assign(p, tr.decode(p, an, st), an, st, case.gts, case.hyper)
    gt = case.gt.to(F64)
    for j in range(gt.shape[0]):
        d = tr.inside(gt[j], an, st)
        if bool(((d.abs() < GUARD_GAP) & (d != 0)).any()):
            return False
    pos = (asg["label"] >= 0).nonzero()
    if pos.numel():
        pb = tr.decode(p, an, st)[pos[:, 0], pos[:, 1]]
        X1, Y1, X2, Y2 = tr.corners(pb)
        g = tr.corners(gt[asg["owner"][pos[:, 0], pos[:, 1]]][:, :4])
        iwr, ihr = torch.minimum(X2, g[2]) - torch.maximum(X1, g[0]), torch.minimum(Y2, g[3]) - torch.maximum(Y1, g[1])
        diffs = torch.stack([X2 - g[2], X1 - g[0], Y2 - g[3], Y1 - g[1], iwr, ihr])
        if bool(((diffs.abs() < GUARD_GAP) & (diffs != 0)).any()):
            return False
    return True


def grid_index(w, level, col, row):
    """index of the anchor (col, row) of `level` (0: stride 8, ...) in make_anchors(h, w); h = 64"""
    off = 0
    for lv in range(level):
        s = 8 << lv
        off += (64 // s) * (w // s)
    return off + row * (w // (8 << level)) + col


def make_case(n, w, nc, dtype, seed=0, empty=(), hyper=None, grad_scale=None, built=True, h=64, fill=2, capacity=None):
    """anchors of an h x w input (h = 64 for the built sets) around a random fill; the built target sets of tests/test_gpu_tal.py,
    every property asserted here on the CPU against the float64 reference.  At most one draw in four may be rejected."""
    rejected = 0
    for attempt in range(12):
        case = _make_case(n, w, h, nc, dtype, seed + 1000 * attempt, tuple(empty), hyper, grad_scale, built, fill, capacity)
        if guard_ok(case):
            case.redraws = rejected
            if built:
                _assert_built(case)
            return case
        rejected += 1
        assert rejected <= 1 + attempt // 4, f"{rejected} of {attempt + 1} draws rejected: more than one in four"
    raise RuntimeError("no case found")


def _make_case(n, w, h, nc, dtype, seed, empty, hyper, grad_scale, built, fill, capacity):
    g = torch.Generator().manual_seed(9000 + seed)
    anchors, strides = tr.make_anchors(h, w)
    a = anchors.shape[1]
    preds = torch.randn(n, 64 + nc, a, generator=g)
    preds[:, 64:] = preds[:, 64:] * 0.9 - 2.0
    live = [i for i in range(n) if i not in empty]
    rows = {i: [] for i in range(n)}
    props = {}
    if built and live:
        i0, i1, i2 = live[0], live[len(live) // 2], live[-1]
        c_hi, c_mid = nc - 1, nc // 2
        # ---- image i0: more than topk candidates on every level; 1, 2 and 3 candidates; no anchor centre at all
        rows[i0].append(box_gt(2.125, 2.125, w - 2.125, 61.875, 0))
        rows[i0].append(box_gt(10.125, 10.125, 14.125, 14.125, c_hi))                 # (12, 12) only
        rows[i0].append(box_gt(34.125, 10.125, 46.125, 14.125, c_mid))                # (36, 12), (44, 12)
        rows[i0].append(box_gt(34.125, 50.125, 54.125, 54.125, 0))                    # (36, 52), (44, 52), (52, 52)
        rows[i0].append(box_gt(5.125, 21.125, 7.125, 23.125, c_hi))                   # none
        props["many"], props["few"], props["none"] = (i0, 0), [(i0, 1, 1), (i0, 2, 2), (i0, 3, 3)], (i0, 4)
        # ---- image i1: two overlapping GTs that contest anchors; two identical rows
        b = len(rows[i1])
        rows[i1].append(box_gt(6.125, 6.125, 40.125, 42.125, 0))
        rows[i1].append(box_gt(20.125, 18.125, 58.125, 60.125, c_hi))
        rows[i1].append(box_gt(w - 30.125, 2.125, w - 2.125, 30.125, c_mid))
        rows[i1].append(box_gt(w - 30.125, 2.125, w - 2.125, 30.125, c_mid))
        props["contest"], props["twins"] = (i1, b, b + 1), (i1, b + 2, b + 3)
        kc = grid_index(w, 0, 3, 4)                            # the point (28, 36) lies in both: a tight box [20, 44]^2 and a high
        preds[i1, :64, kc] = 0.0                               # score for both labels make it the first choice of both rows
        for side, b_ in enumerate((1, 2, 2, 1)):
            preds[i1, side * REG + b_, kc] = 200.0
        preds[i1, 64, kc] = preds[i1, 64 + c_hi, kc] = 3.0
        props["contested_anchor"] = kc
        # ---- image i2: an exact metric tie at mirror-image anchors (stride 8, row 3, the two columns around w / 2)
        b = len(rows[i2])
        rows[i2].append(box_gt(w / 2 - 19.875, 18.125, w / 2 + 19.875, 37.875, c_mid))
        k1, k2 = grid_index(w, 0, w // 16 - 1, 3), grid_index(w, 0, w // 16, 3)
        for kk in (k1, k2):                                   # identical logits: one-hot sides l = r = 2, t = b = 1 (exact in
            preds[i2, :64, kk] = 0.0                          # fp32 and float64), so the two boxes mirror each other about w / 2
            for side, b_ in enumerate((2, 1, 2, 1)):
                preds[i2, side * REG + b_, kk] = 200.0
            preds[i2, 64 + c_mid, kk] = 3.0
        props["tie"] = (i2, b, k1, k2)
    for i in live:
        for _ in range(fill):
            rows[i].append(rand_gt(g, w, h, int(torch.randint(0, nc, (1,), generator=g))))
    gts = [torch.tensor(rows[i], dtype=F32).reshape(-1, 5) for i in range(n)]
    case = Case(preds, anchors, strides, gts, nc, dtype, f"N {n} {h}x{w} nc {nc} {str(dtype)[6:]} empty {list(empty)} seed {seed}",
                hyper, grad_scale, capacity)
    case.props = props
    return case


def _assert_built(case):
    p = case.props
    if not p:
        return
    asg, _ = reference(case)
    offs = [0]
    for g in case.gts:
        offs.append(offs[-1] + g.shape[0])
    k = case.hyper["topk"]
    ncand = [int(c.sum()) for c in asg["cand"]]
    i, r = p["many"]
    cand = asg["cand"][offs[i] + r]
    st = case.strides[0].float()
    assert ncand[offs[i] + r] > k and all(bool(cand[st == s].any()) for s in (8.0, 16.0, 32.0))
    for i, r, want in p["few"]:
        assert ncand[offs[i] + r] == want, (ncand[offs[i] + r], want)
    i, r = p["none"]
    assert ncand[offs[i] + r] == 0 and asg["lists"][offs[i] + r] == []
    i, r1, r2 = p["contest"]
    s1, s2 = ({q[0] for q in asg["lists"][offs[i] + r]} for r in (r1, r2))
    assert p["contested_anchor"] in s1 & s2, "the two overlapping GTs do not both choose the anchor built for them"
    assert int(asg["owner"][i, p["contested_anchor"]]) not in (-1, offs[i] + r1)      # r2 has the larger IoU there
    i, r1, r2 = p["twins"]
    assert torch.equal(case.gts[i][r1], case.gts[i][r2]) and asg["lists"][offs[i] + r1] == asg["lists"][offs[i] + r2] != []
    own = asg["owner"][i]
    assert int((own == offs[i] + r2).sum()) == 0 and int((own == offs[i] + r1).sum()) > 0
    i, r, k1, k2 = p["tie"]
    al = asg["align"][offs[i] + r]
    assert k1 < k2 and float(al[k1]) == float(al[k2]) and [q[0] for q in asg["lists"][offs[i] + r][:2]] == [k1, k2][:k]
    p32 = case.preds.float()                                      # the tie is exact in fp32 as well
    pb32 = tr.decode(p32, case.anchors.float(), case.strides.float())
    row = case.gts[i][r]
    _, al32, _ = tr.metrics(pb32[i], p32[i, 64 + int(row[4])], row, case.anchors.float(), case.strides.float(),
                            case.hyper["alpha"], case.hyper["beta"])
    assert float(al32[k1]) == float(al32[k2])


# ------------------------------------------------------------------------------------------------------ the CPU stand-in
def stand_in(case, want_grad=True):
    """the kernel's computation in fp32 torch on the CPU -> State (what tests/test_tal_cpu.py holds the comparator against)"""
    p, an, st = case.f(F32)
    hy = case.hyper
    pbox = tr.decode(p, an, st)
    lists, rows_img, labels = [], [], []
    for n, g in enumerate(case.gts):
        for row in g:
            cls = int(row[4])
            cand, align, iou = tr.metrics(pbox[n], p[n, 64 + cls], row, an, st, hy["alpha"], hy["beta"])
            lists.append([(k, float(align[k]), float(iou[k])) for k in tr.choose(cand, align, hy["topk"])])
            rows_img.append(n), labels.append(cls)
    owner = tr.owners(lists, rows_img, case.N, case.A)
    g_live = len(lists)
    ma, mi, ts = torch.full((g_live,), -1.0), torch.full((g_live,), -1.0), torch.zeros(g_live)
    label, t = torch.full((case.N, case.A), -1, dtype=torch.long), torch.zeros(case.N, case.A)
    label[~torch.isfinite(pbox).all(-1)] = -2
    for j, lst in enumerate(lists):
        n = rows_img[j]
        mine = [q for q in lst if int(owner[n, q[0]]) == j]
        if mine:
            ma[j], mi[j] = max(q[1] for q in mine), max(q[2] for q in mine)
            for k, al, _ in mine:
                t[n, k] = torch.tensor(al) * mi[j] / (ma[j] + tr.EPS9)
                label[n, k] = labels[j]
                ts[j] = ts[j] + t[n, k]
    tss = float(torch.maximum(ts.sum(), torch.tensor(1.0))) if case.tss is None else case.tss
    st_ = State(pbox, lists, owner, label, t, ma, mi, ts, tss, None, None)
    ev = evaluate(case, st_, F32)
    dp = ev["dp"].to(case.dtype) if want_grad else None
    st_.out, st_.dp = ev["out"].float(), dp
    return st_


# ------------------------------------------------------------------------------------------------------ evaluation
def evaluate(case, state, dt=F64):
    """gradients and scalars from the state's pbox, (label, t) and tss in `dt` by the kernel's formulas -> dict(dp, dp_noise
    (N, 64 + nc, A) before the rounding to T, out (4,), out_noise, tss, tss_noise).  float64: the limits (and a second
    evaluation of the values, which the tests compare with autograd); fp32: the CPU stand-in."""
    c = sc.C
    p, an, st = case.f(dt)
    hy, n, a, nc = case.hyper, case.N, case.A, case.nc
    label, t = state.label, state.t.to(dt)
    pos = (label >= 0).nonzero()
    tsum = t.sum() if dt == F64 else state.t.sum()
    tss_v = torch.maximum(tsum, torch.ones((), dtype=tsum.dtype)).to(dt) if case.tss is None else torch.tensor(case.tss, dtype=dt)
    tss_e = c["tal_scalars"] * U * t.abs().sum() if case.tss is None else torch.zeros((), dtype=dt)
    if dt != F64:
        tss_v = torch.tensor(state.tss, dtype=dt)
    gsc = None if case.grad_scale is None else tr.f32_of(case.grad_scale)
    target = torch.zeros(n, nc, a, dtype=dt)
    if pos.numel():
        target[pos[:, 0], label[pos[:, 0], pos[:, 1]], pos[:, 1]] = t[pos[:, 0], pos[:, 1]]
    g_cls, v_cls = dense_chain(p[:, 64:], target, V(tss_v.reshape(1, 1, 1), tss_e.reshape(1, 1, 1)), hy["cls"], gsc)
    dp, dpn = torch.zeros(n, 64 + nc, a, dtype=dt), torch.zeros(n, 64 + nc, a, dtype=dt)
    dp[:, 64:], dpn[:, 64:] = g_cls.v, g_cls.e
    dp[:, 64:][~torch.isfinite(p[:, 64:])] = float("nan")
    dp[:, :64] = torch.where((label == -2)[:, None, :], torch.full_like(dp[:, :64], float("nan")), dp[:, :64])
    cls = vsum(V(v_cls.v.reshape(-1), v_cls.e.reshape(-1)), 0, c["tal_scalars"])
    box = dfl = V(torch.zeros((), dtype=dt))
    if pos.numel():
        pn, pa = pos[:, 0], pos[:, 1]
        rows = case.gt.to(dt)[state.owner[pn, pa]]
        m = pn.numel()
        grad, box_e, dfl_e = positives_chain(p[pn, :64, pa], state.pbox.to(dt)[pn, pa], rows, an[:, pa].t(), st[0, pa], t[pn, pa],
                                             V(tss_v.expand(m), tss_e.expand(m)), hy, gsc)
        dp[pn, :64, pa], dpn[pn, :64, pa] = grad.v, grad.e
        box, dfl = vsum(box_e, 0, c["tal_scalars"]), vsum(dfl_e, 0, c["tal_scalars"])
    tss = V(tss_v, tss_e)
    box, cls, dfl = box / tss, cls / tss, dfl / tss
    total = hy["box"] * box + hy["cls"] * cls + hy["dfl"] * dfl
    return dict(dp=dp, dp_noise=dpn, out=torch.stack([total.v, box.v, cls.v, dfl.v]), out_noise=torch.stack([total.e, box.e, cls.e, dfl.e]),
                tss=tss_v, tss_noise=tss_e, pos=pos)


# ------------------------------------------------------------------------------------------------------ the checks
def _close(got, ref, noise, dtype, what, family):
    try:
        return sc.assert_close(got, ref, noise / U24, dtype, what, family=family, c=1.0)
    except StrictMismatch as ex:
        raise StrictMismatch(f"[tal: c = 1 on M = noise / 2^-24, the noise budget of strict_tal.py at c = "
                             f"{sc.C.get(family, sc.C_DEFAULT):g}]\n{ex}", ex.count, ex.hist, ex.worst) from None


def _observe(fam, share, count):
    o = sc.OBSERVED.setdefault(fam, [float("-inf"), 0, 0])
    o[0], o[1], o[2] = max(o[0], share), o[1] + count, o[2] + 1


def check_topk(case, state):
    """the lists against the float64 metrics of the kernel's pbox"""
    p, an, st = case.f(F64)
    hy = case.hyper
    k = hy["topk"]
    pbox = state.pbox.to(F64)
    gt, img = case.gt.to(F64), case.img
    lines, worst = [], 0.0
    assert len(state.lists) == gt.shape[0], (len(state.lists), gt.shape[0])
    for j in range(gt.shape[0]):
        n, cls = int(img[j]), int(gt[j, 4])
        cand, _, _ = tr.metrics(pbox[n], p[n, 64 + cls], gt[j], an, st, hy["alpha"], hy["beta"])
        al, io = metric_chain(pbox[n].nan_to_num(0.0), gt[j].expand(case.A, 5), p[n, 64 + cls].nan_to_num(0.0), hy["alpha"], hy["beta"])
        lst = state.lists[j]
        chosen = [q[0] for q in lst]
        ci = cand.nonzero().flatten()
        want_n = min(k, int(ci.numel()))
        tag = f"{case.what} row {j} (image {n})"
        if len(set(chosen)) != len(chosen) or any(not (0 <= q < case.A) for q in chosen):
            lines.append(f"{tag}: list {chosen} has repeated or out-of-range anchors")
            continue
        if len(chosen) != want_n or any(not bool(cand[q]) for q in chosen):
            lines.append(f"{tag}: {len(chosen)} chosen, {[q for q in chosen if not bool(cand[q])]} not candidates; want {want_n} of {ci.numel()}")
            continue
        keys = [(-q[1], q[0]) for q in lst]
        if keys != sorted(keys):
            lines.append(f"{tag}: list not sorted by (align descending, anchor): {lst}")
        for q, a32, i32 in lst:
            if abs(a32 - float(al.v[q])) > float(al.e[q]) + 0.5 * float(sc.ulp(al.v[q], F32)) or \
                    abs(i32 - float(io.v[q])) > float(io.e[q]) + 0.5 * float(sc.ulp(io.v[q], F32)):
                lines.append(f"{tag}: stored (align, iou) of anchor {q} = ({a32:.9g}, {i32:.9g}), float64 ({float(al.v[q]):.9g} +- "
                             f"{float(al.e[q]):.3g}, {float(io.v[q]):.9g} +- {float(io.e[q]):.3g})")
        if ci.numel() > k:
            order = torch.sort(al.v[ci], descending=True, stable=True)[1]
            ranked = ci[order]
            kth, nxt = ranked[k - 1], ranked[k]
            mk, ek = float(al.v[kth]), float(al.e[kth])
            cs = set(chosen)
            for q in ci.tolist():
                m, e = float(al.v[q]), float(al.e[q])
                over = (mk - m) if q in cs else (m - mk)
                if over > 0:
                    share = over / max(e + ek, 1e-300)
                    worst = max(worst, share)
                    if share > 1:
                        lines.append(f"{tag}: anchor {q} ({'chosen' if q in cs else 'left out'}) metric {m:.9g}, k-th {mk:.9g}: "
                                     f"{share:.2f} of the margin")
            gap, marg = mk - float(al.v[nxt]), ek + float(al.e[nxt])
            if (gap > marg or gap == 0.0) and cs != set(ranked[:k].tolist()):
                lines.append(f"{tag}: chosen {sorted(cs)} != reference {sorted(ranked[:k].tolist())} although the k-th and the next "
                             f"metric are {'equal' if gap == 0 else 'separated'}")
        elif set(chosen) != set(ci.tolist()):
            lines.append(f"{tag}: chosen {chosen} != all {ci.numel()} candidates")
    _observe("tal_topk", worst, sum(len(q) for q in state.lists))
    if lines:
        raise StrictMismatch(f"[tal_topk, c = 1]: " + "\n  ".join(lines[:32]), len(lines), {}, [])


def check_owner(case, state):
    """the owner word against the lists: the maximum of the stored iou (lower row among equals), and in float64 within the
    margin of the largest float64 iou; the (label, t) words name the owner's class and nothing else is labelled"""
    pbox = state.pbox.to(F64)
    gt, img = case.gt.to(F64), case.img
    bids, lines, worst = {}, [], 0.0
    for j, lst in enumerate(state.lists):
        for q, _, i32 in lst:
            bids.setdefault((int(img[j]), q), []).append((j, i32))
    want = torch.full_like(state.owner, -1)
    for (n, q), bs in bids.items():
        win = sorted(bs, key=lambda b: (-b[1], b[0]))[0][0]
        want[n, q] = win
        if len(bs) > 1:
            rows = torch.tensor([b[0] for b in bs])
            _, io = metric_chain(pbox[n, q].expand(len(bs), 4), gt[rows], torch.zeros(len(bs), dtype=F64), 1.0, 1.0)
            got = int(state.owner[n, q])
            if got in rows.tolist():
                gi = rows.tolist().index(got)
                top = int(io.v.argmax())
                over = float(io.v[top] - io.v[gi])
                if over > 0:
                    share = over / max(float(io.e[top] + io.e[gi]), 1e-300)
                    worst = max(worst, share)
                    if share > 1:
                        lines.append(f"{case.what} image {n} anchor {q}: owner row {got} iou {float(io.v[gi]):.9g}, row {int(rows[top])} "
                                     f"has {float(io.v[top]):.9g}: {share:.2f} of the margin")
    bad = (want != state.owner).nonzero()
    if bad.numel():
        lines.append(f"{case.what}: owner differs from the maximum of the stored iou at (n, a, got, want) " +
                     str([(int(n), int(q), int(state.owner[n, q]), int(want[n, q])) for n, q in bad[:16]]))
    lab = torch.where(want >= 0, gt[:, 4].long()[want.clamp(min=0)] if gt.shape[0] else want, torch.full_like(want, -1))
    poisoned = ~torch.isfinite(state.pbox).all(-1)
    lab = torch.where(poisoned & (want < 0), torch.full_like(lab, -2), lab)
    badl = (lab != state.label).nonzero()
    if badl.numel():
        lines.append(f"{case.what}: label word differs at (n, a, got, want) " +
                     str([(int(n), int(q), int(state.label[n, q]), int(lab[n, q])) for n, q in badl[:16]]))
    _observe("tal_owner", worst, len(bids))
    if lines:
        raise StrictMismatch(f"[tal_owner, c = 1]: " + "\n  ".join(lines[:32]), len(lines), {}, [])


def check_target(case, state):
    """ma, mi, t and the rows' sums of t from the stored lists and owners"""
    g_live = len(state.lists)
    if not g_live:
        return
    img = case.img
    ma, mi = torch.full((g_live,), -1.0, dtype=F64), torch.full((g_live,), -1.0, dtype=F64)
    t_ref, t_noise = torch.zeros(case.N, case.A, dtype=F64), torch.zeros(case.N, case.A, dtype=F64)
    ts, ts_noise = torch.zeros(g_live, dtype=F64), torch.zeros(g_live, dtype=F64)
    for j, lst in enumerate(state.lists):
        n = int(img[j])
        mine = [q for q in lst if int(state.owner[n, q[0]]) == j]
        if not mine:
            continue
        ma[j], mi[j] = max(q[1] for q in mine), max(q[2] for q in mine)
        al = V(torch.tensor([q[1] for q in mine], dtype=F64))
        tv = al * float(mi[j]) / (V(ma[j].expand(len(mine))) + tr.EPS9)
        idx = torch.tensor([q[0] for q in mine])
        t_ref[n, idx], t_noise[n, idx] = tv.v, tv.e
        s = vsum(tv, 0, sc.C["tal_target"])
        ts[j], ts_noise[j] = s.v, s.e + 0.5 * float(sc.ulp(tv.v.max(), F32)) * len(mine)     # the stored t are rounded
    zero = torch.zeros(1, 2, g_live, dtype=F64)
    _close(torch.stack([state.ma, state.mi]).view(1, 2, -1), torch.stack([ma, mi]).view(1, 2, -1), zero, F32, f"{case.what} ma, mi", "tal_target")
    _close(state.t.view(case.N, 1, case.A), t_ref.view(case.N, 1, case.A), t_noise.view(case.N, 1, case.A), F32, f"{case.what} t", "tal_target")
    _close(state.ts.view(1, 1, -1), ts.view(1, 1, -1), ts_noise.view(1, 1, -1), F32, f"{case.what} sum of t per row", "tal_target")


def reference_terms(case, state):
    """tal_ref.terms on the state's pbox, owners, labels and t (float64 autograd)"""
    p, an, st = case.f(F64)
    t = state.t.to(F64)
    tss = case.tss if case.tss is not None else max(float(t.sum()), 1.0)
    label = state.label.clamp(min=-1)
    return tr.terms(p, an, st, case.gt.to(F64), None, state.owner, label, t, case.hyper, pbox_in=state.pbox, grad_scale=case.grad_scale, tss=tss)


def check_values(case, state, families=("tal_dense", "tal_box", "tal_scalars")):
    """gradients and scalars; raises the first family's StrictMismatch after trying every family (`.families`)"""
    ref = reference_terms(case, state)
    ev = evaluate(case, state)
    failed = []
    pos_mask = (state.label >= 0)[:, None, :].expand(case.N, 64, case.A)

    def run(fam, fn):
        if fam not in families:
            return
        try:
            fn()
        except StrictMismatch as ex:
            failed.append((fam, ex))

    def scalars():
        noise = ev["out_noise"]
        _close(state.out.view(1, 4, 1), ref["out"].view(1, 4, 1), noise.view(1, 4, 1), F32, f"{case.what} out", "tal_scalars")
        if case.tss is None:
            _close(torch.tensor([state.tss]).view(1, 1, 1), torch.tensor([ref["tss"]], dtype=F64).view(1, 1, 1),
                   ev["tss_noise"].view(1, 1, 1), F32, f"{case.what} tss", "tal_scalars")

    run("tal_scalars", scalars)
    if state.dp is not None:
        dp = state.dp.detach().cpu()
        assert dp.dtype == case.dtype and tuple(dp.shape) == tuple(ref["dp"].shape), (dp.dtype, dp.shape)
        g64, r, nz = dp.to(F64), ref["dp"], ev["dp_noise"]
        nan_ref = torch.isnan(r)
        assert torch.equal(torch.isnan(g64), nan_ref), \
            f"{case.what}: NaN pattern differs at {(torch.isnan(g64) != nan_ref).nonzero()[:16].tolist()}"
        g64, r = torch.where(nan_ref, torch.zeros_like(g64), g64), torch.where(nan_ref, torch.zeros_like(r), r)
        nz = torch.where(nan_ref, torch.zeros_like(nz), nz)
        box_got, box_ref, box_nz = g64[:, :64], r[:, :64], nz[:, :64]
        dense_got = torch.cat([torch.where(pos_mask, box_ref, box_got), g64[:, 64:]], 1)
        dense_nz = torch.cat([torch.zeros_like(box_nz), nz[:, 64:]], 1)
        run("tal_dense", lambda: _close(dense_got, r, dense_nz, case.dtype, f"{case.what} dpreds", "tal_dense"))
        if bool(pos_mask.any()):
            run("tal_box", lambda: _close(torch.where(pos_mask, box_got, box_ref), box_ref, box_nz, case.dtype,
                                          f"{case.what} dpreds of the positives", "tal_box"))
    if failed:
        ex = failed[0][1]
        ex.families = [f for f, _ in failed]
        raise ex
    return ref, ev


def verify(case, state):
    """every stage on what one launch left behind; raises StrictMismatch naming every family outside its limits"""
    failed = []
    steps = [("loss_decode", lambda: sl.check_decode(case, state.pbox)), ("tal_topk", lambda: check_topk(case, state)),
             ("tal_owner", lambda: check_owner(case, state)), ("tal_target", lambda: check_target(case, state)),
             ("values", lambda: check_values(case, state))]
    finite = bool(torch.isfinite(case.preds.float()[:, :64]).all())
    for fam, fn in steps:
        if fam == "loss_decode" and not finite:
            continue
        try:
            fn()
        except StrictMismatch as ex:
            failed.append((getattr(ex, "families", [fam]), ex))
    if failed:
        ex = failed[0][1]
        fams = [f for fs, _ in failed for f in fs]
        raise StrictMismatch(str(ex) + f"\n[families outside their limits: {fams}]", ex.count, ex.hist, ex.worst)


def failing_families(fn):
    import re
    try:
        fn()
    except StrictMismatch as ex:
        m = re.search(r"\[families outside their limits: \[(.*?)\]\]", str(ex))
        if m:
            return [s.strip(" '") for s in m.group(1).split(",")]
        return getattr(ex, "families", None) or [re.search(r"\[(\w+), c = ", str(ex)).group(1)]
    return []
