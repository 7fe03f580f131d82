"""float64 restatement of YoloTALoss (the kernels are csrc/loss_tal.hip), stage by stage.

Every stage is a function of the buffers that stage receives, so a caller can feed it either the previous stage of this
file (the pure reference: tests/test_tal_cpu.py) or what the kernel itself left behind (tests/strict_tal.py): fp32 and
float64 then never disagree about a discrete choice, and one stage's error cannot hide in another's slack.

    decode(preds, anchors, strides)                          -> pbox (N, A, 4) centre-xywh pixels
    metrics(pbox_n, logit, row, anchors, strides, a, b)      -> candidate mask, align, iou over the image's anchors
    choose(cand, align, topk)                                -> the row's list of anchors, best first
    owners(lists, n_img, A)                                  -> owner row per (n, a), -1: none
    targets(lists, owner)                                    -> per row ma, mi and t per entry; label / t per (n, a)
    terms(...)                                               -> the four scalars, tss and d total / d preds by autograd

The constants are the kernel's fp32 constants (1e-7f, 1e-9f, 15 - 0.01f, 4 / pi^2 as a float), so the two sides evaluate the
same formula and differ by roundings only.  Non-finite inputs follow the definition's item 10 by explicit rules: an anchor
whose decoded box is not finite is never a candidate and gets NaN in its 64 box-logit gradients; a NaN metric is never chosen;
a class logit that is not finite gets a NaN gradient."""
import math

import torch

F32, F64 = torch.float32, torch.float64
REG = 16


def f32_of(x):
    return float(torch.tensor(x, dtype=F32))


EPS7, EPS9 = f32_of(1e-7), f32_of(1e-9)
CLAMP = float(torch.tensor(15.0, dtype=F32) - torch.tensor(0.01, dtype=F32))
KV = f32_of(4.0 / math.pi ** 2)
DEFAULTS = dict(topk=10, alpha=0.5, beta=6.0, box=7.5, cls=0.5, dfl=1.5)


def make_anchors(h, w):
    """anchors (2, A) in grid units and strides (1, A) of an h x w input: levels of stride 8, 16, 32, row-major"""
    ax, ay, st = [], [], []
    for s in (8, 16, 32):
        gh, gw = h // s, w // s
        yy, xx = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
        ax.append(xx.flatten() + 0.5), ay.append(yy.flatten() + 0.5), st.append(torch.full((gh * gw,), float(s)))
    return torch.stack([torch.cat(ax), torch.cat(ay)]).float(), torch.cat(st).view(1, -1).float()


def decode(preds, anchors, strides):
    n, _, a = preds.shape
    x = preds[:, :64].reshape(n, 4, REG, a)
    p = torch.softmax(x, 2)
    e = (p * torch.arange(REG, dtype=preds.dtype).view(1, 1, REG, 1)).sum(2)
    ax, ay, st = anchors[0], anchors[1], strides[0]
    x1, y1, x2, y2 = (ax - e[:, 0]) * st, (ay - e[:, 1]) * st, (ax + e[:, 2]) * st, (ay + e[:, 3]) * st
    return torch.stack([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1], -1)


def corners(pb):
    return pb[..., 0] - pb[..., 2] / 2, pb[..., 1] - pb[..., 3] / 2, pb[..., 0] + pb[..., 2] / 2, pb[..., 1] + pb[..., 3] / 2


def plain_iou(pb, g):
    """the metric's IoU of boxes pb (..., 4) with GT corners g = (gx1, gy1, gx2, gy2)"""
    X1, Y1, X2, Y2 = corners(pb)
    iw = (torch.minimum(X2, g[2]) - torch.maximum(X1, g[0])).clamp(min=0)
    ih = (torch.minimum(Y2, g[3]) - torch.maximum(Y1, g[1])).clamp(min=0)
    inter = iw * ih
    return inter / ((X2 - X1) * (Y2 - Y1) + (g[2] - g[0]) * (g[3] - g[1]) - inter + EPS7)


def inside(row, anchors, strides):
    """min distance of every anchor point to the four sides of GT `row` (5,) -> (A,), > 1e-9 for a candidate"""
    g = corners(row[:4])
    px, py = anchors[0] * strides[0], anchors[1] * strides[0]
    return torch.stack([px - g[0], py - g[1], g[2] - px, g[3] - py]).amin(0)


def metrics(pbox_n, logit, row, anchors, strides, alpha, beta):
    """pbox_n (A, 4), logit (A,): the class logit of the row's label -> (cand (A,) bool, align (A,), iou (A,))"""
    g = corners(row[:4])
    finite = torch.isfinite(pbox_n).all(-1)
    pb = torch.where(finite[:, None], pbox_n, torch.zeros_like(pbox_n))
    iou = plain_iou(pb, g)
    align = torch.sigmoid(logit) ** alpha * iou ** beta
    cand = (inside(row, anchors, strides) > EPS9) & finite & ~torch.isnan(align)
    return cand, align, iou


def choose(cand, align, topk):
    """the `topk` candidates with the largest align, the lower anchor first among equals -> list of anchor indices"""
    idx = cand.nonzero().flatten()
    order = torch.sort(align[idx], descending=True, stable=True)[1]
    return idx[order][:topk].tolist()


def owners(lists, rows_img, n_img, a):
    """lists: per row a list of (anchor, align, iou); rows_img: the image of each row -> owner (n_img, a) long, -1 = none:
    the larger iou wins an anchor, the lower row among equals"""
    owner = torch.full((n_img, a), -1, dtype=torch.long)
    best = torch.full((n_img, a), -1.0, dtype=F64)
    for j, lst in enumerate(lists):
        n = int(rows_img[j])
        for anchor, _, iou in lst:
            if iou > best[n, anchor]:
                best[n, anchor], owner[n, anchor] = iou, j
    return owner


def targets(lists, rows_img, labels, owner):
    """-> ma (G,), mi (G,), t per entry (list of lists, 0 where the entry is not owned), label (N, A) long (-1: none), t (N, A)"""
    n_img, a = owner.shape
    g = len(lists)
    ma, mi = torch.full((g,), -1.0, dtype=F64), torch.full((g,), -1.0, dtype=F64)
    label, tmap = torch.full((n_img, a), -1, dtype=torch.long), torch.zeros(n_img, a, dtype=F64)
    t_lists = []
    for j, lst in enumerate(lists):
        n = int(rows_img[j])
        mine = [(anchor, al, io) for anchor, al, io in lst if int(owner[n, anchor]) == j]
        if mine:
            ma[j], mi[j] = max(al for _, al, _ in mine), max(io for _, _, io in mine)
        ts = []
        for anchor, al, io in lst:
            if int(owner[n, anchor]) == j:
                t = al * float(mi[j]) / (float(ma[j]) + EPS9)
                label[n, anchor], tmap[n, anchor] = int(labels[j]), t
                ts.append(t)
            else:
                ts.append(0.0)
        t_lists.append(ts)
    return ma, mi, t_lists, label, tmap


def assign(preds, pbox, anchors, strides, gts, hyper):
    """every discrete stage from pbox on -> dict(lists, rows_img, labels, owner, ma, mi, t_lists, label, t, cand, align, iou)"""
    n_img, _, a = preds.shape
    lists, rows_img, labels, cands, aligns, ious = [], [], [], [], [], []
    for n, g in enumerate(gts):
        for row in g.to(F64).reshape(-1, 5):
            cls = int(row[4])
            cand, align, iou = metrics(pbox[n], preds[n, 64 + cls], row, anchors, strides, hyper["alpha"], hyper["beta"])
            chosen = choose(cand, align, hyper["topk"])
            lists.append([(k, float(align[k]), float(iou[k])) for k in chosen])
            rows_img.append(n), labels.append(cls), cands.append(cand), aligns.append(align), ious.append(iou)
    owner = owners(lists, rows_img, n_img, a)
    ma, mi, t_lists, label, t = targets(lists, rows_img, labels, owner)
    return dict(lists=lists, rows_img=rows_img, labels=labels, owner=owner, ma=ma, mi=mi, t_lists=t_lists, label=label, t=t,
                cand=cands, align=aligns, iou=ious)


def ciou(pb, g):
    """CIoU of boxes pb (M, 4) with GT corners g (4 tensors (M,)); alpha_v detached"""
    X1, Y1, X2, Y2 = corners(pb)
    w1, h1, w2, h2 = X2 - X1, (Y2 - Y1) + EPS7, g[2] - g[0], (g[3] - g[1]) + EPS7
    iw = (torch.minimum(X2, g[2]) - torch.maximum(X1, g[0])).clamp(min=0)
    ih = (torch.minimum(Y2, g[3]) - torch.maximum(Y1, g[1])).clamp(min=0)
    inter = iw * ih
    iou = inter / (w1 * h1 + w2 * h2 - inter + EPS7)
    cw, ch = torch.maximum(X2, g[2]) - torch.minimum(X1, g[0]), torch.maximum(Y2, g[3]) - torch.minimum(Y1, g[1])
    c2 = cw * cw + ch * ch + EPS7
    rho2 = (((g[0] + g[2]) - (X1 + X2)) ** 2 + ((g[1] + g[3]) - (Y1 + Y2)) ** 2) / 4
    v = KV * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
    av = (v / (v - iou + 1.0 + EPS7)).detach()
    return iou - (rho2 / c2 + v * av)


def bce(x, t):
    return x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))


def terms(preds, anchors, strides, gt, rows_img, owner, label, t, hyper, pbox_in=None, grad_scale=None, tss=None):
    """preds (N, 64 + nc, A), anchors, strides float64; gt (G, 5) float64; owner / label (N, A) long, t (N, A) float64: the
    assignment, detached.  pbox_in: the boxes the CIoU term is evaluated at (the kernel's own); its gradient then goes back
    through the float64 decode.  None: the float64 decode itself.  tss: override (a slice of a larger batch).
    -> dict(out (4,), tss, dp (N, 64 + nc, A) incl. grad_scale, box_e / dfl_e: the per-positive values, pos: (n, a) pairs)"""
    n_img, ch, a = preds.shape
    nc = ch - 64
    x = preds.detach().clone().requires_grad_(True)
    finite_x = torch.isfinite(x.detach())
    xs = torch.where(finite_x, x, torch.zeros_like(x))        # the explicit rules below replace what autograd would smear
    pb64 = decode(xs, anchors, strides)
    pbox = pb64.detach() if pbox_in is None else pbox_in.to(F64)
    bad_box = ~torch.isfinite(decode(x.detach(), anchors, strides)).all(-1) if pbox_in is None else ~torch.isfinite(pbox).all(-1)
    if tss is None:
        tss = max(float(t.sum()), 1.0)
    tgt = torch.zeros(n_img, nc, a, dtype=F64)
    pos = (label >= 0).nonzero()
    if pos.numel():
        tgt[pos[:, 0], label[pos[:, 0], pos[:, 1]], pos[:, 1]] = t[pos[:, 0], pos[:, 1]]
    cls_sum = bce(x[:, 64:], tgt).sum()
    box_e, dfl_e = torch.zeros(0, dtype=F64), torch.zeros(0, dtype=F64)
    total = hyper["cls"] * cls_sum / tss
    box_sum = dfl_sum = torch.zeros((), dtype=F64)
    g_pb = None
    if pos.numel():
        pn, pa = pos[:, 0], pos[:, 1]
        rows = gt[owner[pn, pa]]
        g = corners(rows[:, :4])
        tw = t[pn, pa]
        pb_leaf = pbox[pn, pa].clone().requires_grad_(True)
        box_e = tw * (1.0 - ciou(pb_leaf, g))
        box_sum = box_e.sum()
        g_pb, = torch.autograd.grad(hyper["box"] * box_sum / tss, pb_leaf)
        ax, ay, st = anchors[0][pa], anchors[1][pa], strides[0][pa]
        px, py = ax * st, ay * st
        tv = torch.stack([(px - g[0]) / st, (py - g[1]) / st, (g[2] - px) / st, (g[3] - py) / st], 1).clamp(0.0, CLAMP)
        lo = tv.floor()
        wl, wr = (lo + 1.0) - tv, tv - lo
        logp = torch.log_softmax(xs[pn, :64, pa].view(-1, 4, REG), 2)
        ce = -(wl * logp.gather(2, lo.long()[:, :, None])[:, :, 0] + wr * logp.gather(2, lo.long()[:, :, None] + 1)[:, :, 0])
        dfl_e = tw * ce.mean(1)
        dfl_sum = dfl_e.sum()
        total = total + hyper["dfl"] * dfl_sum / tss
    total.backward(retain_graph=True)
    if g_pb is not None:
        pb64[pn, pa].backward(g_pb)
    dp = x.grad.clone()
    dp[:, 64:][~finite_x[:, 64:]] = float("nan")
    dp[:, :64] = torch.where(bad_box[:, None, :], torch.full_like(dp[:, :64], float("nan")), dp[:, :64])
    if grad_scale is not None:
        dp = dp * f32_of(grad_scale)
    box, cls, dfl = box_sum.detach() / tss, cls_sum.detach() / tss, dfl_sum.detach() / tss
    out = torch.stack([hyper["box"] * box + hyper["cls"] * cls + hyper["dfl"] * dfl, box, cls, dfl])
    return dict(out=out, tss=tss, dp=dp, box_e=box_e.detach(), dfl_e=dfl_e.detach(), pos=pos)


def loss(preds, anchors, strides, gts, hyper=None, grad_scale=None):
    """the whole reference on rounded inputs of any dtype -> (assignment dict, terms dict)"""
    hyper = dict(DEFAULTS, **(hyper or {}))
    p, an, st = preds.to(F64), anchors.to(F64), strides.to(F64)
    pbox = decode(p, an, st)
    asg = assign(p, pbox, an, st, gts, hyper)
    live = [g.reshape(-1, 5).to(F64) for g in gts if g.numel()]
    gt = torch.cat(live) if live else torch.zeros(0, 5, dtype=F64)
    return asg, terms(p, an, st, gt, asg["rows_img"], asg["owner"], asg["label"], asg["t"], hyper, grad_scale=grad_scale)
