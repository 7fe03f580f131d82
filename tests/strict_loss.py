"""Strict per-element comparator for the loss kernels of csrc/loss.hip (k_front, k_assign, k_back): float64 references and
derived limits, on top of strict_compare.py (its ulp(), assert_close, StrictMismatch, OBSERVED / report() and failure
histograms).  Shared by tests/test_strict_loss_cpu.py (the proof of the comparator, no GPU) and tests/test_gpu_loss.py.

Every stage is compared with the float64 evaluation of its formula from exactly the buffers that stage receives: the decode
from the rounded preds / anchors / strides, the assignment from the kernel's own pbox, the gradients and the scalars from
the kernel's own pbox AND idx.  fp32 and float64 then never disagree about a discrete choice, and the error of one stage
cannot hide in the slack of another.

Arithmetic model (the kernel's header): 16-bit or fp32 inputs taken as exact, fp32 arithmetic without contraction, ONE
rounding to T; with grad_scale the multiplication is in fp32 before that rounding (u_T at the scaled magnitude).
Notation: U = 2^-24, one fp32 rounding, relative; u_T(x) = 1/2 ulp_T(x), granted by the comparator itself; c = 16 (sc.C per
family, the rule of strict_compare.py applies) multiplies the SUMMATION terms only; every other term is a first-order
propagation of the roundings of the kernel's formula, carried element by element next to the float64 value (`e_` below).

Transcendental terms (the accurate expf / logf of the device library and IEEE division, not __expf):
    expf(z), logf(z)   2 U relative (one ulp), + the error of the argument: expf amplifies an absolute error d by d,
                       logf an absolute error d by d / z
    sigm(x)            1 / (1 + expf(-x)): 4 U relative (expf 2 U (1 - s), the add, the division; rounded up)
    These are modelled, not taken from a hardware specification: the CPU stand-ins (libm / sleef through torch, <= 1 ulp)
    and the MI355X both stay inside them, see the recorded shares below.

loss_decode   pbox = decode(softmax expectation): per side E = sum_b p_b b with
                  dE = U sum_b p_b b (|x_b - mx| + 6) + c U E
              (x - mx rounds: U |x - mx| into expf; expf 2 U; the division, the product with b, and 2 U for the sum the
              softmax divides by; c: the two 16-term sums), corners (a -+ E) st: st dE + 2 U (|a| + E) st; the centre and
              the width count the two corners' mass once more each (the add / subtract).
loss_assign   (a) idx == torch.cdist(gt_xy, pbox_xy).argmin(1) in fp32 on the CPU, exactly;
              (b) in float64 d^2(chosen) <= min d^2 + margin, margin = the fp32 rounding of |a|^2 + |b|^2 - 2ab at those
              magnitudes on both sides: 2 x 8 U (|a|^2 + |b|^2 + 2 |a.b|) + 2 U d^2 (the square root).
loss_dense    g = -(2 s l1 - s^2 / (1 - s + 1e-12)) s (1 - s) coef [grad_scale], l1 = log(1 - s + 1e-12): qfl_elem() below
              carries s, 1 - s (absolute error 4 U s + U: l1 = -s for small s, and U / s relative is what fp32 gives),
              l1, both terms of dneg and the three products; coef = lambda_cls / N / A is formed in fp32 on the host (3 U),
              one more U with grad_scale.  Every box-logit gradient of an unmatched anchor: reference 0, noise 0 (the
              comparator's limit at 0 is half the smallest subnormal: any other value, NaN included, fails).
loss_box      the 64 box logits of a matched anchor: sum over EVERY GT mapped there of
                  cdfl (p - wl [bin = lo] - wr [bin = lo + 1])  +  gs p (bin - E)
              p, E with the softmax terms above; the target tv through its division by the stride; the IoU chain term by
              term from the kernel's pbox: corners, iwr / ihr (differences of corners: their ABSOLUTE error), inter, den,
              kI, kA, giou (its two log terms cancel: both absolute errors), kI dI and kA dA separately and then their
              difference, dcx / dw / dcy / dh, the four sides.  Summation over the K GTs of the anchor: min(c, 2 K - 1) U
              on the sum of absolute terms.
loss_slot     the class logit at (anchor, cls) of the LAST GT mapped there: qfl_elem(x, iou) with the float64 IoU and its
              propagated error as the target's; t dpos + (1 - t) dneg cancels: mass t |dpos| + (1 - t) |dneg|.
loss_scalars  out[3] = total, mean DFL, mean class loss given idx: c U sum of absolute terms (fp32 per-thread sums, folded
              in double) + the propagated error of every term; u_32 of the three values.

What strict_compare.assert_close receives: c = 1 and mass = noise / U, so its limit IS u_T + noise and the figure recorded
per family is the largest share of the noise budget used, (|got - ref| - u_T) / noise, limit 1.  dpreds goes in as
(N, channels, A): the histogram by image names the image, the one by 16-pixel block the anchor block (n A + a) / 16.  For
loss_dense and loss_slot the class region goes in whole and the elements of the other family are replaced by their
reference (so they count among the elements and can never fail).

Cases: make_case() builds anchors, strides, preds and GT sets so that every property is exact by construction and asserted on
the CPU (collisions, exact distance ties, DFL and IoU edges, empty images); a random draw is rejected and redrawn when a
min/max or clamp operand pair of the IoU is closer than 2^-10 px without being exactly equal (guard_ok).

Recorded maxima, largest share of the noise budget used per family, (|got - ref| - u_T) / noise (limit 1; c = 16 held for
every family, none was raised).
MI355X, tests/test_gpu_loss.py plus the loss tests of tests/test_gpu_kernels.py, 2026-10-19, on the kernels of the commit
that adds this file (csrc/loss.hip of f3a49ae plus the NaN sweep of k_back); 41 comparisons, 15.1 M box and 15.2 M class elements:
    loss_decode 0.229   loss_assign 0.000 (idx exact on every case; the chosen anchor is the float64 minimum everywhere)
    loss_dense 0.248    loss_box 0.664    loss_scalars 0.028
    loss_slot 0.397 (test_loss_random_s640_shape; 0.263 on the built cases of tests/test_gpu_loss.py)
CPU stand-ins (tests/test_strict_loss_cpu.py, STAND_IN_MAXIMA): decode 0.229, assign 0.000, dense 0.246, box 0.684,
slot 0.263, scalars 0.036.
Not measured: the error of expf / logf / the division on their own (the constants above are a model, checked only through
these shares), and the i0 loop of the dense pass wrapping a second time (that needs more than 4 x 2048 x 256 class packets:
17 M class elements in 16 bit; the grid-cap cases reach the cap and the guarded tail, not the second trip)."""

import re

import torch

import strict_compare as sc
from strict_compare import U24, StrictMismatch, ulp  # noqa: F401  (re-exported for the tests)

F32, F64, BF, HF = torch.float32, torch.float64, torch.bfloat16, torch.float16
REG = 16
FAMILIES = ("loss_decode", "loss_assign", "loss_dense", "loss_box", "loss_slot", "loss_scalars")
for _f in FAMILIES:
    sc.C[_f] = sc.C_DEFAULT
    sc.BUDGET_FAMILIES.add(_f)
QEPS = float(torch.tensor(1e-12, dtype=F32))
IOU_EPS = float(torch.tensor(1e-6, dtype=F32))
CLAMP = float(torch.tensor(15.0, dtype=F32) - torch.tensor(0.01, dtype=F32))     # (float)(REG - 1) - 0.01f
GUARD_GAP = 2.0 ** -10
OLD_TOL = {F32: 1e-4, BF: 2.0 ** -6, HF: 2.0 ** -6}     # test_loss_random_s640_shape: share of max |dpreds|
GUARD = True


def f32_of(x):
    return float(torch.tensor(x, dtype=F32))


# ------------------------------------------------------------------------------------------------------ the cases
class Case:
    """preds (N, 64 + nc, A), anchors (2, A), strides (1, A) in `dtype` on the CPU; gts: N tensors (M, 5) fp32"""

    def __init__(self, preds, anchors, strides, gts, nc, dtype, what, lam=(1.5, 1.0), grad_scale=None):
        self.preds, self.anchors, self.strides = preds.to(dtype), anchors.to(dtype), strides.to(dtype)
        self.gts = [g.reshape(-1, 5).to(F32) for g in gts]
        self.nc, self.dtype, self.what, self.lam, self.grad_scale = nc, dtype, what, lam, grad_scale
        self.N, _, self.A = preds.shape
        self.expect_idx = None          # where the construction fixes the assignment: list of (row, anchor)
        self.props, self.pairs = {}, []
        self.n_mean = None              # the image count of the means, where the case is a slice of a larger batch

    @property
    def gt(self):
        live = [g for g in self.gts if g.shape[0]]
        return torch.cat(live) if live else torch.zeros(0, 5)

    @property
    def img(self):
        return torch.tensor([i for i, g in enumerate(self.gts) for _ in range(g.shape[0])], dtype=torch.long)

    def with_(self, dtype=None, grad_scale="same"):
        c = Case(self.preds.float(), self.anchors.float(), self.strides.float(), self.gts, self.nc, dtype or self.dtype,
                 self.what, self.lam, self.grad_scale if grad_scale == "same" else grad_scale)
        c.expect_idx, c.props, c.pairs = self.expect_idx, self.props, self.pairs
        return c


def make_grid(a):
    """anchors (2, A), strides (1, A): a 32-wide stride-8 level, then a 16-wide stride-16 level; every value exact in bf16"""
    a1 = 64 if a < 128 else (a * 3 // 4) // 32 * 32
    i1, i2 = torch.arange(a1), torch.arange(a - a1)
    ax = torch.cat([(i1 % 32) + 0.5, (i2 % 16) + 0.5])
    ay = torch.cat([(i1 // 32) + 0.5, (i2 // 16) + 0.5])
    st = torch.cat([torch.full((a1,), 8.0), torch.full((a - a1,), 16.0)])
    return torch.stack([ax, ay]).float(), st.view(1, -1).float()


ZERO_BLOCK = list(range(16, 25)) + list(range(48, 57))        # all-zero box logits: centre = anchor * stride, w = h = 15 st
TWO_HOT = (20, 22)                                            # l one-hot at bin 0; t, r, b two-hot at bins 0, 1: E = 0, .5, .5, .5
TIE_ANCHOR, INT_ANCHOR = 18, 50


def tie_pairs(a):
    """(i, j), i < j: anchor j becomes a bit-identical copy of anchor i"""
    p = [(10, 27)]                                            # different lanes (at A = 84 both in the tail loop)
    if a >= 512:
        p += [(5, 69)]                                        # the same lane, unrolled slots 0 and 1
    if a == 724:
        p += [(100, 600), (520, 650)]                         # the unrolled part against the tail; both in the tail
    if a in (1030, 1032):
        p += [(300, 1027), (1025, 1029)]
    return p


def decode64(case, dt=F64):
    """-> pbox (N, A, 4) centre-xywh and its noise, from the rounded inputs"""
    x = case.preds[:, :64].to(dt).view(case.N, 4, REG, case.A)
    mx = x.amax(2, keepdim=True)
    d = x - mx
    ex = torch.exp(d)
    p = ex / ex.sum(2, keepdim=True)
    bins = torch.arange(REG, dtype=dt).view(1, 1, REG, 1)
    e = torch.zeros_like(p[:, :, 0])
    for b in range(REG):                                      # the kernel's order: bin after bin
        e = e + p[:, :, b] * float(b)
    de = U24 * (p * bins * (d.abs() + 6.0)).sum(2) + sc.C["loss_decode"] * U24 * e
    ax, ay, st = case.anchors[0].to(dt), case.anchors[1].to(dt), case.strides[0].to(dt)
    x1, y1, x2, y2 = (ax - e[:, 0]) * st, (ay - e[:, 1]) * st, (ax + e[:, 2]) * st, (ay + e[:, 3]) * st
    m = [(a_.abs() + e[:, s]) * st for s, a_ in enumerate((ax, ay, ax, ay))]
    dc = [st * de[:, s] + 2.0 * U24 * m[s] for s in range(4)]
    pbox = torch.stack([(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1], 2)
    nx, ny = dc[0] + dc[2] + U24 * (m[0] + m[2]), dc[1] + dc[3] + U24 * (m[1] + m[3])
    return pbox, torch.stack([nx / 2, ny / 2, nx, ny], 2)


def assign_cpu(case, pbox):
    """torch.cdist(...).argmin(1) in fp32 on the CPU, image by image -> (G,) long"""
    out = []
    for n, g in enumerate(case.gts):
        if g.shape[0]:
            out.append(torch.cdist(g[:, :2].float(), pbox[n, :, :2].float()).argmin(1))
    return torch.cat(out) if out else torch.zeros(0, dtype=torch.long)


def _corners(pb, g, textbook=False):
    x1, x2, y1 = pb[:, 0] - pb[:, 2] / 2, pb[:, 0] + pb[:, 2] / 2, pb[:, 1] - pb[:, 3] / 2
    y2 = pb[:, 1] + pb[:, 3] / 2 if textbook else pb[:, 3] + pb[:, 1] / 2
    return (x1, y1, x2, y2), (g[:, 0] - g[:, 2] / 2, g[:, 1] - g[:, 3] / 2, g[:, 0] + g[:, 2] / 2, g[:, 1] + g[:, 3] / 2)


def guard_ok(case, idx=None, pbox=None):
    """no min/max or clamp operand pair of any (GT, its anchor) closer than 2^-10 px unless exactly equal"""
    if pbox is None:
        pbox = decode64(case)[0]
    if idx is None:
        idx = assign_cpu(case, pbox)
    if not idx.numel():
        return True
    (x1, y1, x2, y2), (gx1, gy1, gx2, gy2) = _corners(pbox[case.img, idx].to(F64), case.gt.to(F64))
    iwr, ihr = torch.minimum(x2, gx2) - torch.maximum(x1, gx1), torch.minimum(y2, gy2) - torch.maximum(y1, gy1)
    diffs = torch.stack([x2 - gx2, x1 - gx1, y2 - gy2, y1 - gy1, iwr, ihr])
    return not bool(((diffs.abs() < GUARD_GAP) & (diffs != 0)).any())


def _rand_gt(g, cx, cy, cls):
    w, h = torch.rand(2, generator=g) * 120 + 8
    return [float(cx), float(cy), float(w), float(h), float(cls)]


def make_case(n, a, nc, dtype, empty=(), seed=0, grad_scale=None, built=True, crowd=70):
    """the built target sets of tests/test_gpu_loss.py around a random fill; every property asserted here, on the CPU"""
    for attempt in range(50):
        case = _make_case(n, a, nc, dtype, tuple(empty), seed + 1000 * attempt, grad_scale, built, crowd)
        if case is not None:
            return case
    raise RuntimeError("no case without near-ties found")


def _make_case(n, a, nc, dtype, empty, seed, grad_scale, built, crowd):
    g = torch.Generator().manual_seed(7000 + seed)
    anchors, strides = make_grid(a)
    preds = torch.randn(n, 64 + nc, a, generator=g)
    preds[:, 64:] = preds[:, 64:] * 0.7 - 3.5
    pairs = tie_pairs(a) if built else []
    if built:
        preds[:, :64, ZERO_BLOCK] = 0.0
        for e in TWO_HOT:
            preds[:, 0, e] = 200.0                             # left: one-hot at bin 0, E = 0
            for s in (1, 2, 3):
                preds[:, s * REG:s * REG + 2, e] = 200.0       # two-hot: E = 0.5 exactly, in fp32 and in float64
        for i, j in pairs:
            anchors[:, j], strides[:, j] = anchors[:, i], strides[:, i]
            preds[:, :64, j] = preds[:, :64, i]
    preds = preds.to(dtype).float()
    case = Case(preds, anchors, strides, [torch.zeros(0, 5)] * n, nc, dtype,
                f"N {n} A {a} nc {nc} {str(dtype)[6:]} empty {list(empty)} seed {seed}", grad_scale=grad_scale)
    live = [i for i in range(n) if i not in empty]
    if not live:
        case.props = {"all_empty": True}
        return case
    pbox = decode64(case)[0]
    rows = {i: [] for i in live}
    expect = {i: [] for i in live}                            # (row within the image, anchor)
    used = set(ZERO_BLOCK) | {k for p in pairs for k in p}
    cls_cycle = [0, nc - 1, nc // 2, min(1, nc - 1)]
    props = {}

    def iso(img, k):                                          # no other predicted centre within 2 px of anchor k's
        d = (pbox[img, :, :2] - pbox[img, k, :2]).norm(dim=1)
        return int((d <= 2.0).sum()) == 1

    def free_anchor(img, cond=lambda k: True):
        for _ in range(10000):
            k = int(torch.randint(0, a, (1,), generator=g))
            if k not in used and iso(img, k) and cond(k):
                used.add(k)
                return k
        raise RuntimeError("no anchor")

    def add(img, row, anchor):
        rows[img].append(row)
        expect[img].append((len(rows[img]) - 1, anchor))

    def near(img, k, cls, w=None):
        off = torch.rand(2, generator=g) * 1.0 - 0.5
        r = _rand_gt(g, pbox[img, k, 0] + off[0], pbox[img, k, 1] + off[1], cls)
        if w is not None:
            r[2] = w
        add(img, r, k)

    i0, i1, i2 = live[0], live[len(live) // 2], live[-1]
    if built:
        # ---- collisions (image i0): different classes, the same class, three at once, a pair five rows apart
        k_far = free_anchor(i0)
        near(i0, k_far, cls_cycle[0])                          # row 0; its partner comes after the others
        k = free_anchor(i0)
        near(i0, k, 0), near(i0, k, nc - 1)
        k = free_anchor(i0)
        near(i0, k, nc // 2), near(i0, k, nc // 2)
        k = free_anchor(i0)
        near(i0, k, 0), near(i0, k, min(1, nc - 1)), near(i0, k, nc - 1)
        near(i0, k_far, cls_cycle[1])                          # row 8: more than four rows after row 0
        props["collisions"] = (2 if nc > 1 else 0, 2 if nc > 1 else 4, 1)
        # ---- exact distance ties (image i1): the lower index, for every GT aimed at the pair
        for q, (i, j) in enumerate(pairs):
            for r in range(2):
                off = torch.tensor([0.25, -0.5]) * (r + 1)
                add(i1, _rand_gt(g, pbox[i1, i, 0] + off[0], pbox[i1, i, 1] + off[1], cls_cycle[(q + r) % 4]), i)
        # ---- IoU edges (image i1): both x corners tie; touching in x; disjoint in x
        c18 = pbox[i1, TIE_ANCHOR]
        add(i1, [float(c18[0]), float(c18[1]) + 0.375, float(c18[2]), 50.0, 0.0], TIE_ANCHOR)
        e, e2 = TWO_HOT
        add(i1, [float(pbox[i1, e, 0]) + 2.25, 4.0, 0.5, 6.0, float(nc - 1)], e)        # gx1 == X2: iwr = 0
        add(i1, [float(pbox[i1, e2, 0]) + 2.5, 4.0, 0.5, 6.0, 0.0], e2)                  # gx1 = X2 + 0.25: iwr < 0
        # ---- DFL edges (image i2): a target below 0, one above 14.99, an exact integer, classes 0 and nc - 1
        st, anc = case.strides[0].double(), case.anchors.double()
        k = free_anchor(i2, lambda k: float(pbox[i2, k, 0] - anc[0, k] * st[k]) > 1.0)
        near(i2, k, 0, w=0.5)                                  # its left edge is right of the anchor point: tl < 0
        props["below0"] = (i2, len(rows[i2]) - 1)
        k = free_anchor(i2)
        near(i2, k, nc - 1, w=2 * 24.0 * float(st[k]))         # tr, tl above 16 > 14.99
        props["above"] = (i2, len(rows[i2]) - 1)
        c50 = pbox[i2, INT_ANCHOR]
        add(i2, [float(c50[0]) + 0.5, float(c50[1]) + 0.25, 17.0, 30.0, float(nc - 1)], INT_ANCHOR)    # gx1 = 140: tl = 1 exactly
        props["integer"] = (i2, len(rows[i2]) - 1)
    # ---- random fill: distinct anchors, and in image i0 enough to pass 64 GTs
    for i in live:
        want = crowd if (i == i0 and built) else 3 + int(torch.randint(0, 6, (1,), generator=g))
        want = min(want, a // 4 + len(rows[i]))
        while len(rows[i]) < want:
            near(i, free_anchor(i), int(torch.randint(0, nc, (1,), generator=g)))
    case.gts = [torch.tensor(rows[i], dtype=F32).reshape(-1, 5) if i in rows and rows[i] else torch.zeros(0, 5) for i in range(n)]
    case.props = props
    case.pairs = pairs
    # ---- the construction's own properties, checked in float64
    offs, tot = {}, 0
    for i in range(n):
        offs[i] = tot
        tot += case.gts[i].shape[0]
    case.expect_idx = [(offs[i] + r, k) for i in live for r, k in expect[i]]
    for i in live:
        gt = case.gts[i].double()
        d = torch.cdist(gt[:, :2], pbox[i, :, :2])
        for r, k in expect[i]:
            row = d[r].clone()
            twins = [k] + [j for p, j in pairs if p == k] + [p for p, j in pairs if j == k]
            best = float(row[k])
            row[twins] = float("inf")
            if not (float(row.min()) - best > 1e-2):           # another predicted centre is as near: redraw
                return None
    if not guard_ok(case, pbox=pbox):
        return None
    if built:
        _assert_built(case, pbox, offs, pairs)
    return case


def _assert_built(case, pbox, offs, pairs):
    idx = torch.empty(len(case.expect_idx), dtype=torch.long)
    for r, k in case.expect_idx:
        idx[r] = k
    gt, img, p = case.gt.double(), case.img, case.props
    (x1, y1, x2, y2), (gx1, gy1, gx2, gy2) = _corners(pbox[img, idx], gt)
    iwr = torch.minimum(x2, gx2) - torch.maximum(x1, gx1)
    by_anchor = {}
    for r in range(len(idx)):
        by_anchor.setdefault((int(img[r]), int(idx[r])), []).append(r)
    groups = [v for v in by_anchor.values() if len(v) > 1 and not any(int(idx[v[0]]) == i for i, _ in pairs)
              and int(idx[v[0]]) not in ZERO_BLOCK]
    assert sorted(len(v) for v in groups) == [2, 2, 2, 3], groups
    assert any(v[-1] - v[0] > 4 for v in groups) and (case.A < 512 or max(g.shape[0] for g in case.gts) > 64)
    for i, j in pairs:
        assert torch.equal(case.preds[:, :64, i], case.preds[:, :64, j]) and torch.equal(case.anchors[:, i], case.anchors[:, j])
    zb = pbox[:, [k for k in ZERO_BLOCK if k not in TWO_HOT]]
    anc, st = case.anchors.double(), case.strides[0].double()
    zi = [k for k in ZERO_BLOCK if k not in TWO_HOT]
    assert torch.equal(zb[..., 0], (anc[0, zi] * st[zi]).expand_as(zb[..., 0])) and torch.equal(zb[..., 2], (15 * st[zi]).expand_as(zb[..., 2]))
    rows = {int(idx[r]): r for r in range(len(idx)) if int(idx[r]) in (TIE_ANCHOR,) + TWO_HOT}
    r = rows[TIE_ANCHOR]
    assert x1[r] == gx1[r] and x2[r] == gx2[r]
    assert iwr[rows[TWO_HOT[0]]] == 0 and iwr[rows[TWO_HOT[1]]] < 0
    tl = anc[0, idx] - gx1 / st[idx]
    tr = gx2 / st[idx] - anc[0, idx]
    b0, ab, it = (offs[p[k][0]] + p[k][1] for k in ("below0", "above", "integer"))
    assert tl[b0] < 0 and tr[ab] > 15 and tl[it] == 1.0
    cls = gt[:, 4]
    assert bool((cls == 0).any()) and bool((cls == case.nc - 1).any())


# --------------------------------------------------------------------------------------- the float64 restatement
def qfl_elem(x, t, et):
    """quality-focal element with target t (absolute error et): value, d / d logit, d value / d t, and the propagated errors
    -> (val, e_val, dx, e_dx, dval_dt).  Written in the kernel's order (qfl_elem of csrc/loss.hip); any float dtype."""
    u = U24
    s = 1.0 / (1.0 + torch.exp(-x))
    es = 4.0 * u * s
    om = 1.0 - s
    eom = es + u * om
    a1 = om + QEPS
    ea1 = eom + u * a1
    l1 = torch.log(a1)
    el1 = ea1 / a1 + 2.0 * u * l1.abs()
    a0 = s + QEPS
    ea0 = es + u * a0
    ls = torch.log(a0)
    els = ea0 / a0 + 2.0 * u * ls.abs()
    pos, neg = om * om * ls, s * s * l1
    e_pos = 2.0 * om * eom * ls.abs() + om * om * els + 2.0 * u * pos.abs()
    e_neg = 2.0 * s * es * l1.abs() + s * s * el1 + 2.0 * u * neg.abs()
    val = -(t * pos + (1.0 - t) * neg)
    e_val = et * (pos.abs() + neg.abs()) + t * e_pos + (1.0 - t) * e_neg + 3.0 * u * (t * pos.abs() + (1.0 - t) * neg.abs())
    dpos = -2.0 * om * ls + om * om / a0
    e_dpos = 2.0 * (eom * ls.abs() + om * els) + 2.0 * om * eom / a0 + om * om * ea0 / (a0 * a0) + 5.0 * u * dpos.abs()
    dneg = 2.0 * s * l1 - s * s / a1
    e_dneg = 2.0 * (es * l1.abs() + s * el1) + 2.0 * s * es / a1 + s * s * ea1 / (a1 * a1) + 5.0 * u * dneg.abs()
    inner = t * dpos + (1.0 - t) * dneg
    e_in = et * (dpos.abs() + dneg.abs()) + t * e_dpos + (1.0 - t) * e_dneg + 3.0 * u * (t * dpos.abs() + (1.0 - t) * dneg.abs())
    dx = -inner * s * om
    e_dx = e_in * s * om + inner.abs() * (es * om + s * eom) + 2.0 * u * dx.abs()
    return val, e_val, dx, e_dx, -(pos - neg)


MUTANTS_EVAL = ("iou_detached", "loser_without_iou_gradient", "first_gt_wins_the_slot", "textbook_iou", "dfl_by_distinct_anchors",
                "empty_image_left_out", "clamp_at_15", "tie_gradient_to_one_operand", "slot_with_target_0", "dense_zeroed")


def evaluate(case, idx, pbox, dt=F64, mut=None):
    """the loss given the assignment `idx` (G,) and the predicted boxes `pbox` (N, A, 4): every formula of k_front's dense
    half and of k_back, GT by GT, in the kernel's operation order, in `dt` (float64: the reference; float32: stand-in (ii)).
    -> dict: dp, dp_noise (N, 64 + nc, A; WITHOUT the rounding to T, with grad_scale), slot / matched masks, out (3,), out_noise"""
    assert mut is None or mut in MUTANTS_EVAL, mut
    u, c = U24, sc.C
    n, a, nc = case.N, case.A, case.nc
    lam_dfl, lam_cls = f32_of(case.lam[0]), f32_of(case.lam[1])
    gsc = 1.0 if case.grad_scale is None else f32_of(case.grad_scale)
    n_eff = case.n_mean or n
    if mut == "empty_image_left_out":
        n_eff = max(1, sum(1 for g in case.gts if g.shape[0]))
    x_all = case.preds.to(dt)
    zero = torch.zeros((), dtype=dt)
    # ---- the dense class pass: target 0
    ccls = lam_cls / n_eff / a
    xc = x_all[:, 64:]
    v0, e_v0, dx0, e_dx0, _ = qfl_elem(xc, zero, zero)
    coefg = ccls * gsc
    g_cls = dx0 * coefg
    n_cls = e_dx0 * coefg + (4.0 + (1.0 if case.grad_scale is not None else 0.0)) * u * g_cls.abs()
    if mut == "dense_zeroed":
        g_cls = torch.zeros_like(g_cls)
    dp = torch.zeros(n, 64 + nc, a, dtype=dt)
    dpn = torch.zeros_like(dp)
    dp[:, 64:], dpn[:, 64:] = g_cls, n_cls
    slot = torch.zeros(n, nc, a, dtype=torch.bool)
    matched = torch.zeros(n, a, dtype=torch.bool)
    cls_sum, cls_noise = v0.sum(dtype=F64 if dt == F64 else dt), c["loss_scalars"] * u * v0.abs().sum() + e_v0.sum()
    dfl_img = torch.zeros(n, dtype=dt)
    dfl_noise = torch.zeros(n, dtype=dt)
    G = int(idx.numel())
    if G:
        gt, img = case.gt.to(dt), case.img
        idx = idx.long()
        m_img = torch.tensor([g.shape[0] for g in case.gts], dtype=dt)[img]
        key = img * a + idx
        order = {}
        first, last, count = torch.zeros(G, dtype=torch.bool), torch.zeros(G, dtype=torch.bool), {}
        for r, k in enumerate(key.tolist()):
            if k not in order:
                first[r] = True
            order[k] = r
            count[k] = count.get(k, 0) + 1
        for k, r in order.items():
            last[r] = True
        winner = first if mut == "first_gt_wins_the_slot" else last
        kcount = torch.tensor([count[k] for k in key.tolist()], dtype=dt)
        # ---- softmax of the 4 x 16 box logits of each GT's anchor
        x = x_all[img, :64, idx].view(G, 4, REG)
        mx = x.amax(2, keepdim=True)
        d = x - mx
        ex = torch.exp(d)
        ssum = ex.sum(2, keepdim=True)
        p = ex / ssum
        rel_sum = u * ((p * (d.abs() + 2.0)).sum(2, keepdim=True) + 4.0)
        e_p = p * (u * (d.abs() + 3.0) + rel_sum)
        lse = mx + torch.log(ssum)
        e_lse = rel_sum + 2.0 * u * torch.log(ssum).abs() + u * lse.abs()
        bins = torch.arange(REG, dtype=dt).view(1, 1, REG)
        ev = (p * bins).sum(2, keepdim=True)
        e_ev = (e_p * bins).sum(2, keepdim=True) + 5.0 * u * ev
        ax, ay, st = case.anchors[0].to(dt)[idx], case.anchors[1].to(dt)[idx], case.strides[0].to(dt)[idx]
        pb = pbox.to(dt)[img, idx]
        (X1, Y1, X2, Y2), (gx1, gy1, gx2, gy2) = _corners(pb, gt, textbook=(mut == "textbook_iou"))
        eX1, eY1, eX2, eY2 = (u * v.abs() for v in (X1, Y1, X2, Y2))
        eg = [u * v.abs() for v in (gx1, gy1, gx2, gy2)]
        # ---- DFL
        q = torch.stack([gx1 / st, gy1 / st, gx2 / st, gy2 / st], 1)
        e_q = torch.stack(eg, 1) / st[:, None] + u * q.abs()
        anc4 = torch.stack([ax, ay, ax, ay], 1)
        sign = torch.tensor([1.0, 1.0, -1.0, -1.0], dtype=dt)
        t = (anc4 - q) * sign
        e_t = e_q + u * t.abs()
        tv = t.clamp(0.0, 15.0 if mut == "clamp_at_15" else CLAMP)
        lo = tv.floor()
        wl, wr = (lo + 1.0) - tv, tv - lo
        oh_lo, oh_hi = (bins == lo[:, :, None]).to(dt), (bins == (lo[:, :, None] + 1.0)).to(dt)
        lx = lse - x
        e_lx = e_lse + u * lx.abs()
        terms = oh_lo * wl[:, :, None] * lx + oh_hi * wr[:, :, None] * lx
        e_terms = (oh_lo + oh_hi) * (e_t[:, :, None] * lx.abs() + e_lx) + u * terms.abs()
        dfl_gt = terms.sum((1, 2)) * 0.25 / m_img
        e_dfl_gt = (e_terms.sum((1, 2)) + 8.0 * u * terms.abs().sum((1, 2))) * 0.25 / m_img
        m_dfl = m_img
        if mut == "dfl_by_distinct_anchors":
            distinct = torch.zeros(n, dtype=dt).index_add_(0, img, first.to(dt))
            m_dfl = distinct[img]
            dfl_gt = dfl_gt * m_img / m_dfl
        dfl_img = dfl_img.index_add(0, img, dfl_gt)
        dfl_noise = dfl_noise.index_add(0, img, e_dfl_gt + c["loss_scalars"] * u * dfl_gt.abs())
        cdfl = (lam_dfl / n_eff * 0.25 / m_dfl)[:, None, None]
        body = p - oh_lo * wl[:, :, None] - oh_hi * wr[:, :, None]
        mass_d = cdfl * (p + oh_lo * wl[:, :, None] + oh_hi * wr[:, :, None])
        g_dfl = cdfl * body
        e_dfl = cdfl * (e_p + e_t[:, :, None]) + 6.0 * u * mass_d
        # ---- the IoU chain
        iwr, ihr = torch.minimum(X2, gx2) - torch.maximum(X1, gx1), torch.minimum(Y2, gy2) - torch.maximum(Y1, gy1)
        e_iwr = torch.maximum(eX2, eg[2]) + torch.maximum(eX1, eg[0]) + u * iwr.abs()
        e_ihr = torch.maximum(eY2, eg[3]) + torch.maximum(eY1, eg[1]) + u * ihr.abs()
        pw, ph = (iwr >= 0).to(dt), (ihr >= 0).to(dt)
        iw, ih = iwr.clamp(min=0.0), ihr.clamp(min=0.0)
        e_iw, e_ih = e_iwr * pw, e_ihr * ph
        inter = iw * ih
        e_inter = e_iw * ih + iw * e_ih + u * inter
        wP, hP = X2 - X1, Y2 - Y1
        e_wP, e_hP = eX2 + eX1 + u * wP.abs(), eY2 + eY1 + u * hP.abs()
        a1 = wP * hP
        e_a1 = e_wP * hP.abs() + wP.abs() * e_hP + u * a1.abs()
        wG, hG = gx2 - gx1, gy2 - gy1
        a2 = wG * hG
        e_a2 = (eg[2] + eg[0] + u * wG.abs()) * hG.abs() + wG.abs() * (eg[3] + eg[1] + u * hG.abs()) + u * a2.abs()
        den = a1 + a2 - inter + IOU_EPS
        e_den = e_a1 + e_a2 + e_inter + 3.0 * u * (a1.abs() + a2.abs() + inter)
        iou = inter / den
        e_iou = e_inter / den.abs() + inter * e_den / (den * den) + u * iou.abs()
        kA = inter / (den * den)
        e_kA = e_inter / (den * den) + kA * (2.0 * e_den / den.abs() + 2.0 * u)
        kI = 1.0 / den + kA
        e_kI = e_den / (den * den) + u / den.abs() + e_kA + u * kI.abs()
        cls = gt[:, 4].long()
        xg = x_all[img, 64 + cls, idx]
        _, _, _, _, dv_dt = qfl_elem(xg, zero, zero)
        # d value / d target = -(om^2 ls - s^2 l1): both terms' absolute errors (they cancel)
        s_ = 1.0 / (1.0 + torch.exp(-xg))
        om_ = 1.0 - s_
        l1_, ls_ = torch.log(om_ + QEPS), torch.log(s_ + QEPS)
        e_t1 = (om_ * om_ * ls_).abs() * 12.0 * u + om_ * om_ * (6.0 * u + 2.0 * u * ls_.abs()) + 2.0 * om_ * (4.0 * u * s_ + u) * ls_.abs()
        e_t2 = (s_ * s_ * l1_).abs() * 12.0 * u + s_ * s_ * ((4.0 * u * s_ + 2.0 * u) / (om_ + QEPS) + 2.0 * u * l1_.abs())
        giou = ccls * dv_dt
        e_giou = ccls * (e_t1 + e_t2 + u * dv_dt.abs()) + 3.0 * u * giou.abs()
        if mut == "iou_detached":
            giou = giou * 0.0
        if mut == "loser_without_iou_gradient":
            giou = giou * last.to(dt)

        def half(a_, b_):                                      # d min(a, b) / d a: a tie splits evenly
            if mut == "tie_gradient_to_one_operand":
                return (a_ <= b_).to(dt)
            return (a_ < b_).to(dt) + 0.5 * (a_ == b_).to(dt)
        mX2, mX1, mY2, mY1 = half(X2, gx2), half(-X1, -gx1), half(Y2, gy2), half(-Y1, -gy1)
        dI = [-ih * pw * mX1, -iw * ph * mY1, ih * pw * mX2, iw * ph * mY2]           # X1, Y1, X2, Y2
        e_dI = [e_ih * pw * mX1, e_iw * ph * mY1, e_ih * pw * mX2, e_iw * ph * mY2]
        dA = [-hP, -wP, hP, wP]
        e_dA = [e_hP, e_wP, e_hP, e_wP]
        dC, e_dC = [], []
        for k_ in range(4):
            t1, t2 = kI * dI[k_], kA * dA[k_]
            e1 = e_kI * dI[k_].abs() + kI.abs() * e_dI[k_] + u * t1.abs()
            e2 = e_kA * dA[k_].abs() + kA.abs() * e_dA[k_] + u * t2.abs()
            diff = t1 - t2
            v = giou * diff
            dC.append(v)
            e_dC.append(e_giou * diff.abs() + giou.abs() * (e1 + e2 + u * diff.abs()) + u * v.abs())
        dX1, dY1, dX2, dY2 = dC
        eX1_, eY1_, eX2_, eY2_ = e_dC
        dcx, dw = dX1 + dX2, (dX2 - dX1) / 2.0
        e_dcx, e_dw = eX1_ + eX2_ + u * dcx.abs(), (eX1_ + eX2_) / 2.0 + u * dw.abs()
        if mut == "textbook_iou":
            dcy, dh = dY1 + dY2, (dY2 - dY1) / 2.0
            e_dcy, e_dh = eY1_ + eY2_ + u * dcy.abs(), (eY1_ + eY2_) / 2.0 + u * dh.abs()
        else:
            dcy, dh = dY1 + dY2 / 2.0, dY2 - dY1 / 2.0
            e_dcy, e_dh = eY1_ + eY2_ / 2.0 + u * dcy.abs(), eY2_ + eY1_ / 2.0 + u * dh.abs()
        d4 = torch.stack([dcx / 2.0 - dw, dcy / 2.0 - dh, dcx / 2.0 + dw, dcy / 2.0 + dh], 1)      # x1, y1, x2, y2
        e_d4 = torch.stack([e_dcx / 2.0 + e_dw, e_dcy / 2.0 + e_dh, e_dcx / 2.0 + e_dw, e_dcy / 2.0 + e_dh], 1) + u * d4.abs()
        gs = d4 * st[:, None] * torch.tensor([-1.0, -1.0, 1.0, 1.0], dtype=dt)
        e_gs = (e_d4 * st[:, None] + u * gs.abs())[:, :, None]
        gs = gs[:, :, None]
        be = bins - ev
        g_iou = gs * p * be
        e_iou_g = e_gs * p * be.abs() + gs.abs() * (e_p * be.abs() + p * (e_ev + u * be.abs())) + 2.0 * u * g_iou.abs()
        # ---- sum over every GT of the anchor, in row order (the kernel: DFL term, then IoU term, GT after GT)
        flat = torch.zeros(n * a, 64, dtype=dt)
        fe, fm = torch.zeros_like(flat), torch.zeros_like(flat)
        for r in range(G):                                     # the per-GT loop: a deterministic order in every dtype
            k = int(key[r])
            flat[k] = (flat[k] + g_dfl[r].reshape(64)) + g_iou[r].reshape(64)
            fe[k] += (e_dfl[r] + e_iou_g[r]).reshape(64)
            fm[k] += (mass_d[r] + g_iou[r].abs()).reshape(64)
        kc = torch.zeros(n * a, dtype=dt)
        kc[key] = kcount
        cmul = torch.minimum(torch.full_like(kc, c["loss_box"]), (2.0 * kc - 1.0).clamp_min(0.0))[:, None]
        box = flat * gsc
        box_n = (fe + cmul * u * fm) * gsc + (u * box.abs() if case.grad_scale is not None else 0.0)
        dp[:, :64] = box.view(n, a, 64).transpose(1, 2)
        dpn[:, :64] = box_n.view(n, a, 64).transpose(1, 2)
        matched.view(-1)[key] = True
        # ---- the slot: the class logit of the GT that owns it
        w = winner.nonzero().flatten()
        t_w, et_w = iou[w], e_iou[w]
        if mut == "slot_with_target_0":
            t_w, et_w = t_w * 0.0, et_w * 0.0
        v1, e_v1, dx1_, e_dx1, _ = qfl_elem(xg[w], t_w, et_w)
        v0w, e_v0w, _, _, _ = qfl_elem(xg[w], zero, zero)
        g_slot = dx1_ * ccls * gsc
        n_slot = e_dx1 * ccls * gsc + 5.0 * u * g_slot.abs()
        dp[img[w], 64 + cls[w], idx[w]] = g_slot
        dpn[img[w], 64 + cls[w], idx[w]] = n_slot
        slot[img[w], cls[w], idx[w]] = True
        cls_sum = cls_sum + (v1 - v0w).sum()
        cls_noise = cls_noise + (e_v1 + e_v0w + u * (v1.abs() + v0w.abs())).sum()
    mean_cls, mean_dfl = cls_sum / a / n_eff, dfl_img.sum() / n_eff
    out = torch.stack([lam_dfl * mean_dfl + lam_cls * mean_cls, mean_dfl, mean_cls]).to(dt)
    n_c, n_d = cls_noise / a / n_eff, dfl_noise.sum() / n_eff
    out_noise = torch.stack([lam_dfl * n_d + lam_cls * n_c + 2.0 * u * out[0].abs(), n_d, n_c]).to(dt)
    return {"dp": dp, "dp_noise": dpn, "slot": slot, "matched": matched, "out": out, "out_noise": out_noise}


def round_to(t, dtype):
    return t.to(F32).to(dtype)


# ------------------------------------------------------------------------------------------------------ the comparison
def _close(got, ref, noise, dtype, what, family, old=None):
    try:
        return sc.assert_close(got, ref, noise / U24, dtype, what, family=family, c=1.0, old_abs=old if GUARD else None)
    except StrictMismatch as ex:
        raise StrictMismatch(f"[loss: c = 1 on M = noise / 2^-24, the noise budget of strict_loss.py at c = "
                             f"{sc.C.get(family, sc.C_DEFAULT):g}; 'image' is the image, a 16-pixel block the anchor block "
                             f"(n A + a) / 16]\n{ex}", ex.count, ex.hist, ex.worst) from None


def check_decode(case, pbox):
    ref, noise = decode64(case)
    _close(pbox.detach().cpu().view(case.N, case.A, 4).permute(0, 2, 1), ref.permute(0, 2, 1), noise.permute(0, 2, 1), F32,
           f"{case.what} pbox", "loss_decode")


def check_assign(case, idx, pbox):
    """(a) exact against fp32 cdist + argmin on the CPU; (b) the float64 margin.  Both on the kernel's own pbox."""
    idx = idx.detach().cpu().long()
    pbox = pbox.detach().cpu().view(case.N, case.A, 4)
    want = assign_cpu(case, pbox)
    fam = "loss_assign"
    o = sc.OBSERVED.setdefault(fam, [float("-inf"), 0, 0])
    bad = (idx != want).nonzero().flatten().tolist()
    worst = float("-inf")
    lines = []
    if bad:
        lines.append(f"{len(bad)} of {idx.numel()} GT rows differ from cdist().argmin(1): " +
                     ", ".join(f"row {r}: {int(idx[r])} != {int(want[r])}" for r in bad[:16]))
    if case.expect_idx:
        off = [(r, k) for r, k in case.expect_idx if int(idx[r]) != k]
        if off:
            lines.append("rows not on the anchor their construction aims at (row, got, want): " +
                         ", ".join(f"({r}, {int(idx[r])}, {k})" for r, k in off[:16]))
    row = 0
    for n, g in enumerate(case.gts):
        m = g.shape[0]
        if not m:
            continue
        a_, b_ = g[:, :2].double(), pbox[n, :, :2].double()
        d2 = ((a_[:, None] - b_[None]) ** 2).sum(2)
        mass = (a_ ** 2).sum(1)[:, None] + (b_ ** 2).sum(1)[None] + 2.0 * (a_[:, None] * b_[None]).abs().sum(2)
        eps = 8.0 * U24 * mass + 2.0 * U24 * d2
        ch = idx[row:row + m].clamp(0, case.A - 1)
        best = d2.argmin(1)
        ar = torch.arange(m)
        over = d2[ar, ch] - d2[ar, best]
        margin = eps[ar, ch] + eps[ar, best]
        share = over / margin.clamp_min(1e-300)
        worst = max(worst, float(share.max()))
        for r in (share > 1).nonzero().flatten().tolist():
            lines.append(f"image {n} row {row + r}: anchor {int(ch[r])} at d^2 {float(d2[r, ch[r]]):.9g}, the minimum "
                         f"{float(d2[r, best[r]]):.9g} at {int(best[r])}: {float(share[r]):.2f} of the margin")
        row += m
    o[0], o[1], o[2] = max(o[0], worst), o[1] + idx.numel(), o[2] + 1
    if lines:
        raise StrictMismatch(f"{case.what} idx [{fam}, c = 1]: " + "\n  ".join(lines), len(lines), {}, [])


def check_gradients(case, dp, ref, old=None, families=("loss_dense", "loss_box", "loss_slot")):
    """dp: (N, 64 + nc, A) in case.dtype; ref: evaluate(...) in float64 from the same idx and pbox.  Raises the first
    family's StrictMismatch after trying every family (`.families`: all that failed)."""
    dp = dp.detach().cpu()
    assert dp.dtype == case.dtype and tuple(dp.shape) == tuple(ref["dp"].shape), (dp.dtype, dp.shape)
    failed = []
    r, nz = ref["dp"], ref["dp_noise"]
    g64 = dp.to(F64)
    cls_got, cls_ref, cls_nz = g64[:, 64:], r[:, 64:], nz[:, 64:]
    parts = {"loss_dense": (torch.where(ref["slot"], cls_ref, cls_got), cls_ref, cls_nz, old),
             "loss_slot": (torch.where(ref["slot"], cls_got, cls_ref), cls_ref, cls_nz, None),
             "loss_box": (g64[:, :64], r[:, :64], nz[:, :64], old)}
    for fam in families:
        got, rf, nn, o = parts[fam]
        if fam == "loss_slot" and not bool(ref["slot"].any()):
            continue
        try:
            _close(got, rf, nn, case.dtype, f"{case.what} dpreds", fam, o)
        except StrictMismatch as ex:
            failed.append((fam, ex))
    if failed:
        ex = failed[0][1]
        ex.families = [f for f, _ in failed]
        raise ex


def check_scalars(case, out, ref):
    try:
        _close(out.detach().cpu().view(1, 3, 1), ref["out"].view(1, 3, 1), ref["out_noise"].view(1, 3, 1), F32,
               f"{case.what} out", "loss_scalars")
    except StrictMismatch as ex:
        ex.families = ["loss_scalars"]
        raise


def old_abs(ref_dp, dtype):
    return OLD_TOL[dtype] * max(float(ref_dp.abs().max()), 1e-30)


def verify(case, out, dp, pbox, idx, old=None):
    """all six families, stage-wise, on what one launch left behind.  Raises StrictMismatch (`.families`) after every family
    has been tried."""
    failed = []
    pbox = pbox.detach().cpu().view(case.N, case.A, 4)
    idx = idx.detach().cpu().long()
    ref = evaluate(case, idx.clamp(0, case.A - 1), pbox)
    steps = [(("loss_decode",), lambda: check_decode(case, pbox)), (("loss_assign",), lambda: check_assign(case, idx, pbox)),
             (("loss_scalars",), lambda: check_scalars(case, out, ref))]
    if dp is not None:
        steps.append((("loss_dense", "loss_box", "loss_slot"), lambda: check_gradients(case, dp, ref, old)))
    for fams, fn in steps:
        try:
            fn()
        except StrictMismatch as ex:
            failed.append((getattr(ex, "families", list(fams)), ex))
    if failed:
        ex = failed[0][1]
        ex.families = [f for fs, _ in failed for f in fs]
        raise StrictMismatch(str(ex) + f"\n[families outside their limits: {ex.families}]", ex.count, ex.hist, ex.worst)
    return ref


def failing_families(fn):
    """the families a call of verify / check_* fails in (empty: it passes)"""
    try:
        fn()
    except StrictMismatch as ex:
        m = re.search(r"\[families outside their limits: \[(.*?)\]\]", str(ex))
        if m:
            return [s.strip(" '") for s in m.group(1).split(",")]
        return getattr(ex, "families", None) or [re.search(r" \[(loss_\w+), c = ", str(ex)).group(1)]
    return []
