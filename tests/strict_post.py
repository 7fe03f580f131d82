"""Strict comparators for the post-processing kernels of csrc/decode_nms.hip: k_head_decode, k_dfl_expect, the five NMS
kernels (k_cand_count, k_candidates, k_rank, k_mask, k_scan) and the five validation kernels (k_val_count,
k_val_candidates, k_val_rank, k_val_gather, k_val_match).  On top of strict_compare.py (its ulp(), assert_close,
StrictMismatch, OBSERVED / report()) and strict_move.py (bits(): the integer image of a tensor, every NaN one value).
Shared by tests/test_strict_post_cpu.py (the proof of the comparators, no GPU) and tests/test_gpu_post.py (the kernels).

Bound class (families post_decode, post_dfl).  float64 reference from the T-rounded inputs; U = 2^-24 (one fp32 rounding,
relative), c = 16 (sc.C, the rule of strict_compare.py applies) on the summation term only.  Per side, the model of
strict_loss.py's loss_decode:
    E  = sum_b p_b b,  p = softmax of the 16 logits x_b, mx their maximum
    dE = U sum_b p_b b (|x_b - mx| + 6) + c U E + 120 x 2^-149
(x - mx rounds: U |x - mx| into expf; expf 2 U; the division, the product with b, 2 U for the sum the softmax divides by;
c: the two 16-term sums; the last term: an expf result below 2^-126 is a subnormal and carries an ABSOLUTE error of one
subnormal spacing 2^-149, times the bin, summed over the bins 1..15 = 120).  k_dfl_expect stores round_T(E): noise dE.
k_head_decode forms, in fp32, x1 = a - E_l, x2 = a + E_r, then (x1 + x2) / 2 * st and (x2 - x1) * st, one rounding to T:
    corners   d1 = dE_l + U (|a| + E_l),  d2 = dE_r + U (|a| + E_r)               (the subtraction / addition rounds once)
    centre    st ((d1 + d2) / 2 + 2 U (|x1| + |x2| + d1 + d2) / 2)                 (the add and the product with st; / 2 exact)
    size      st ((d1 + d2)     + 2 U (|x2 - x1| + d1 + d2))                       (x2 - x1 cancels: the corners' ABSOLUTE error)
The comparator grants 1/2 ulp_T(max(|ref|, |got|)) itself; no constant is fitted.  strict_compare.assert_close carries the
limit with c = 1 and mass = noise / U, so the figure recorded per family is the share of the noise used (limit 1).  The
former check() limit (TOL x the largest element of the WHOLE decoded tensor) goes in as old_abs: the new limit is asserted
to be nowhere wider.  The class rows of k_head_decode are copies: exact class (family post_cls), -0.0 and NaN preserved.

Exact class, NMS (family post_nms): the padded [bs][max_det][6] rows, the counts and the status of ops.nms against
oracle.postproc.non_max_suppression, bit for bit; the rows past the count are zero.  A mismatch names the image, the row and
the column.  nms_emul() restates the device's structure (candidates in T arithmetic, stable rank, cut at MAX_NMS, greedy
scan over the offset boxes) in numpy fp32; without a mutation it equals the oracle on every case (asserted on the CPU), with
one it is the subtly wrong kernel the cases must catch.

Decided-set class, val_select (family post_select).  s = sigmoid(x) in float64 from the T-rounded logit, e = 4 U s (the
sigmoid term of strict_loss.py: expf 2 U (1 - s), the add, the division).  The kernel stores round_T(v) for some fp32 v in
[s - e, s + e]; rounding is monotone, so the stored score lies in [lo, hi] = [round_T(s - e), round_T(s + e)] (one value
when both ends round alike).  Per anchor, L = max_c lo_c, H = max_c hi_c:
    score     the got score lies in [lo, hi] of the got class and is >= L (the kernel took a maximum)
    class     the got class is a contender (hi_c >= L: no other class can hold the maximum); contenders that hold ONE logit store one value
              (the score is a function of the logit alone), so the first of them is the class, a single contender
              included; when every contender is decided (lo_c == hi_c) the stored values are known and the FIRST class
              holding the largest must be reported; otherwise the anchor is class-undecided (counted where it can be kept)
    kept      conf_T = round_T(conf).  L >= conf_T: must be kept; H < conf_T, or a NaN class logit (amax / max(1) propagate
              NaN and NaN >= conf is false: the reference drops the anchor): must be dropped; else threshold-undecided
    order     at most top_k anchors can pass (count of H >= conf_T): ascending anchor, every must-keep present.  More than
              top_k must pass: exactly top_k rows, descending got score, lower anchor first on equal got scores; a dropped
              must-keep anchor a is WRONG when it certainly ranks before the last kept row (score s_k, anchor a_k):
              L_a > s_k, or L_a == s_k with a < a_k; when only its upper value does (H_a > s_k, or == with a < a_k) the
              anchor is rank-undecided; H_a <= s_k otherwise is what a correct kernel leaves.  Two anchors whose score comes
              from ONE logit hold equal scores whatever they are: the lower anchor must win, nothing is undecided.  Between the two counts the
              path itself is open: the whole image counts as undecided.
    copies    the box columns are the anchor's, bit for bit (they carry the anchor index); rows past the count are zero
An anchor with any check undecided counts as undecided; above UNDECIDED_CAP = 0.5 % of a case's anchors the case fails as
"cannot tell".  That is a condition on the inputs: select_undecided() evaluates it from the reference alone.

Exact class, val_match (family post_match): the int64 counters and the status against emulated_ops.val_match (the oracle's
MetricCounters), an image with more than 1024 targets left out of the expectation (the kernel reports status 1 and skips it).

Recorded on the MI355X: OBSERVED_GPU.  CPU stand-ins: tests/test_strict_post_cpu.py, STAND_IN_MAXIMA."""
import functools

import numpy as np
import torch

import strict_compare as sc
from strict_compare import U24, StrictMismatch, ulp  # noqa: F401  (re-exported for the tests)
from strict_move import bits

F32, F64, BF, HF = torch.float32, torch.float64, torch.bfloat16, torch.float16
REG = 16
MAX_WH, MAX_NMS, NMS_CAP, VAL_MAX_GT = 7680.0, 30000, 131072, 1024
FAMILIES = ("post_decode", "post_dfl")
for _f in FAMILIES:
    sc.C[_f] = sc.C_DEFAULT
    sc.BUDGET_FAMILIES.add(_f)
OLD_TOL = {F32: 1e-4, BF: 2.0 ** -6, HF: 2.0 ** -9}       # check() of tests/test_gpu_kernels.py
SUBNORMAL = 120.0 * 2.0 ** -149
UNDECIDED_CAP = 0.005
GUARD = True
EXACT = {}                    # family -> [comparisons, elements] of the exact classes
UNDECIDED = [0.0]             # largest undecided share of a post_select case
OBSERVED_GPU = """MI355X, tests/test_gpu_post.py, 2026-10-20 (467 cases, every one twice: 93 decode / DFL, 39 + 42 known-answer NMS, 259 select,
34 match; 1.44 M bound-class elements): post_decode 0.860 (the width of the 1280 input's first level at anchor x = 129.5, fp32:
x2 - x1 cancels and carries the corners' absolute error, as the derivation has it), post_dfl 0.577 (of the noise, limit 1);
exact classes bit-equal: post_cls 93 comparisons / 3.14 M elements, post_nms 203 / 270 k (rows, counts, status), post_match
34 / 938 counters; post_select 259 / 516 k, largest undecided share 0.0476 % (cap 0.5 %).
Defect found: a NaN class score did not drop its anchor (cand_eval in both modes, val_eval): nonfinite-* failed on the
kernels before this file (NMS counts [45, 43] for [43, 42]; val_select kept anchors 5, 6, 256 of image 0 / 1), fixed with
one comparison per class; nothing else mismatched.  The module takes 2.6 s (2.2 s inside the tests)."""


def _tally(family, elems):
    o = EXACT.setdefault(family, [0, 0])
    o[0], o[1] = o[0] + 1, o[1] + int(elems)


def _fail(family, lines, count=1):
    e = StrictMismatch("\n".join(lines), count, {}, [])
    e.families = [family]
    raise e


def failing_families(fn):
    try:
        fn()
    except StrictMismatch as e:
        return list(getattr(e, "families", ["?"]))
    return []


def round_to(t, dtype):
    """float64 -> the value of `dtype` the device's fp32 -> T conversion stores, as float64"""
    return t.to(F32).to(dtype).to(F64)


# ====================================================================================================== decode, DFL
def level_anchors(a, size=320):
    """anchors (2, A) and strides (1, A) fp32.  A == 2100 (size 320): make_anchors' 40^2 + 20^2 + 10^2; a smaller A takes
    the first ceil(0.6 A) anchors of level 0, then ceil(0.3 A) of level 1, the rest from level 2 (A == 1: level 0 alone)"""
    lv = []
    for s in (8, 16, 32):
        g = size // s
        yy, xx = torch.meshgrid(torch.arange(g), torch.arange(g), indexing="ij")
        lv.append((xx.flatten() + 0.5, yy.flatten() + 0.5, torch.full((g * g,), float(s))))
    full = sum(v[0].numel() for v in lv)
    if a == full:
        take = [v[0].numel() for v in lv]
    else:
        assert a < lv[2][0].numel() * 3
        t0 = -(-a * 6 // 10)
        t1 = min(a - t0, -(-a * 3 // 10))
        take = [t0, t1, a - t0 - t1]
    ax = torch.cat([v[0][:t] for v, t in zip(lv, take)])
    ay = torch.cat([v[1][:t] for v, t in zip(lv, take)])
    st = torch.cat([v[2][:t] for v, t in zip(lv, take)])
    return torch.stack([ax, ay]).float(), st.view(1, -1).float(), take


def first_level_1280():
    """the 160 x 160 stride-8 anchors of a 1280 input: coordinates reach 159.5"""
    yy, xx = torch.meshgrid(torch.arange(160), torch.arange(160), indexing="ij")
    return torch.stack([xx.flatten() + 0.5, yy.flatten() + 0.5]).float(), torch.full((1, 25600), 8.0)


def decode_logits(n, a, nc, dtype, seed):
    """preds (N, 64 + nc, A) of `dtype`.  The four logit classes by (image + side + anchor) % 4:
    0 flat: base + randn / 4, base in {0, 100, -100} by anchor (exp(100) overflows fp32 without the max subtraction);
    1 one dominant bin at 0 (+ 8); 2 one dominant bin at 15; 3 a spread of +-60.
    Class logits: randn * 3 with -0.0, NaN, +-inf and a subnormal of T in the first anchors of class 0"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 4, REG, a, generator=g)
    kind = (torch.arange(n).view(n, 1, 1) + torch.arange(4).view(1, 4, 1) + torch.arange(a).view(1, 1, a)) % 4
    base = torch.tensor([0.0, 100.0, -100.0])[(torch.arange(a) // 4) % 3].view(1, 1, 1, a)
    flat = base + x / 4
    dom0, dom15 = x.clone(), x.clone()
    dom0[:, :, 0] += 8.0
    dom15[:, :, 15] += 8.0
    spread = (torch.rand(n, 4, REG, a, generator=g) * 2 - 1) * 60
    k = kind.unsqueeze(2)
    box = torch.where(k == 0, flat, torch.where(k == 1, dom0, torch.where(k == 2, dom15, spread)))
    cls = torch.randn(n, nc, a, generator=g) * 3
    edge = [-0.0, float("nan"), float("inf"), float("-inf"), 2.0 ** -140 if dtype != HF else 2.0 ** -20]
    for i, v in enumerate(edge[:a]):
        cls[0, 0, i] = v
        cls[n - 1, nc - 1, a - 1 - i] = v
    return torch.cat([box.reshape(n, 64, a), cls], 1).to(dtype)


def dfl_ref(x64):
    """x64 (B, 4, 16, A) float64 -> (E, dE), both (B, 4, A)"""
    mx = x64.amax(2, keepdim=True)
    d = x64 - mx
    ex = torch.exp(d)
    p = ex / ex.sum(2, keepdim=True)
    bins = torch.arange(REG, dtype=F64).view(1, 1, REG, 1)
    e = torch.zeros_like(p[:, :, 0])
    for b in range(REG):                                      # the kernel's order: bin after bin
        e = e + p[:, :, b] * float(b)
    de = U24 * (p * bins * (d.abs() + 6.0)).sum(2) + sc.C["post_dfl"] * U24 * e + SUBNORMAL
    return e, de


def decode_ref(preds, anchors, strides):
    """preds (N, 64 + nc, A), anchors (2, A), strides (1, A), all values of T -> (box (N, 4, A) float64 cx cy w h, noise)"""
    n, _, a = preds.shape
    e, de = dfl_ref(preds[:, :64].double().view(n, 4, REG, a))
    ax, ay, st = anchors[0].double(), anchors[1].double(), strides[0].double()
    out, noise = [], []
    for an, lo, hi in ((ax, 0, 2), (ay, 1, 3)):
        x1, x2 = an - e[:, lo], an + e[:, hi]
        d1, d2 = de[:, lo] + U24 * (an.abs() + e[:, lo]), de[:, hi] + U24 * (an.abs() + e[:, hi])
        out.append(((x1 + x2) / 2 * st, (x2 - x1) * st))
        noise.append((st * ((d1 + d2) / 2 + 2 * U24 * (x1.abs() + x2.abs() + d1 + d2) / 2),
                      st * ((d1 + d2) + 2 * U24 * ((x2 - x1).abs() + d1 + d2))))
    box = torch.stack([out[0][0], out[1][0], out[0][1], out[1][1]], 1)
    return box, torch.stack([noise[0][0], noise[1][0], noise[0][1], noise[1][1]], 1)


def decode_emul(preds, anchors, strides, nc, mut=None, take=None):
    """the kernel's formula in fp32 torch, one rounding to T; mut: bins1 | round_e | no_max | stride"""
    dtype = preds.dtype
    n, _, a = preds.shape
    x = preds[:, :64].float().view(n, 4, REG, a)
    if mut != "no_max":
        x = x - x.amax(2, keepdim=True)
    ex = torch.exp(x)
    p = ex / ex.sum(2, keepdim=True)
    e = torch.zeros(n, 4, a)
    for b in range(REG):
        e = e + p[:, :, b] * float(b + 1 if mut == "bins1" else b)
    if mut == "round_e":
        e = e.to(dtype).float()
    st = strides[0].float().clone()
    if mut == "stride":                                       # the first anchor of a level takes the level before's stride
        for first in np.cumsum(take)[:-1]:
            if first < a:
                st[first] = st[first - 1]
    ax, ay = anchors[0].float(), anchors[1].float()
    x1, y1, x2, y2 = ax - e[:, 0], ay - e[:, 1], ax + e[:, 2], ay + e[:, 3]
    box = torch.stack([(x1 + x2) / 2 * st, (y1 + y2) / 2 * st, (x2 - x1) * st, (y2 - y1) * st], 1)
    return torch.cat([box.to(dtype), preds[:, 64:]], 1)


def dfl_emul(x, mut=None):
    """k_dfl_expect's formula in fp32 torch, one rounding to T; mut: bins1 | no_max"""
    n, _, a = x.shape
    v = x.float().view(n, 4, REG, a)
    if mut != "no_max":
        v = v - v.amax(2, keepdim=True)
    ex = torch.exp(v)
    p = ex / ex.sum(2, keepdim=True)
    e = torch.zeros(n, 4, a)
    for b in range(REG):
        e = e + p[:, :, b] * float(b + 1 if mut == "bins1" else b)
    return e.to(x.dtype)


def _old_abs(whole_ref, dtype):
    fin = torch.where(torch.isfinite(whole_ref), whole_ref, torch.zeros_like(whole_ref))
    return OLD_TOL[dtype] * max(float(fin.abs().max()) if fin.numel() else 0.0, 1e-6)


def assert_exact(got, want, what, family, names=("image", "row", "column")):
    """bit equality (NaN == NaN) of two tensors of one shape and dtype; the message names the first differing elements"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    _tally(family, got.numel())
    bad = bits(got) != bits(want)
    if bool(bad.any()):
        idx = bad.nonzero()
        lines = [f"{what} [{family}]: {int(bad.sum())} of {got.numel()} elements differ bit for bit; first ({', '.join(names[:got.dim()])}): got, want"]
        for i in idx[:32]:
            t = tuple(i.tolist())
            lines.append(f"    {dict(zip(names, t))}  {float(got[t]):.9g}  {float(want[t]):.9g}")
        _fail(family, lines, int(bad.sum()))


def check_decode(preds, anchors, strides, nc, got, what):
    """got (N, 4 + nc, A) of T: the box rows inside the bound, the class rows bit-equal -> share of the noise used"""
    dtype = preds.dtype
    box, noise = decode_ref(preds.cpu(), anchors.cpu(), strides.cpu())
    got = got.detach().cpu()
    assert got.dtype == dtype and tuple(got.shape) == (preds.shape[0], 4 + nc, preds.shape[2]), (what, got.shape, got.dtype)
    assert_exact(got[:, 4:], preds.cpu()[:, 64:], what + " class rows", "post_cls", ("image", "class", "anchor"))
    whole = torch.cat([box, preds.cpu()[:, 64:].double()], 1)
    try:
        return sc.assert_close(got[:, :4], box, noise / U24, dtype, what + " (image, row cx cy w h, anchor)", "post_decode", c=1.0,
                               old_abs=_old_abs(whole, dtype) if GUARD else None)
    except StrictMismatch as e:
        e.families = ["post_decode"]
        raise


def check_dfl(x, got, what):
    dtype = x.dtype
    n, _, a = x.shape
    e, de = dfl_ref(x.cpu().double().view(n, 4, REG, a))
    got = got.detach().cpu()
    assert got.dtype == dtype and tuple(got.shape) == (n, 4, a), (what, got.shape, got.dtype)
    try:
        return sc.assert_close(got, e, de / U24, dtype, what + " (image, side, anchor)", "post_dfl", c=1.0,
                               old_abs=_old_abs(e, dtype) if GUARD else None)
    except StrictMismatch as e_:
        e_.families = ["post_dfl"]
        raise


DECODE_A = (1, 255, 256, 257, 2100)
DECODE_CASES = [(a, n, nc) for a in DECODE_A for n in (1, 3) for nc in (1, 8, 80)]


def decode_case(a, n, nc, dtype):
    """-> preds, anchors, strides (values of T, CPU), take (anchors per level)"""
    if a == 25600:
        anc, st = first_level_1280()
        take = [a]
    else:
        anc, st, take = level_anchors(a)
    return decode_logits(n, a, nc, dtype, 7 * a + 3 * n + nc), anc.to(dtype), st.to(dtype), take


# ====================================================================================================== NMS
class NmsCase:
    def __init__(self, name, y, nc, **kw):
        self.name, self.y, self.nc = name, y, nc
        self.kw = dict(conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, max_det=300)
        self.kw.update(kw)
        self.keep = None                # known answer: per image the kept input anchors, in output order

    def args(self):
        k = self.kw
        return (self.nc, k["conf_thres"], k["iou_thres"], k["classes"], k["agnostic"], k["multi_label"], k["max_det"])


def nms_expect(case):
    """-> (rows fp32 [bs][max_det][6], counts int32 [bs], status) of the oracle; more candidates than the capacity: status 1"""
    from oracle import postproc as opost
    k = case.kw
    y = case.y
    bs, _, m = y.shape
    ml = k["multi_label"] and case.nc > 1
    if ml:
        confT = torch.tensor(k["conf_thres"]).to(y.dtype)
        cand = (y[:, 4:].amax(1) > confT).unsqueeze(1) & (y[:, 4:] > confT)
        if k["classes"] is not None:
            keep = torch.zeros(case.nc, dtype=torch.bool)
            keep[list(k["classes"])] = True
            cand &= keep.view(1, -1, 1)
        if int(cand.sum((1, 2)).max()) > NMS_CAP:
            return None, None, 1
    res = opost.non_max_suppression(y.clone(), k["conf_thres"], k["iou_thres"], k["classes"], k["agnostic"], k["multi_label"], (),
                                    k["max_det"], case.nc)
    rows = torch.zeros(bs, k["max_det"], 6)
    counts = torch.zeros(bs, dtype=torch.int32)
    for i, r in enumerate(res):
        rows[i, :r.shape[0]] = r.float()
        counts[i] = r.shape[0]
    return rows, counts, 0


def check_nms(case, got_rows, got_counts, got_status, want=None):
    """the device's padded rows, counts and status against the oracle's, bit for bit"""
    rows, counts, status = want if want is not None else nms_expect(case)
    what = f"nms {case.name}"
    gs = int(torch.as_tensor(got_status).reshape(-1)[0])
    _tally("post_nms", 1)
    if gs != status:
        _fail("post_nms", [f"{what} [post_nms]: status {gs}, want {status}"])
    if status:
        return
    gc = got_counts.detach().cpu().to(torch.int32)
    if not torch.equal(gc, counts):
        badi = (gc != counts).nonzero().flatten().tolist()
        _fail("post_nms", [f"{what} [post_nms]: counts differ in images {badi[:16]}: got {gc[badi[:16]].tolist()}, want {counts[badi[:16]].tolist()}"],
              len(badi))
    assert_exact(got_rows.detach().cpu().reshape(rows.shape), rows, what + " rows (x1 y1 x2 y2 conf cls)", "post_nms")


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _iou_row(bi, rest, mut):
    """fp32 IoU of box bi (4,) with boxes rest (k, 4), torchvision's formula; mut: eps | fma"""
    f = np.float32
    w = np.maximum(f(0), np.minimum(bi[2], rest[:, 2]) - np.maximum(bi[0], rest[:, 0]))
    h = np.maximum(f(0), np.minimum(bi[3], rest[:, 3]) - np.maximum(bi[1], rest[:, 1]))
    inter = w * h
    ai = (bi[2] - bi[0]) * (bi[3] - bi[1])
    dxj, dyj = rest[:, 2] - rest[:, 0], rest[:, 3] - rest[:, 1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if mut == "fma":
            union = _fma32(-w, h, _fma32(dxj, dyj, np.broadcast_to(ai, dxj.shape)))
        else:
            union = ai + dxj * dyj - inter
        if mut == "eps":
            union = union + f(1e-6)
        return inter / union


def nms_emul(y, nc, conf_thres, iou_thres, classes, agnostic, multi_label, max_det, mut=None):
    """the device's structure in numpy fp32 (see the module docstring) -> rows [bs][max_det][6], counts, status.
    mut: ge | eps | tie_high | xyxy_f32 | fma | off4096 | cut | past_max_det | mask_prev | nan_skip"""
    dtype = y.dtype
    bs, _, m = y.shape
    cap = min(m * (nc if multi_label else 1), NMS_CAP)
    flat = np.zeros((bs * max_det + 1, 6), np.float32)        # one row to spare: the last image's row max_det
    counts = np.zeros(bs, np.int32)
    status = 0
    conf_t = torch.tensor(conf_thres).to(dtype).float()
    thr = np.float32(iou_thres)
    sorted_boxes = []
    for img in range(bs):
        yi = y[img]
        cls = yi[4:4 + nc].float()
        nan = torch.isnan(cls).any(0)
        if mut == "nan_skip":
            cls = torch.where(torch.isnan(cls), torch.full_like(cls, float("-inf")), cls)
            nan = torch.zeros_like(nan)
        if multi_label:
            ok = (cls > conf_t) & ~nan.unsqueeze(0)
            if classes is not None:
                keep = torch.zeros(nc, dtype=torch.bool)
                keep[list(classes)] = True
                ok &= keep.view(-1, 1)
            a_idx, c_idx = ok.t().nonzero(as_tuple=True)      # anchor-major, classes ascending
            score = cls[c_idx, a_idx]
        else:
            best, bc = cls.max(0)                             # first maximum; a NaN propagates and fails the comparison
            ok = (best > conf_t) & ~nan
            if classes is not None:
                ok &= (bc.view(-1, 1) == torch.tensor(list(classes)).view(1, -1)).any(1)
            a_idx = ok.nonzero().flatten()
            c_idx, score = bc[a_idx], best[a_idx]
        b4 = yi[:4] if mut != "xyxy_f32" else yi[:4].float()  # each operation rounded in T
        dw, dh = b4[2] / 2, b4[3] / 2
        box = torch.stack([b4[0] - dw, b4[1] - dh, b4[0] + dw, b4[1] + dh], 1).float()[a_idx].numpy()
        score, clsf = score.numpy().astype(np.float32), c_idx.float().numpy()
        n = len(score)
        if n > cap:
            status, n = 1, cap
            box, score, clsf = box[:n], score[:n], clsf[:n]
        if mut == "tie_high":
            order = np.lexsort((-np.arange(n), -score))
        else:
            order = np.argsort(-score, kind="stable")
        order = order[:MAX_NMS - 1 if mut == "cut" else MAX_NMS]
        off = clsf[order, None] * np.float32(0.0 if agnostic else (4096.0 if mut == "off4096" else MAX_WH))
        ob = (box[order] + off).astype(np.float32)
        sorted_boxes.append(ob)
        mb = ob if not (mut == "mask_prev" and img >= 8) else sorted_boxes[img - 8]
        ns = len(order)
        dead = np.zeros(ns, bool)
        kept = 0
        for i in range(ns):
            if dead[i]:
                continue
            if kept == max_det:
                if mut == "past_max_det":
                    flat[img * max_det + kept] = np.concatenate([box[order[i]], [score[order[i]], clsf[order[i]]]])
                break
            flat[img * max_det + kept] = np.concatenate([box[order[i]], [score[order[i]], clsf[order[i]]]])
            kept += 1
            hi = min(ns, len(mb))
            if i + 1 < hi:
                iou = _iou_row(mb[i], mb[i + 1:hi], mut)
                with np.errstate(invalid="ignore"):
                    dead[i + 1:hi] |= (iou >= thr) if mut == "ge" else (iou > thr)
        counts[img] = kept
    rows = torch.from_numpy(flat[:bs * max_det].reshape(bs, max_det, 6).copy())
    return rows, torch.from_numpy(counts), status


def _xywh(b):
    b = torch.as_tensor(b, dtype=F32)
    return torch.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 0)


def cluster_pred(bs, m, nc, dtype, seed, npass, cls_set=(0,), nclus=24, levels=None, multi=False, ladder=False):
    """(bs, 4 + nc, M): boxes in `nclus` tight clusters (centres 96 px apart, jitter of +-2 px in quarter pixels, sides
    48 .. 52), so that the oracle keeps about nclus x len(cls_set) rows per image.  npass[i] anchors of image i (a random
    subset) carry a score in (0.3, 0.95) in one class of cls_set, every other score is at most 0.2.  levels: the passing
    scores come from that many distinct values (ties); multi: every class of an anchor draws its own score, npass is
    ignored; ladder: distinct scores 0.95 - k 2^-16 in a random order (every anchor passes)"""
    g = torch.Generator().manual_seed(seed)
    y = torch.zeros(bs, 4 + nc, m)
    cl = torch.randint(0, nclus, (bs, m), generator=g)
    y[:, 0] = 64 + 96.0 * (cl % 6) + torch.randint(-8, 9, (bs, m), generator=g) * 0.25
    y[:, 1] = 64 + 96.0 * (cl // 6) + torch.randint(-8, 9, (bs, m), generator=g) * 0.25
    y[:, 2] = 48 + torch.randint(0, 17, (bs, m), generator=g) * 0.25
    y[:, 3] = 48 + torch.randint(0, 17, (bs, m), generator=g) * 0.25
    if multi:
        y[:, 4:] = torch.rand(bs, nc, m, generator=g) * 0.65 + 0.3
        return y.to(dtype)
    y[:, 4:] = torch.rand(bs, nc, m, generator=g) * 0.2
    for i in range(bs):
        k = m if ladder else int(npass[i])
        pick = torch.randperm(m, generator=g)[:k]
        if ladder:
            sc_ = 0.95 - torch.randperm(m, generator=g).float() * 2.0 ** -16
        elif levels:
            sc_ = 0.3 + torch.randint(0, levels, (k,), generator=g).float() * (0.64 / levels)
        else:
            sc_ = 0.3 + torch.rand(k, generator=g) * 0.65
        c = torch.tensor(cls_set)[torch.randint(0, len(cls_set), (k,), generator=g)]
        y[i, 4 + c, pick] = sc_
    return y.to(dtype)


@functools.lru_cache(maxsize=None)
def fma_pair():
    """two fp32 boxes whose IoU differs in the last place between separate roundings and fused multiply-adds, and the
    threshold that separates the two values -> (boxes xyxy (2, 4) numpy fp32, thr)"""
    rng = np.random.RandomState(5)
    k = 200000
    a = np.array([10.0, 10.0, 50.0, 50.0], np.float32) + rng.rand(k, 4).astype(np.float32)
    b = a + (rng.rand(k, 4).astype(np.float32) * 6 - 3)
    p = np.stack([_iou_row(a[i], b[i:i + 1], None)[0] for i in range(2000)])
    q = np.stack([_iou_row(a[i], b[i:i + 1], "fma")[0] for i in range(2000)])
    i = int(np.nonzero((p != q) & (np.minimum(p, q) > 0.3))[0][0])
    return np.stack([a[i], b[i]]), float(min(p[i], q[i]))


def _score_rows(boxes_xyxy, scores, nc=1, cls=None):
    """y (1, 4 + nc, n) fp32 from xyxy boxes at coordinates whose xywh form is exact"""
    b = torch.as_tensor(np.asarray(boxes_xyxy), dtype=F32)
    n = b.shape[0]
    y = torch.zeros(1, 4 + nc, n)
    y[0, :4] = _xywh(b)
    back = torch.stack([y[0, 0] - y[0, 2] / 2, y[0, 1] - y[0, 3] / 2, y[0, 0] + y[0, 2] / 2, y[0, 1] + y[0, 3] / 2], 1)
    assert torch.equal(back, b), "xywh -> xyxy is not exact for these boxes"
    for i in range(n):
        y[0, 4 + (0 if cls is None else cls[i]), i] = scores[i]
    return y


# the cases of tests/test_nms_known.py: (name, boxes xyxy, scores, thr, hand-computed keep list); 10.2 there is 10.25 here
_CHAIN = [[0., 0., 10., 10.], [2.5, 0., 12.5, 10.], [5., 0., 15., 10.]]
_HALF = [[0., 0., 10., 7.5], [0., 2.5, 10., 10.]]
_DISJ = [[0., 0., 1., 1.], [5., 5., 6., 6.], [10., 10., 11., 11.], [20., 0., 21., 1.]]
_ZERO = [[1., 1., 1., 1.], [1., 1., 1., 1.], [0., 0., 4., 4.]]
_CONT = [[0., 0., 10., 10.], [2., 2., 8., 8.], [0., 0., 10., 10.25]]
_TIE = [[0., 0., 10., 10.], [0., 0., 10., 10.]]
_S = 2.0 ** -6       # two 1/64 squares a quarter side apart: inter 3 / 16384, union 5 / 16384, IoU = fl(0.6) exactly
_TINY = [[0., 0., _S, _S], [_S / 4, 0., _S + _S / 4, _S]]
KNOWN = [("chain.5", _CHAIN, [.9, .8, .7], 0.5, [0, 2]), ("chain.3", _CHAIN, [.9, .8, .7], 0.3, [0]),
         ("chain.7", _CHAIN, [.9, .8, .7], 0.7, [0, 1, 2]), ("half.5", _HALF, [.6, .5], 0.5, [0, 1]),
         ("half.4999", _HALF, [.6, .5], 0.4999, [0]), ("disjoint", _DISJ, [.1, .9, .5, .7], 0.45, [1, 3, 2, 0]),
         ("zero_area", _ZERO, [.9, .8, .7], 0.45, [0, 1, 2]), ("contained.45", _CONT, [.5, .9, .7], 0.45, [1, 2]),
         ("contained.3", _CONT, [.5, .9, .7], 0.3, [1]), ("tie", _TIE, [.5, .5], 0.45, [0]),
         # IoU = fl(0.6): strict at thr fl(0.6); just above the float below it (1e-6 in the union would lose the pair)
         ("tiny.6", _TINY, [.9, .8], float(np.float32(0.6)), [0, 1]),
         ("tiny.6-", _TINY, [.9, .8], float(np.nextafter(np.float32(0.6), np.float32(0))), [0])]


def known_cases(dtype):
    out = []
    for name, boxes, scores, thr, keep in KNOWN:
        if name.startswith("tiny") and dtype == HF:
            continue                                          # 3 / 16384 sits in f16's subnormal range: fp32 / bf16 only
        c = NmsCase(f"known-{name}", _score_rows(boxes, scores).to(dtype), 1, conf_thres=0.05, iou_thres=thr)
        c.keep = [keep]
        out.append(c)
    # the class offset: identical boxes in classes 0 and 79 both survive class-aware, one with agnostic; a box of class 1
    # at (100, 24) and one of class 0 at (4196, 4120) are 4096 apart in x and y: they meet only under an offset of 4096
    two = [[8., 8., 40., 40.], [8., 8., 40., 40.]]
    for ag, keep in ((False, [0, 1]), (True, [0])):
        c = NmsCase(f"known-offset-agnostic{int(ag)}", _score_rows(two, [.9, .8], 80, [0, 79]).to(dtype), 80, conf_thres=0.05, agnostic=ag)
        c.keep = [keep]
        out.append(c)
    if dtype != BF:
        far = [[4180., 4104., 4212., 4136.], [84., 8., 116., 40.]]
        c = NmsCase("known-offset-4096", _score_rows(far, [.9, .8], 2, [0, 1]).to(dtype), 2, conf_thres=0.05)
        c.keep = [[0, 1]]
        out.append(c)
    return out


def known_rows(case):
    """the rows a known-answer case must give, from its keep list alone (no oracle): boxes exact, scores as stored in T"""
    y = case.y.float()[0]
    k = case.kw["max_det"]
    rows = torch.zeros(1, k, 6)
    for r, a in enumerate(case.keep[0]):
        sc_, c = y[4:, a].max(0)
        rows[0, r] = torch.tensor([y[0, a] - y[2, a] / 2, y[1, a] - y[3, a] / 2, y[0, a] + y[2, a] / 2, y[1, a] + y[3, a] / 2,
                                   float(sc_), float(c)])
    return rows, torch.tensor([len(case.keep[0])], dtype=torch.int32), 0


def _kept(case):
    return [int(v) for v in nms_expect(case)[1]]


@functools.lru_cache(maxsize=None)
def nms_cases(group):
    """the cases of one group -> list of NmsCase (built once; every tensor stays unchanged)"""
    out = []
    if group == "compaction":
        for i, m in enumerate((1, 63, 64, 65, 255, 256, 257, 513)):
            d = (F32, HF, BF)[i % 3]
            out.append(NmsCase(f"M{m}", cluster_pred(2, m, 3, d, 100 + m, [m, max(1, m // 2)], (0, 2)), 3))
        out.append(NmsCase("counts-0-1-64-65-128-129", cluster_pred(6, 257, 3, F32, 120, [0, 1, 64, 65, 128, 129], (0, 1)), 3))
    elif group == "images":
        for bs in (1, 8, 9, 17):
            npass = [(37 * i + 11) % 200 + 1 for i in range(bs)]
            if bs > 1:
                npass[bs // 2], npass[bs - 1] = 0, 0          # an empty image in the middle, an empty last image
            if bs == 9:
                npass[8] = 150                                # image 8 opens the second launch pair and is not empty
            for d in ((F32, HF, BF) if bs == 9 else (F32,)):
                out.append(NmsCase(f"bs{bs}-{str(d)[6:]}", cluster_pred(bs, 257, 4, d, 200 + bs, npass, (0, 3)), 4))
        y = cluster_pred(17, 257, 2, F32, 230, [120] * 17, (0, 1), nclus=6)
        y[9, 4:] = 0.0                                        # a full image, then an empty one: a row past max_det shows
        out.append(NmsCase("bs17-max_det1", y, 2, max_det=1))
    elif group == "ties":
        y = cluster_pred(2, 513, 2, BF, 300, [400, 513], (0, 1), levels=20)
        c = NmsCase("bf16-20-levels", y, 2)
        out.append(c)
        rows = nms_expect(c)[0][0]
        cut = next(k for k in range(1, int(nms_expect(c)[1][0])) if rows[k - 1, 4] == rows[k, 4])
        out.append(NmsCase("bf16-ties-straddle-max_det", y, 2, max_det=cut))
    elif group == "options":
        ym = cluster_pred(2, 257, 8, F32, 400, None, multi=True, nclus=4)
        out.append(NmsCase("multi_label", ym, 8, multi_label=True, conf_thres=0.6, iou_thres=0.5))
        out.append(NmsCase("multi_label-classes", ym, 8, multi_label=True, conf_thres=0.6, iou_thres=0.5, classes=[1, 3, 6]))
        out.append(NmsCase("multi_label-f16", ym.to(HF), 8, multi_label=True, conf_thres=0.6, iou_thres=0.5))
        out.append(NmsCase("multi_label-nc1", cluster_pred(2, 257, 1, F32, 401, None, multi=True), 1, multi_label=True, conf_thres=0.6))
        ys = cluster_pred(2, 257, 4, F32, 402, [200, 180], (0, 1, 3))
        out.append(NmsCase("classes", ys, 4, classes=[1, 3]))
        out.append(NmsCase("agnostic", ys, 4, agnostic=True))
        kept = max(_kept(NmsCase("probe", ys, 4)))
        for md in (1, kept, kept + 1):
            out.append(NmsCase(f"max_det-{md}(kept {kept})", ys, 4, max_det=md))
    elif group == "max_nms":
        m = 30208
        y = cluster_pred(1, m, 2, F32, 500, None, (0, 1), ladder=True)
        score, cl = y[0, 4:].max(0)
        order = torch.sort(score, descending=True, stable=True)[1]
        iso = {29999: (1000.0, 8.0), 30000: (1100.0, 8.0), 30100: (1200.0, 8.0)}     # rank -> the isolated box's centre
        for rank, (cx, cy) in iso.items():
            y[0, :4, order[rank]] = torch.tensor([cx, cy, 8.0, 8.0])
        out.append(NmsCase("30208-isolated-rank-30100-dropped", y, 2))
        y2 = y.clone()
        a, b = int(order[30100]), int(order[100])             # the same box with the score of rank 100: inside the cut
        ca, cb = 4 + int(cl[a]), 4 + int(cl[b])
        y2[0, ca, a], y2[0, cb, b] = y[0, cb, b], y[0, ca, a]
        out.append(NmsCase("30208-isolated-rank-100-kept", y2, 2))
    elif group == "capacity":
        y = cluster_pred(1, 2049, 64, F32, 600, None, multi=True, nclus=2)
        out.append(NmsCase("2048x64-exact-capacity", y[:, :, :2048].contiguous(), 64, multi_label=True))
        out.append(NmsCase("2049x64-overflow", y, 64, multi_label=True))
    elif group == "chunks":
        m = 65793
        y = cluster_pred(2, m, 1, HF, 700, [300, 290], (0,))
        y[:, 4, 65536:] = 0.0
        y[:, 4, [65540, 65700, 65791, 65792]] = 0.5          # candidates behind chunk 256, the last anchor included
        y[0, 4, :256] = 0.0
        y[0, 4, [0, 255]] = 0.75
        out.append(NmsCase("65793-f16-258-chunks", y, 1))
    elif group == "nonfinite":
        for d in (F32, HF, BF):
            y = cluster_pred(2, 257, 3, d, 800, [100, 90], (0, 2)).float()
            nan, inf = float("nan"), float("inf")
            y[0, 4:, 5] = torch.tensor([nan, 0.9, 0.1])       # a NaN class score next to a passing one
            y[0, 4:, 6] = torch.tensor([0.9, 0.8, nan])
            y[0, 4:, 7] = nan                                 # an all-NaN anchor
            y[0, 4:, 8] = torch.tensor([inf, 0.5, 0.1])
            y[1, 4:, 9] = torch.tensor([-inf, 0.6, -inf])
            y[1, 4:, 10] = torch.tensor([inf, inf, nan])
            y[1, 4:, 256] = torch.tensor([0.5, nan, 0.7])
            y[:, 0, 5:11] += 900.0                            # away from the clusters: nothing suppresses them
            y[:, 1, 5:11] = 40.0 + 80.0 * torch.arange(6)
            for ml in (False, True):
                out.append(NmsCase(f"nonfinite-{str(d)[6:]}-multi{int(ml)}", y.to(d), 3, multi_label=ml))
    elif group == "fma":
        boxes, thr = fma_pair()
        b = torch.from_numpy(boxes)
        y = torch.zeros(1, 5, 2)
        y[0, :4] = _xywh(b)
        y[0, 4] = torch.tensor([0.9, 0.8])
        out.append(NmsCase("fma-pair", y, 1, conf_thres=0.05, iou_thres=thr))
    else:
        raise KeyError(group)
    return out


NMS_GROUPS = ("compaction", "images", "ties", "options", "max_nms", "capacity", "chunks", "nonfinite", "fma")


# ====================================================================================================== val_select
class SelCase:
    def __init__(self, name, y, nc, conf, top_k):
        self.name, self.y, self.nc, self.conf, self.top_k = name, y, nc, conf, top_k


def sel_boxes(n, m):
    """box columns that carry the anchor index at values exact in bf16: cx = a % 128, cy = a // 128, w = a % 7 + 1, h = (a % 5) / 2"""
    a = torch.arange(m)
    return torch.stack([(a % 128).float(), (a // 128).float(), (a % 7 + 1).float(), (a % 5).float() / 2]).unsqueeze(0).repeat(n, 1, 1)


def sel_sets(y, nc, conf):
    """-> dict of float64 / bool tensors: lo, hi (N, nc, M); L, H, must, maybe, drop_nan, class_und, first (N, M)"""
    dtype = y.dtype
    x = y[:, 4:4 + nc].double()
    nan = torch.isnan(x).any(1)
    x = torch.where(nan.unsqueeze(1), torch.zeros_like(x), x)
    s = torch.sigmoid(x)
    e = 4.0 * U24 * s
    lo, hi = round_to(s - e, dtype), round_to(s + e, dtype)
    L, H = lo.amax(1), hi.amax(1)
    cont = hi >= L.unsqueeze(1)
    fc = cont.to(torch.uint8).argmax(1, keepdim=True)        # the first contender
    same = (~cont | (x == x.gather(1, fc))).all(1)            # every contender holds one logit: one stored value, the first wins
    decided = ((lo == hi) | ~cont).all(1) | same              # or every contender's stored value is known
    first = torch.where(same, fc.squeeze(1), (cont & (lo == L.unsqueeze(1))).to(torch.uint8).argmax(1))
    key = torch.where(same, x.gather(1, fc).squeeze(1), torch.full_like(L, float("nan")))     # the one logit the score comes from
    c_t = round_to(torch.tensor(conf, dtype=F64), dtype)
    must, maybe = (L >= c_t) & ~nan, (H >= c_t) & ~nan
    return dict(lo=lo, hi=hi, L=L, H=H, cont=cont, first=first, must=must, maybe=maybe, nan=nan, class_und=~decided & maybe, conf_t=c_t, key=key, s=s.amax(1))


def select_undecided(case):
    """the undecided share of a case from the reference alone (no kernel output): class, threshold and rank"""
    st = sel_sets(case.y, case.nc, case.conf)
    n, m = st["L"].shape
    und = st["class_und"] | (st["maybe"] & ~st["must"])
    for b in range(n):
        nm, ny = int(st["must"][b].sum()), int(st["maybe"][b].sum())
        if ny <= case.top_k:
            continue
        if nm <= case.top_k:
            und[b] = True
            continue
        L, H, ok = st["L"][b], st["H"][b], st["maybe"][b]
        cut_l = torch.sort(L[ok], descending=True)[0][case.top_k - 1]
        cut_h = torch.sort(H[ok], descending=True)[0][case.top_k - 1]
        ref_order = torch.sort(torch.where(ok, st["s"][b], torch.full_like(L, -1.0)), descending=True, stable=True)[1]
        tied = st["key"][b] == st["key"][b][ref_order[case.top_k - 1]]       # one logit with the reference's last kept anchor
        und[b] |= ok & ~tied & (H >= cut_l) & (L <= cut_h) & ((L < H) | (cut_l < cut_h))
    return float(und.sum()) / (n * m)


def check_select(case, got_rows, got_count):
    """got_rows fp32 [N][top_k][6] = cx, cy, w, h, cls, score; got_count [N] -> the undecided share (see the module docstring)"""
    y, nc, top_k = case.y, case.nc, case.top_k
    st = sel_sets(y, nc, case.conf)
    n, m = st["L"].shape
    rows, cnt = got_rows.detach().cpu(), got_count.detach().cpu().to(torch.int64)
    assert tuple(rows.shape) == (n, top_k, 6) and rows.dtype == F32, (case.name, rows.shape, rows.dtype)
    what = f"val_select {case.name}"
    _tally("post_select", rows.numel())
    und = st["class_und"] | (st["maybe"] & ~st["must"])
    boxes = y[:, :4].float()
    errs = []

    def bad(b, r, col, msg):
        errs.append(f"    image {b} row {r} column {col}: {msg}")

    for b in range(n):
        k = int(cnt[b])
        if not 0 <= k <= top_k:
            bad(b, "-", "count", f"count {k} outside [0, {top_k}]")
            continue
        tail = bits(rows[b, k:]) != 0
        for r, c in tail.nonzero()[:8].tolist():
            bad(b, k + r, c, f"past the count {k} but {float(rows[b, k + r, c])!r}, not +0.0")
        g = rows[b, :k]
        anc = (g[:, 0] + 128.0 * g[:, 1]).to(torch.int64)
        okr = (anc >= 0) & (anc < m) & (g[:, 0] == g[:, 0].round()) & (g[:, 1] == g[:, 1].round())
        for r in (~okr).nonzero().flatten()[:8].tolist():
            bad(b, r, "0..1", f"box columns {g[r, :2].tolist()} name no anchor")
        if not bool(okr.all()):
            continue
        cp = bits(g[:, :4]) != bits(boxes[b][:, anc].t())
        for r, c in cp.nonzero()[:8].tolist():
            bad(b, r, c, f"box copy {float(g[r, c])!r}, the anchor {int(anc[r])} holds {float(boxes[b, c, anc[r]])!r}")
        if len(set(anc.tolist())) != k:
            bad(b, "-", "0..1", "an anchor is reported twice")
            continue
        cls, scv = g[:, 4].to(torch.int64), g[:, 5].double()
        cls_ok = (g[:, 4] == cls.float()) & (cls >= 0) & (cls < nc)
        for r in (~cls_ok).nonzero().flatten()[:8].tolist():
            bad(b, r, 4, f"class {float(g[r, 4])!r} of anchor {int(anc[r])} is no class id")
        if not bool(cls_ok.all()):
            continue
        lo_g, hi_g = st["lo"][b][cls, anc], st["hi"][b][cls, anc]
        for r in range(k):
            a = int(anc[r])
            if bool(st["nan"][b, a]):
                bad(b, r, 4, f"anchor {a} has a NaN class logit and must be dropped")
                continue
            if not bool(st["maybe"][b, a]):
                bad(b, r, 5, f"anchor {a} kept, but its largest possible score {float(st['H'][b, a])!r} < conf_T {float(st['conf_t'])!r}")
            if not bool(st["cont"][b, cls[r], a]):
                bad(b, r, 4, f"class {int(cls[r])} of anchor {a} cannot hold the maximum (upper {float(hi_g[r])!r} < best lower {float(st['L'][b, a])!r})")
            elif not bool(st["class_und"][b, a]) and int(cls[r]) != int(st["first"][b, a]):
                bad(b, r, 4, f"class {int(cls[r])} of anchor {a}, the first maximum is class {int(st['first'][b, a])}")
            if not (float(lo_g[r]) <= float(scv[r]) <= float(hi_g[r]) and float(scv[r]) >= float(st["L"][b, a])):
                bad(b, r, 5, f"score {float(scv[r])!r} of anchor {a} outside [{float(max(lo_g[r], st['L'][b, a]))!r}, {float(hi_g[r])!r}]")
        got_set = torch.zeros(m, dtype=torch.bool)
        got_set[anc] = True
        nm, ny = int(st["must"][b].sum()), int(st["maybe"][b].sum())
        if ny <= top_k:
            if k and not bool((anc[1:] > anc[:-1]).all()):
                bad(b, int((anc[1:] <= anc[:-1]).nonzero()[0]) + 1, "0..1", "at most top_k anchors pass: the rows must ascend by anchor")
            for a in (st["must"][b] & ~got_set).nonzero().flatten()[:8].tolist():
                bad(b, "-", 5, f"anchor {a} (block {a // 256}) must be kept: its smallest possible score {float(st['L'][b, a])!r} >= conf_T")
        elif nm > top_k:
            if k != top_k:
                bad(b, "-", "count", f"{nm} anchors must pass, count {k} != top_k {top_k}")
                continue
            for r in range(k - 1):
                if not (scv[r] > scv[r + 1] or (scv[r] == scv[r + 1] and anc[r] < anc[r + 1])):
                    bad(b, r + 1, 5, f"order: score {float(scv[r + 1])!r} anchor {int(anc[r + 1])} after score {float(scv[r])!r} anchor {int(anc[r])}")
            s_k, a_k = float(scv[-1]), int(anc[-1])
            idx = torch.arange(m)
            dropped = st["maybe"][b] & ~got_set
            L, H = st["L"][b], st["H"][b]
            tied = st["key"][b] == st["key"][b, a_k]           # the score comes from the same logit: equal, whatever it is
            wrong = dropped & st["must"][b] & torch.where(tied, idx < a_k, (L > s_k) | ((L == s_k) & (idx < a_k)))
            for a in wrong.nonzero().flatten()[:8].tolist():
                bad(b, "-", 5, f"anchor {a} (block {a // 256}) dropped with smallest possible score {float(L[a])!r}, the last kept row has {s_k!r} (anchor {a_k})")
            und[b] |= dropped & ~wrong & ~tied & ((H > s_k) | ((H == s_k) & (idx < a_k)))
        else:
            und[b] = True                                     # between the two counts the path itself is open
    if errs:
        _fail("post_select", [f"{what} [post_select]: {len(errs)} findings"] + errs[:48], len(errs))
    share = float(und.sum()) / (n * m)
    UNDECIDED[0] = max(UNDECIDED[0], share)
    if share > UNDECIDED_CAP:
        _fail("post_select", [f"{what} [post_select]: cannot tell: {int(und.sum())} of {n * m} anchors undecided ({100 * share:.3f} % > 0.5 %)"])
    return share


def select_emul(y, nc, conf, top_k, mut=None):
    """the kernel's selection in T arithmetic on the CPU -> rows, counts.  mut: gt | conf_raw | last_max | tie_high | nan_skip"""
    dtype = y.dtype
    n, _, m = y.shape
    rows = torch.zeros(n, top_k, 6)
    counts = torch.zeros(n, dtype=torch.int32)
    c_t = float(conf) if mut == "conf_raw" else float(torch.tensor(conf).to(dtype))
    for b in range(n):
        x = y[b, 4:4 + nc].float()
        s = torch.sigmoid(x).to(dtype).float()                # (nc, M)
        nan = torch.isnan(s).any(0)
        s = torch.where(torch.isnan(s), torch.full_like(s, float("-inf")), s)
        if mut == "last_max":
            best, ci = s.flip(0).max(0)
            ci = nc - 1 - ci
        else:
            best, ci = s.max(0)
        keep = (best > c_t) if mut == "gt" else (best >= c_t)
        if mut != "nan_skip":
            keep &= ~nan
        idx = keep.nonzero().flatten()
        if idx.numel() > top_k:
            sc_ = best[idx]
            if mut == "tie_high":
                o = torch.from_numpy(np.lexsort((-idx.numpy(), -sc_.numpy())).copy())
            else:
                o = torch.sort(sc_, descending=True, stable=True)[1]
            idx = idx[o[:top_k]]
        k = idx.numel()
        rows[b, :k, :4] = y[b, :4, idx].float().t()
        rows[b, :k, 4], rows[b, :k, 5] = ci[idx].float(), best[idx]
        counts[b] = k
    return rows, counts


def _logit_for(score_t, dtype):
    """a logit of T whose sigmoid is decided and rounds to the T value score_t"""
    x0 = float(np.log(score_t / (1.0 - score_t)))
    cand = torch.tensor([x0]).to(dtype)
    step = float(ulp(torch.tensor(x0, dtype=F64), dtype))
    for k in range(-40, 41):
        x = torch.tensor([x0 + k * step / 4]).to(dtype)
        s = torch.sigmoid(x.double())
        lo, hi = round_to(s - 4 * U24 * s, dtype), round_to(s + 4 * U24 * s, dtype)
        if float(lo) == float(hi) == score_t:
            return float(x)
    raise RuntimeError(f"no logit of {dtype} gives the score {score_t}, nearest {float(cand)}")


@functools.lru_cache(maxsize=None)
def select_cases(dtype):
    out = []
    for m in (1, 255, 256, 257, 2100):
        for nc in (1, 80):
            for n in (1, 3):
                g = torch.Generator().manual_seed(1000 + 7 * m + nc + n)
                y = torch.cat([sel_boxes(n, m), torch.randn(n, nc, m, generator=g) * 1.5 - (2.5 if nc > 1 else 0.5)], 1)
                if n == 3:
                    y[1, 4:] = -9.0                           # an image without a survivor, in the middle
                y = y.to(dtype)
                for top_k in (1, 7, 100, max(m, 128)):
                    out.append(SelCase(f"M{m}-nc{nc}-N{n}-k{top_k}", y, nc, 0.25 if nc > 1 else 0.5, top_k))
    # survivor counts of exactly top_k and top_k + 1: logits +-4, far from the threshold, every score distinct and decided
    for surv in (7, 8):
        y = torch.cat([sel_boxes(2, 300), torch.full((2, 3, 300), -4.0)], 1)
        pos = torch.tensor([3, 64, 100, 255, 256, 257, 299, 280][:surv])
        y[0, 4 + 1, pos] = 1.0 + torch.arange(surv).float() * 0.25
        y[1, 4 + 2, pos[:3]] = 2.0
        out.append(SelCase(f"survivors-{surv}-top_k-7", y.to(dtype), 3, 0.5, 7))
    # equal logits straddling the cut: nine anchors share the top_k-th score; decided, the lower anchors win
    y = torch.cat([sel_boxes(1, 600), torch.full((1, 2, 600), -4.0)], 1)
    y[0, 4, [10, 300, 511]] = 3.0
    y[0, 5, [5, 20, 255, 256, 257, 400, 512, 513, 599]] = 1.5
    out.append(SelCase("equal-logits-straddle-top_k-7", y.to(dtype), 2, 0.5, 7))
    # logit 0 at conf 0.5: the score is exactly 0.5 and >= keeps it
    if dtype != F32:                                          # (in fp32 the interval around 0.5 leaves the threshold open)
        y = torch.cat([sel_boxes(1, 257), torch.full((1, 2, 257), -1.0)], 1)
        y[0, 4, [0, 100, 256]] = 0.0
        y[0, 5, [100]] = 0.0                                  # and the first of two equal maxima
        out.append(SelCase("logit0-conf0.5", y.to(dtype), 2, 0.5, 100))
        # a conf that rounds DOWN in T, and a score that is exactly conf_T: kept only when conf is rounded to T first
        conf = next(c for c in (0.7, 0.45, 0.35, 0.3, 0.55, 0.65) if float(torch.tensor(c).to(dtype)) < c)
        xt = _logit_for(float(torch.tensor(conf).to(dtype)), dtype)
        y = torch.cat([sel_boxes(1, 257), torch.full((1, 2, 257), -3.0)], 1)
        y[0, 4, [1, 255, 256]] = xt
        y[0, 5, [7]] = 4.0
        out.append(SelCase(f"conf{conf}-rounds-down", y.to(dtype), 2, conf, 100))
    # the NaN cases of the NMS: next to a passing score, all NaN, with +-inf
    nan, inf = float("nan"), float("inf")
    for top_k in (100, 3):
        y = torch.cat([sel_boxes(2, 257), torch.full((2, 3, 257), -3.0)], 1)
        y[0, 4:, 5] = torch.tensor([nan, 2.0, -1.0])
        y[0, 4:, 6] = torch.tensor([2.0, 1.0, nan])
        y[0, 4:, 7] = nan
        y[0, 4:, 8] = torch.tensor([inf, 0.5, 0.1])
        y[0, 4:, 9] = torch.tensor([-inf, 1.0, -inf])
        y[0, 4:, 256] = torch.tensor([1.25, 1.0, 0.0])
        y[1, 4:, 0] = torch.tensor([inf, inf, nan])
        y[1, 4:, [60, 70, 80, 90]] = torch.tensor([[0.5, 1.5, 2.5, 3.5], [0.0] * 4, [-1.0] * 4])
        y[1, 4:, 256] = torch.tensor([0.5, nan, 3.0])
        out.append(SelCase(f"nonfinite-k{top_k}", y.to(dtype), 3, 0.5, top_k))
    return out


# ====================================================================================================== val_match
class MatchCase:
    def __init__(self, name, rows, count, gts, thr, nc, skip=False, start=None):
        self.name, self.rows, self.count, self.gts, self.thr, self.nc, self.skip = name, rows, count.to(torch.int32), gts, thr, nc, skip
        self.start = torch.zeros(5 + 4 * nc, dtype=torch.int64) if start is None else start

    @property
    def gt(self):
        live = [g for g in self.gts if g.shape[0]]
        return (torch.cat(live) if live else torch.zeros(0, 5)).float().contiguous()

    @property
    def off(self):
        return torch.tensor(np.concatenate([[0], np.cumsum([g.shape[0] for g in self.gts])]), dtype=torch.int32)


def match_expect(case, fn=None):
    """-> (counters int64, status): the oracle on every image with at most 1024 targets, on top of the starting counters"""
    import emulated_ops as emu
    fn = fn or emu.val_match
    keep = [i for i, g in enumerate(case.gts) if g.shape[0] <= VAL_MAX_GT]     # a skipped image contributes nothing
    want = case.start.clone()
    if keep:
        sub = MatchCase(case.name, case.rows[keep], case.count[keep], [case.gts[i] for i in keep], case.thr, case.nc, case.skip)
        fn(sub.rows, sub.count, sub.gt, sub.off, sub.thr, sub.nc, sub.skip, want, None)
    return want, int(len(keep) < len(case.gts))


def check_match(case, got_ctr, got_status, want=None):
    want, status = want if want is not None else match_expect(case)
    what = f"val_match {case.name}"
    _tally("post_match", want.numel())
    gs = int(torch.as_tensor(got_status).reshape(-1)[0])
    if gs != status:
        _fail("post_match", [f"{what} [post_match]: status {gs}, want {status}"])
    got = got_ctr.detach().cpu()
    if not torch.equal(got, want):
        nc = case.nc
        names = ["total_pred", "total_gt", "tp", "fp", "fn"] + [f"class_{k}[{c}]" for k in ("tp", "fp", "fn", "gt") for c in range(nc)]
        badi = (got != want).nonzero().flatten().tolist()
        _fail("post_match", [f"{what} [post_match]: {len(badi)} counters differ (counter: got, want, start)"] +
              [f"    {names[i]}: {int(got[i])}, {int(want[i])}, {int(case.start[i])}" for i in badi[:32]], len(badi))


def match_emul(rows, count, gt, gt_off, thr, nc, skip, counters, status, mut=None):
    """MetricCounters.update restated with mutation switches: tie_last | thr_float | totals_n0 | reuse | cls_round"""
    from oracle.postproc import box_iou_batch
    add = torch.zeros_like(counters)
    c_tp, c_fp, c_fn, c_gt = 5, 5 + nc, 5 + 2 * nc, 5 + 3 * nc

    def ids(t):
        return [int(v) for v in (t.round() if mut == "cls_round" else t).long()]

    for b in range(rows.shape[0]):
        t = gt[int(gt_off[b]):int(gt_off[b + 1])]
        p = rows[b, :int(count[b]), :5]
        n, m = p.shape[0], t.shape[0]
        if (n == 0 and m == 0) or (m == 0 and skip):
            continue
        pc, tc = ids(p[:, 4]) if n else [], ids(t[:, 4]) if m else []
        if n == 0:
            add[4] += m
            if mut == "totals_n0":
                add[1] += m
            for c in tc:
                if 0 <= c < nc:
                    add[c_fn + c] += 1
                    add[c_gt + c] += 1
            continue
        if m == 0:
            add[3] += n
            for c in pc:
                if 0 <= c < nc:
                    add[c_fp + c] += 1
            continue
        iou = box_iou_batch(p[:, :4].float(), t[:, :4].float())
        taken, tp = set(), 0
        for i in range(n):
            best, bj = np.float32(0.0), -1
            for j in range(m):
                if (j in taken and mut != "reuse") or pc[i] != tc[j]:
                    continue
                v = np.float32(iou[i, j])
                if v > best or (mut == "tie_last" and v == best and v > 0):
                    best, bj = v, j
            hit = bj >= 0 and ((best >= np.float32(thr)) if mut == "thr_float" else (float(best) >= thr))
            if hit:
                tp += 1
                taken.add(bj)
            if 0 <= pc[i] < nc:
                add[(c_tp if hit else c_fp) + pc[i]] += 1
        add[0] += n
        add[1] += m
        add[2] += tp
        add[3] += n - tp
        add[4] += m - len(taken)
        for j in range(m):
            if 0 <= tc[j] < nc:
                add[c_gt + tc[j]] += 1
                if j not in taken:
                    add[c_fn + tc[j]] += 1
    counters += add


def _gts(g, m, nc, cols=6):
    """m targets on a grid 40 px apart (no two overlap), sides 24 .. 32 in quarter pixels, classes 0 .. nc - 1"""
    i = torch.arange(m)
    return torch.stack([20 + 40.0 * (i % cols), 20 + 40.0 * (i // cols), 24 + torch.randint(0, 33, (m,), generator=g) * 0.25,
                        24 + torch.randint(0, 33, (m,), generator=g) * 0.25, torch.randint(0, nc, (m,), generator=g).float()], 1)


def _preds_from(g, t, n, top_k):
    """n predictions: jittered copies of random targets (duplicates compete for one target), some with another class"""
    rows = torch.zeros(top_k, 6)
    if n and t.shape[0]:
        src = torch.randint(0, t.shape[0], (n,), generator=g)
        p = t[src].clone()
        p[:, :2] += torch.randint(-6, 7, (n, 2), generator=g).float()
        flip = torch.rand(n, generator=g) < 0.15
        p[flip, 4] += 1.0
        rows[:n, :5] = p
        rows[:n, 5] = torch.rand(n, generator=g)
    elif n:
        rows[:n, :5] = torch.cat([torch.rand(n, 4, generator=g) * 50 + 5, torch.randint(0, 3, (n, 1), generator=g).float()], 1)
    return rows


def mirror_image(lo, hi, m, cls=1.0):
    """targets `lo` < `hi` mirror each other about x = 400 (the same fp32 IoU with the prediction between them, dyadic
    coordinates); prediction 0 sits between them and must take `lo`; prediction 1 overlaps `lo` alone and so finds it
    taken (a false positive); had prediction 0 taken `hi`, prediction 1 would be a second true positive"""
    g = torch.Generator().manual_seed(lo * 1000 + hi)
    t = _gts(g, m, 4, cols=8)
    t[:, 0] += 1000.0                                         # the grid, away from the pair
    t[lo] = torch.tensor([392.0, 300.0, 32.0, 32.0, cls])
    t[hi] = torch.tensor([408.0, 300.0, 32.0, 32.0, cls])
    rows = torch.zeros(4, 6)
    rows[0, :5] = torch.tensor([400.0, 300.0, 32.0, 32.0, cls])
    rows[1, :5] = torch.tensor([384.0, 300.0, 32.0, 32.0, cls])     # IoU 0.6 with lo, 1/7 with hi
    return rows, t


@functools.lru_cache(maxsize=None)
def match_cases():
    from oracle.postproc import box_iou_batch
    out = []
    nc, top_k = 6, 12
    g = torch.Generator().manual_seed(77)
    for m in (0, 1, 63, 64, 65, 1024, 1025):
        for n in (0, 1, top_k):
            t = _gts(g, m, nc, cols=40)
            rows = _preds_from(g, t, n, top_k).unsqueeze(0)
            for skip in ((False, True) if m in (0, 65) else (False,)):
                out.append(MatchCase(f"m{m}-n{n}-skip{int(skip)}", rows, torch.tensor([n]), [t], 0.5, nc, skip))
    for lo, hi, m in ((3, 67, 70), (5, 70, 130)):             # the same lane in two slots; two lanes
        rows, t = mirror_image(lo, hi, m)
        out.append(MatchCase(f"tie-{lo}-{hi}", rows.unsqueeze(0), torch.tensor([2]), [t], 0.5, 4))
    # the threshold in double: thr = the double of the pair's fp32 IoU is a hit, the next double above a miss
    p = torch.tensor([[100.3, 50.7, 30.1, 41.9, 2.0]])
    t = torch.tensor([[103.9, 48.2, 33.3, 37.7, 2.0]])
    v = float(box_iou_batch(p[:, :4], t[:, :4])[0, 0])
    rows = torch.zeros(1, 2, 6)
    rows[0, 0, :5] = p
    out.append(MatchCase("thr-equal-hit", rows, torch.tensor([1]), [t], v, 4))
    out.append(MatchCase("thr-next-double-miss", rows, torch.tensor([1]), [t], float(np.nextafter(v, 2.0)), 4))
    # class ids outside [0, nc): -1, nc, and 2.7 (truncated to 2 on both sides, so 2.7 matches 2)
    t = _gts(g, 6, 4)
    t[:, 4] = torch.tensor([-1.0, 4.0, 2.7, 2.0, -0.5, 3.0])
    rows = torch.zeros(1, 8, 6)
    rows[0, :6, :5] = t
    rows[0, :6, 4] = torch.tensor([-1.0, 4.0, 2.0, 2.7, 0.0, 3.5])
    start = torch.arange(5 + 4 * 4, dtype=torch.int64) * 1000 + 7      # counters that start non-zero
    out.append(MatchCase("class-ids-nonzero-start", rows, torch.tensor([6]), [t], 0.5, 4, False, start))
    # 33 images mixing all of the above
    nc, top_k = 5, 10
    rows, count, gts = [], [], []
    sizes = [0, 1, 63, 64, 65, 0, 130, 1025, 7, 200, 1024] + [int(v) for v in torch.randint(0, 90, (22,), generator=g)]
    for b, m in enumerate(sizes):
        n = (0, 1, top_k, 5)[b % 4] if b != 5 else 0          # image 5: no prediction and no target
        t = _gts(g, m, nc, cols=40)
        if b % 7 == 3 and m:
            t[0, 4] = (-1.0, float(nc), 2.7)[b % 3]
        r = _preds_from(g, t, n, top_k)
        if b == 12:
            r4, t = mirror_image(3, 67, 70)
            r[:4], n = r4, 2
        rows.append(r), count.append(n), gts.append(t)
    for skip in (False, True):
        out.append(MatchCase(f"33-images-skip{int(skip)}", torch.stack(rows), torch.tensor(count), gts, 0.5, nc, skip,
                             torch.full((5 + 4 * nc,), 3, dtype=torch.int64)))
    return out


def report():
    lines = ["[strict_post] exact classes, comparisons / elements per family:"]
    lines += [f"[strict_post]   {f:16s} {v[0]:6d} {v[1]:12d}" for f, v in sorted(EXACT.items())]
    lines.append(f"[strict_post] largest undecided share of a post_select case: {100 * UNDECIDED[0]:.4f} % (cap 0.5 %)")
    return "\n".join(lines)
