"""The NaN / infinity propagation rule for the kernels between the image and the logits (dense, stem and depthwise
convolutions with their gradients and fused epilogues, the BatchNorm passes, attention), on top of strict_compare.py (its
StrictMismatch and failure histograms) and strict_move.bits() (bit comparison with every NaN mapped to one value).  Shared by
tests/test_strict_nonfinite_cpu.py (the proof of the rule on CPU stand-ins, honest and leaky) and tests/test_gpu_nonfinite.py.

One launch is run on finite inputs (`clean`) and again with a few input elements replaced (`poisoned`).  `dep` is the set
of output elements that really depend on a replaced element.  It never comes from the kernel: it is the float64 reference
operation on indicator tensors,
    dep = ref_op(indicator(poisoned operand), ones_like(other operand)) > 0
(strict_compare.conv_ref / dgrad_ref / wgrad_ref with `groups`, strict_attention's forward / backward structure through
attention_dep(), 'the whole channel' for BatchNorm), united with the poisoned elements of the operands that are added
element for element (acc_into, acc2, a residual).  assert_propagates() then asserts

    outside dep   poisoned == clean bit for bit: one leaked factor (a neighbouring channel, a padding tap, a clamped row, a
                  stale LDS slot cancelled by a zero weight, a zero probability or a mask factor) changes bits, or turns the
                  element into NaN.  Only the launches of EXEMPT, which add with float atomics in an order that differs from
                  run to run, cannot repeat bit for bit: there the caller passes `bound`, and the tensor that takes the
                  poisoned run's values outside dep and the clean run's inside is held to the family's existing float64
                  comparison (strict_compare.assert_close / assert_stats, strict_bn's stage-wise checks);
    inside dep    kind "nan": every element is NaN;  kind "inf" (+inf and -inf in alternating positions): every element is
                  non-finite -- inf - inf is a legitimate NaN.

and refuses, as conditions on the CASE and before looking at any result, an empty dep, a dep of more than half of the output
(either half of the assertion would be vacuous) and -- require_nonzero() -- a multiplying operand with an exact zero
(0 * inf is NaN in the kernel and absent from dep).  tests/test_strict_nonfinite_cpu.py checks both for every case of the GPU
module's tables from the references alone.

assert_unmoved_by_surroundings(run) runs a launch with finite and then with NaN surroundings: everything the launch is not
supposed to read (the channels of the wider buffers outside every slice, the destination of a non-accumulating form, every
scratch buffer the API does not ask to be zeroed).  The results must be bit-identical and the guard channels still NaN.

Weight gradients: `dep` is whole rows -- "a NaN in one x channel means exactly dw[:, ci] for the taps that exist, in one dy channel
exactly dw[co]" -- because tests/nonfinite_cases.positions() gives each poisoned channel the 2 x 2 pixel block in the middle of the map.
With edge pixels alone the answer depends on the masking idiom: k_wgrad2 (3x3 stride 1), k_stem_wgrad and k_dw3x3_wgrad_strip
read an output pixel past a tile tail, like the padding of x, as a ZERO RECORD, so a tap that pairs the poisoned element only with
something that is not there is 0 x NaN = NaN where torch.nn.grad.conv2d_weight has an empty sum (MI355X, 2026-10-21: 440 of 57 024
elements of dw 72 -> 88 on a 7 x 11 map, all in the poisoned row dw[:, 71]; 64 of 864 in the stem's dw[:, 1]; 1 - 2 per depthwise
case).  The spurious NaN never leaves a row that is poisoned by right; found_inf and the skipped step are the same either way.

OBSERVED_GPU below: the table tests/test_gpu_nonfinite.py printed on the MI355X.

Counters (LAUNCHES, per family: launches, elements compared bit for bit, elements inside dep, launches under the exemption)
are printed by the GPU module when it finishes: report()."""
import torch

import strict_compare as sc
import strict_move as sm
from strict_compare import StrictMismatch  # noqa: F401  (re-exported for the tests)

# the launches that are NOT compared bit for bit outside dep, and why: float atomics only
EXEMPT = {
    "conv_stats": "statistics epilogue of the MFMA / stem forward kernels: atomicAdd into the [8][2][C] accumulator (csrc/conv_dev.h)",
    "depthwise_stats": "statistics epilogue of the depthwise forward: atomicAdd into the [8][2][C] accumulator (csrc/dwconv.hip)",
    "generic_wgrad": "weight gradient of the generic VALU kernels: atomicAdd into the packed matrix (csrc/conv_generic.hip)",
    "fp32_wgrad": "weight gradient of the fp32 kernels: atomicAdd into the packed matrix (csrc/conv_f32.hip)",
    "wgrad_atomics": "wgrad algo 3, the first MFMA design: atomicAdd into one matrix (csrc/conv_mfma.hip)",
    "bn_acc": "BatchNorm's accumulator path: bn_stats_acc / bn_bwd_reduce_acc add with atomicAdd (csrc/elementwise.hip), and "
              "every coefficient and output of that path is formed from those sums",
}
KINDS = ("nan", "inf")
OBSERVED_GPU = """MI355X, tests/test_gpu_nonfinite.py, 2026-10-21: 218 tests in 10 s; 4 378 output tensors of poisoned launches compared (1 222 under the
exemption), 61 M elements bit-equal outside dep, 2.9 M NaN / non-finite inside; 723 launch pairs with NaN surroundings, 24 M elements bit-equal,
8.3 M guard elements still NaN; no kernel leaked or swallowed a NaN / Inf, none was changed"""
LAUNCHES = {}          # family -> [launches, elements compared bit for bit, elements inside dep, launches under the exemption]
SURROUNDINGS = {}      # family -> [launch pairs, elements compared bit for bit, guard elements still NaN]


class Refused(ValueError):
    """the case cannot show what it is meant to show (a condition on the case, not a measurement)"""


def indicator(shape, positions):
    """float64 zeros of `shape` with 1 at every position"""
    t = torch.zeros(tuple(shape), dtype=torch.float64)
    for p in positions:
        t[tuple(p)] = 1.0
    return t


def poison(t, positions, kind):
    """copy of `t` with the positions replaced: "nan": NaN; "inf": +inf, -inf, +inf, ... in the order given"""
    assert kind in KINDS
    t = t.clone()
    for i, p in enumerate(positions):
        t[tuple(p)] = float("nan") if kind == "nan" else float("inf") * (1 - 2 * (i % 2))
    return t


def require_nonzero(what, **operands):
    """the multiplying operands of a case (weights; q, k, v; gamma) hold no exact zero"""
    for name, t in operands.items():
        z = int((t.detach().double() == 0).sum())
        if z:
            raise Refused(f"{what}: {name} holds {z} exact zero(s): 0 * inf would make dep wrong")


def fix_zeros(t, value=2.0 ** -6):
    """a seeded tensor with its (rare: f16 underflow) exact zeros replaced, so that require_nonzero holds by construction"""
    return torch.where(t == 0, torch.full_like(t, value), t)


def check_dep(dep, what):
    """the two refusal conditions on dep alone -> number of elements inside"""
    if dep.dtype != torch.bool:
        raise Refused(f"{what}: dep must be a boolean mask, got {dep.dtype}")
    inside = int(dep.sum())
    if inside == 0:
        raise Refused(f"{what}: dep is empty: nothing would have to become non-finite")
    if 2 * inside > dep.numel():
        raise Refused(f"{what}: dep covers {inside} of {dep.numel()} elements, more than half: 'outside dep' would be vacuous")
    return inside


def conv_dep(x_ind, w_shape, k, s, groups=1):
    """forward: output elements that depend on the marked elements of x (weights all ones)"""
    return sc.conv_ref(x_ind, torch.ones(tuple(w_shape), dtype=torch.float64), k, s, groups)[0] > 0


def conv_dep_w(x_shape, w_ind, k, s, groups=1):
    """forward: output elements that depend on the marked weights"""
    return sc.conv_ref(torch.ones(tuple(x_shape), dtype=torch.float64), w_ind, k, s, groups)[0] > 0


def dgrad_dep(dy_ind, w_shape, in_shape, k, s, groups=1):
    return sc.dgrad_ref(dy_ind, torch.ones(tuple(w_shape), dtype=torch.float64), in_shape, k, s, groups)[0] > 0


def wgrad_dep(x_ind, dy_ind, w_shape, k, s, groups=1):
    """x_ind or dy_ind may be a shape (then: all ones)"""
    x = x_ind if torch.is_tensor(x_ind) else torch.ones(tuple(x_ind), dtype=torch.float64)
    dy = dy_ind if torch.is_tensor(dy_ind) else torch.ones(tuple(dy_ind), dtype=torch.float64)
    return sc.wgrad_ref(x, dy, w_shape, k, s, groups=groups)[0] > 0


def attention_dep(b, t, dk, dh, q_rows=(), k_rows=(), v_elems=(), do_elems=(), dvp_elems=()):
    """Dependency sets of softmax attention over B = image * heads + head problems of T tokens, read off the float64
    reference of strict_attention.py (forward(): s = scale q k^T, P = softmax(s), o = P v, lse; backward(): dP = dO v^T,
    D_i = dO_i . o_i -- or sum_j P_ij dP_ij --, dS = P (dP - D) scale, dQ = dS k, dK = dS^T q, dV = P^T dO + d_vp):
        P_ij, lse_i   q_i and every k of the problem (the softmax of row i; a score sums over all components of q_i and k_j)
        o_id          P_i. and component d of every v           (o = P v keeps the component)
        dS_ij         P_i., dO_i, every v (through dP and D_i, which sum over the components)
        dQ_i          dS_i. and every k            -> q_i, dO_i, every k, every v; all components
        dK_j          every dS_ij and q_i          -> every q, dO, k, v of the problem; all components
        dV_jd         every P_ij, component d of every dO_i, d_vp_jd -> every q, k (all components); dO: its component; NOT v
    Nothing crosses from one (image, head) to another.  tests/test_strict_nonfinite_cpu.py confirms every entry by perturbing
    the float64 reference's inputs.  *_rows: (problem, token); *_elems: (problem, token, component).
    -> dict of boolean masks: lse (B, T), o and dv (B, T, dh), dq and dk (B, T, dk)."""
    def rows(pairs):
        m = torch.zeros(b, t, dtype=torch.bool)
        for e in pairs:
            m[e[0], e[1]] = True
        return m

    def comps(elems):
        m = torch.zeros(b, t, dh, dtype=torch.bool)
        for p, i, d in elems:
            m[p, i, d] = True
        return m
    rq, rk, rv, rdo = rows(q_rows), rows(k_rows), rows(v_elems), rows(do_elems)
    aq, ak, av, ado = (m.any(1, keepdim=True).expand(b, t) for m in (rq, rk, rv, rdo))
    cv, cdo = (comps(e).any(1, keepdim=True).expand(b, t, dh) for e in (v_elems, do_elems))     # the components, for every token
    return {"lse": rq | ak, "o": (rq | ak).unsqueeze(-1).expand(b, t, dh) | cv,
            "dq": (rq | rdo | ak | av).unsqueeze(-1).expand(b, t, dk).clone(), "dk": (aq | ado | ak | av).unsqueeze(-1).expand(b, t, dk).clone(),
            "dv": (aq | ak).unsqueeze(-1).expand(b, t, dh) | cdo | comps(dvp_elems)}


def _count(family, n_bits, n_dep, exempt):
    o = LAUNCHES.setdefault(family, [0, 0, 0, 0])
    o[0], o[1], o[2], o[3] = o[0] + 1, o[1] + n_bits, o[2] + n_dep, o[3] + int(exempt)


def assert_propagates(clean, poisoned, dep, kind, what, family, bound=None):
    """clean, poisoned: results of one launch on finite / poisoned inputs (same shape and dtype, any device); dep: boolean
    CPU tensor of that shape.  bound: only for the families of EXEMPT -- called with the tensor 'poisoned outside dep, clean
    inside'; it applies the family's float64 comparison and raises StrictMismatch."""
    assert kind in KINDS, kind
    clean, poisoned = clean.detach().cpu(), poisoned.detach().cpu()
    assert clean.shape == poisoned.shape == dep.shape and clean.dtype == poisoned.dtype, \
        (what, tuple(clean.shape), tuple(poisoned.shape), tuple(dep.shape), clean.dtype, poisoned.dtype)
    inside = check_dep(dep, what)
    if not bool(torch.isfinite(clean.double()).all()):
        raise Refused(f"{what}: the clean launch is not finite: its inputs are not the finite case they are meant to be")
    exempt = family in EXEMPT
    if exempt != (bound is not None):
        raise Refused(f"{what}: family {family!r} is {'in' if exempt else 'not in'} EXEMPT: bound= belongs to exactly those launches")
    try:
        if exempt:
            bound(torch.where(dep, clean, poisoned))
            leak = ~dep & ~torch.isfinite(poisoned.double())              # a bound's reference may be lenient about nothing here
            if bool(leak.any()):
                sm._raise(what, family, leak, poisoned.double(), clean.double(), "outside dep are not finite")
        else:
            bad = ~dep & (sm.bits(poisoned) != sm.bits(clean))
            if bool(bad.any()):
                sm._raise(what, family, bad, poisoned.double(), clean.double(),
                          f"outside the dependency set differ bit for bit from the clean launch ({kind} leaked)")
        p64 = poisoned.double()
        lost = dep & ~(torch.isnan(p64) if kind == "nan" else ~torch.isfinite(p64))
        if bool(lost.any()):
            sm._raise(what, family, lost, p64, torch.full_like(p64, float("nan")),
                      f"inside the dependency set are {'not NaN' if kind == 'nan' else 'finite'} ({kind} swallowed)")
    except StrictMismatch as e:
        e.families = [family]
        raise
    _count(family, 0 if exempt else dep.numel() - inside, inside, exempt)


def assert_unmoved_by_surroundings(run, what, family):
    """run(hostile) -> (results, guards): results a dict name -> tensor; guards a list of (wider buffer (N, C_total, H, W),
    lo, hi): channels [lo, hi) belong to the launch.  hostile False: finite surroundings; True: NaN in everything the launch
    is not supposed to read.  Statistics accumulators that the API wants zeroed are zeroed by `run` in both."""
    calm, _ = run(False)
    wild, guards = run(True)
    assert calm.keys() == wild.keys()
    n_bits = n_guard = 0
    try:
        for name in calm:
            a, b = calm[name].detach().cpu(), wild[name].detach().cpu()
            assert a.shape == b.shape and a.dtype == b.dtype, (what, name)
            bad = sm.bits(a) != sm.bits(b)
            n_bits += a.numel()
            if bool(bad.any()):
                sm._raise(f"{what}: {name}", family, bad, b.double(), a.double(), "change when the surroundings hold NaN")
        for buf, lo, hi in guards:
            buf = buf.detach().cpu()
            gone = ~torch.isnan(buf.double())
            gone[:, lo:hi] = False
            n_guard += buf.numel() - buf[:, lo:hi].numel()
            if bool(gone.any()):
                sm._raise(f"{what}: guard channels", family, gone, buf.double(), torch.full_like(buf.double(), float("nan")),
                          "beside the slice no longer hold NaN")
    except StrictMismatch as e:
        e.families = [family]
        raise
    o = SURROUNDINGS.setdefault(family, [0, 0, 0])
    o[0], o[1], o[2] = o[0] + 1, o[1] + n_bits, o[2] + n_guard


def failing(fn):
    """-> (families, StrictMismatch) of a call expected to fail, or ([], None)"""
    try:
        fn()
    except StrictMismatch as e:
        return list(e.families), e
    return [], None


def report():
    lines = ["[strict_nonfinite] per family: launches, elements compared bit for bit outside dep, elements inside dep, launches under the exemption"]
    for fam in sorted(LAUNCHES):
        n, nb, nd, ne = LAUNCHES[fam]
        lines.append(f"[strict_nonfinite]   {fam:18s} {n:6d} {nb:12d} {nd:10d} {ne:6d}")
    lines.append("[strict_nonfinite] surroundings (NaN in everything a launch may not read): launch pairs, elements bit for bit, guard elements")
    for fam in sorted(SURROUNDINGS):
        n, nb, ng = SURROUNDINGS[fam]
        lines.append(f"[strict_nonfinite]   {fam:18s} {n:6d} {nb:12d} {ng:10d}")
    used = sorted(f for f in LAUNCHES if LAUNCHES[f][3])
    lines.append(f"[strict_nonfinite] exempt from bit equality (float atomics; held to their float64 bound instead): {used or 'none'}")
    return "\n".join(lines)
